"""MI355X: the hand-built cases of tests/schedule_pool_cases.py (the case_* functions tests/test_emu_schedule_draw.py runs
under the host emulation, which executes the work-items of a workgroup one at a time) through gnnpp_schedule_draw on the
device.  The same runner, the same assertions: every array, poisoned with 0xFF bytes and set between sentinel margins, has
a twin in device memory for the length of a call; a batch equals the rows of the existing sample calls on the same
schedules and the reference-made goldens, the margins keep their bytes, and a refused call writes nothing."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expert_team_lists_cases as lc  # noqa: E402
import schedule_pool_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
GRAPHS = ['dense', 'lists']


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from gnn_pathplanning_amd import _native
    return _native.lib()


@pytest.fixture(scope='module')
def run():
    return lc.DeviceRunner('cuda:0')


@pytest.mark.parametrize('graph', GRAPHS)
@pytest.mark.parametrize('ci', sc.GOLDEN_SMALL)
def test_golden_case(lib, run, ci, graph):
    sc.case_golden(lib, 'small', ci, graph, run)


@pytest.mark.parametrize('graph', GRAPHS)
def test_golden_team_case(lib, run, graph):
    sc.case_golden(lib, 'team', sc.GOLDEN_TEAM[0], graph, run)


@pytest.mark.parametrize('graph', GRAPHS)
@pytest.mark.parametrize('N,side,steps', sc.RANDOM)
def test_random_schedules(lib, run, N, side, steps, graph):
    sc.case_random(lib, N, side, steps, graph, run)


@pytest.mark.parametrize('graph', GRAPHS)
def test_every_pick_gets_the_radius_of_its_own_case(lib, run, graph):
    sc.case_per_case_radius(lib, graph, run)


@pytest.mark.parametrize('graph', GRAPHS)
@pytest.mark.parametrize('H,W', sc.THIN)
def test_thin_map(lib, run, H, W, graph):
    sc.case_thin_map(lib, H, W, graph, run)


def test_pointer_alignment(lib, run):
    sc.case_pointer_alignment(lib, run)


@pytest.mark.parametrize('graph', GRAPHS)
@pytest.mark.parametrize('N,side', [(5, 9), (130, 40)])
def test_flagged_case_among_good_ones(lib, run, N, side, graph):
    sc.case_flagged(lib, N, side, 10, 4, graph, run)        # ten cases, the flagged one in their middle


@pytest.mark.parametrize('graph', GRAPHS)
def test_index_clamping(lib, run, graph):
    sc.case_index_clamping(lib, graph, run)


@pytest.mark.parametrize('graph', GRAPHS)
def test_two_calls_give_the_same_bytes(lib, run, graph):
    sc.case_determinism(lib, graph, run)


def test_argument_errors(lib, run):
    sc.case_argument_errors(lib, run)
