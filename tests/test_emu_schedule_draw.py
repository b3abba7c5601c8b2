"""CPU: gnnpp_schedule_draw (csrc/schedule_draw_kernels.hip, compiled unmodified for the host emulation): a batch of
picked steps against the rows gnnpp_schedule_team_samples, gnnpp_schedule_team_fill_lists and gnnpp_team_lists_gather
make of the same schedules, and against what the REAL reference transformer made (tests/golden/expert_schedules*.npz).
Equality everywhere.  Statement, runner and the hand-built cases (run on the device too): tests/schedule_pool_cases.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expert_team_lists_cases as lc  # noqa: E402
import schedule_pool_cases as sc  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')
GRAPHS = ['dense', 'lists']


@pytest.fixture(scope='module')
def lib():
    import emu_lib
    return emu_lib.load()


@pytest.mark.parametrize('graph', GRAPHS)
@pytest.mark.parametrize('ci', sc.GOLDEN_SMALL)
def test_golden_case(lib, ci, graph):
    sc.case_golden(lib, 'small', ci, graph)


@pytest.mark.parametrize('graph', GRAPHS)
def test_golden_team_case(lib, graph):
    sc.case_golden(lib, 'team', sc.GOLDEN_TEAM[0], graph, most=3)


@pytest.mark.parametrize('graph', GRAPHS)
@pytest.mark.parametrize('N,side,steps', sc.RANDOM)
def test_random_schedules(lib, N, side, steps, graph):
    sc.case_random(lib, N, side, steps, graph)


@pytest.mark.parametrize('graph', GRAPHS)
def test_every_pick_gets_the_radius_of_its_own_case(lib, graph):
    sc.case_per_case_radius(lib, graph)


@pytest.mark.parametrize('graph', GRAPHS)
@pytest.mark.parametrize('H,W', sc.THIN)
def test_thin_map(lib, H, W, graph):
    sc.case_thin_map(lib, H, W, graph)


def test_pointer_alignment(lib):
    sc.case_pointer_alignment(lib)


@pytest.mark.parametrize('graph', GRAPHS)
def test_flagged_case_among_good_ones(lib, graph):
    sc.case_flagged(lib, 5, 9, 3, 1, graph)                 # (fewer than 8 cases)


@pytest.mark.parametrize('graph', GRAPHS)
def test_index_clamping(lib, graph):
    sc.case_index_clamping(lib, graph)


@pytest.mark.parametrize('graph', GRAPHS)
def test_two_calls_give_the_same_bytes(lib, graph):
    sc.case_determinism(lib, graph)


def test_argument_errors(lib):
    sc.case_argument_errors(lib)


def test_runner_with_twins_of_every_array(lib):
    """lc.DeviceRunner, which the device tests run every case through, on twins in host memory: the emulated library sees
    only the twins, and the cases hold as they do on the arrays themselves."""
    run = lc.DeviceRunner('cpu')
    sc.case_per_case_radius(lib, 'dense', run)
    sc.case_flagged(lib, 5, 9, 3, 1, 'lists', run)
    sc.case_pointer_alignment(lib, run)
    sc.case_argument_errors(lib, run)
