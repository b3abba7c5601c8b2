"""MI355X: the hand-built cases of tests/expert_team_lists_cases.py (the case_* functions tests/test_emu_expert_team_lists.py
runs under the host emulation, which executes the work-items of a workgroup one at a time) through
gnnpp_schedule_team_plan, gnnpp_schedule_team_fill_lists and gnnpp_team_lists_gather on the device.  The same runner, the
same assertions: every array, poisoned with 0xFF bytes (NaN, -1) and set between sentinel margins, has a twin in device
memory for the length of a call; the lists equal those of the sequential restatement's dense S and of the dense call,
the margins keep their bytes, and what a call must not write stays poison."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expert_team_lists_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from gnn_pathplanning_amd import _native
    return _native.lib()


@pytest.fixture(scope='module')
def run():
    return lc.DeviceRunner('cuda:0')


@pytest.mark.parametrize('N,side', lc.TINY_MAPS)
def test_tiny_map_where_everybody_neighbours_everybody(lib, run, N, side):
    lc.case_tiny_map_where_everybody_neighbours_everybody(lib, N, side, run)


@pytest.mark.parametrize('N', [7, 130])
def test_set_four_entries_wider_than_needed(lib, run, N):
    lc.case_set_four_entries_wider_than_needed(lib, N, run)


def test_largest_degree_exactly_cap(lib, run):
    lc.case_largest_degree_exactly_cap(lib, run)


def test_flagged_case_between_two_good_ones(lib, run):
    lc.case_flagged_case_between_two_good_ones(lib, run)


@pytest.mark.parametrize('N,side,radius0', lc.SHORT_CAPS)
def test_cap_four_below_the_need(lib, run, N, side, radius0):
    lc.case_cap_four_below_the_need(lib, N, side, radius0, run)


@pytest.mark.parametrize('name', lc.THIN_CALLS)
def test_thin_map(lib, run, name):
    lc.case_thin_map(lib, name, run)


@pytest.mark.parametrize('name', lc.THIN_SHORT_CAPS)
def test_thin_map_cap_four_below_the_need(lib, run, name):
    lc.case_thin_map(lib, name, run, short=True)


@pytest.fixture(scope='module')
def pool(lib, run):
    return lc.gather_pool(lib, run)


@pytest.mark.parametrize('name', sorted(lc.GATHERS))
def test_gather(lib, run, pool, name):
    lc.case_gather(lib, pool, lc.GATHERS[name], run)


def test_gather_clamps_an_index_out_of_range(lib, run, pool):
    lc.case_gather_clamps_an_index_out_of_range(lib, pool, run)


def test_gather_from_a_set_at_the_standard_stride(lib, run):
    lc.case_gather_from_a_set_at_the_standard_stride(lib, run)
