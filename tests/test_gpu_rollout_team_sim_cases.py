"""MI355X (-m gpu): the cases of tests/rollout_team_sim_cases.py (the ones tests/test_emu_rollout_team_sim.py runs under the
host emulation) through libgnnpp.so on the device -- real waves, ballots, barriers and alignment -- plus what only the
device can show: the team launchers' LDS requests either side of the default 64 KB of dynamic LDS and up to the largest
accepted maps (147 728 bytes for move, 96 960 for observe), and the map past the limit."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import filter_f64_cases as fc  # noqa: E402
import rollout_lists_cases as lc  # noqa: E402
import rollout_sim_cases as sc  # noqa: E402
import rollout_team_sim_cases as tsc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def bk():
    from gnn_pathplanning_amd import _native
    assert torch.cuda.is_available(), 'needs the MI355X'
    return fc.TorchBackend(_native.lib(), torch.device('cuda:0'))


@pytest.mark.parametrize('case', tsc.all_cases(), ids=lambda c: c['name'])
def test_rollout_team_sim(bk, case):
    sc.run_case(bk, case)


def test_rollout_team_sim_map_load_paths(bk):
    """With the pointers the calls are really given, the map-load cases reach all three paths of observe_stage."""
    paths = set()
    for case in tsc.map_load_cases():
        paths |= set(sc.load_paths(case, sc.SimState(bk, case).g['grid'].ptr))
    assert paths == {1, 4, 16}


@pytest.mark.parametrize('case', tsc.lists_cases(), ids=lambda c: c['name'])
def test_rollout_team_sim_lists(bk, case):
    lc.run_lists_case(bk, case)


@pytest.mark.parametrize('k', range(len(tsc.LDS_SHAPES)), ids=['%dx%d/N%d' % s[:3] for s in tsc.LDS_SHAPES])
def test_rollout_team_sim_lds_requests(bk, k):
    """Either side of the 64 KB line of the move and the observe kernel (tsc.LDS_SHAPES says which) and the largest accepted
    maps, small maps before large ones: a limit pinned by the first call's size would refuse the later ones."""
    sc.run_case(bk, tsc.lds_cases()[k])


def test_rollout_team_sim_map_past_the_limit_is_unsupported(bk):
    for case in tsc.unsupported_cases():
        sc.run_unsupported(bk, case)
