"""GPU (-m gpu): gnnpp_rollout_lists on the MI355X: the cases of tests/test_emu_rollout_lists.py plus the full
workgroup (2 x 1024 agents on a 64 x 64 map), against the lists of the oracle's dense S and against
gnnpp_team_lists_from_dense of gnnpp_rollout_gso's S, bit for bit.  Instances and runner: tests/rollout_lists_cases.py."""
import pytest
import torch

import filter_f64_cases as fc
import rollout_lists_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def bk():
    from gnn_pathplanning_amd import _native
    assert torch.cuda.is_available()
    return fc.TorchBackend(_native.lib(), torch.device('cuda:0'))


@pytest.mark.parametrize('case', lc.CASES + lc.GPU_CASES, ids=lambda c: c['name'])
def test_rollout_lists(bk, case):
    cnt = lc.run_lists_case(bk, case)
    if case['pos'].shape[1] == 1024:
        assert 1 < cnt.mean() < 200


def test_rollout_lists_errors(bk):
    lc.run_lists_errors(bk)
