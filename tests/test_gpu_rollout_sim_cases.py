"""MI355X (-m gpu): the cases of tests/rollout_sim_cases.py (the ones tests/test_emu_rollout_sim.py runs under the host
emulation) through libgnnpp.so on the device -- real waves, ballots, LDS atomics and alignment -- plus what only the
device can show: the launchers' LDS branches up to the largest accepted map (requests above the default 64 KB of
dynamic LDS included), the map past the limit, and gnnpp_rollout_policy_step (N <= 16, GNNPP_PREC_FP32 and
GNNPP_PREC_SPLIT_F16) against gnnpp_policy_fwd + the separate launches, up to its own map limit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import filter_f64_cases as fc  # noqa: E402
import rollout_sim_cases as sc  # noqa: E402
from oracle import policy_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

PRECISIONS = ('fp32', 'split_f16')
POLICY_CASES = [c for c in sc.all_cases() if c['starts'].shape[1] <= 16]


@pytest.fixture(scope='module')
def bk():
    from gnn_pathplanning_amd import _native
    assert torch.cuda.is_available(), 'needs the MI355X'
    return fc.TorchBackend(_native.lib(), torch.device('cuda:0'))


_NETS = {}


def planner(bk, N, precision):
    """One eval-mode DecentralPlannerNet (K = 3) per team size and precision, shared by the tests."""
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    if (N, precision) not in _NETS:
        class Cfg:
            num_agents, nGraphFilterTaps, device, range_policy = N, 3, bk.dev, 'flag'
        Cfg.precision = precision
        net = DecentralPlannerNet(Cfg()).to(bk.dev).eval()
        net.load_state_dict(orc.init_state_dict(3, seed=9))
        _NETS[(N, precision)] = net
    return _NETS[(N, precision)]


@pytest.mark.parametrize('case', sc.all_cases(), ids=lambda c: c['name'])
def test_rollout_sim(bk, case):
    sc.run_case(bk, case)


def test_rollout_sim_map_load_paths(bk):
    """With the pointers the calls are really given, the map-load cases reach all three paths of observe_stage."""
    paths = set()
    for case in sc.map_load_cases():
        paths |= set(sc.load_paths(case, sc.SimState(bk, case).g['grid'].ptr))
    assert paths == {1, 4, 16}


@pytest.mark.parametrize('k', range(len(sc.LDS_SHAPES)), ids=['%dx%d/N%d' % s[:3] for s in sc.LDS_SHAPES])
def test_rollout_sim_lds_branches(bk, k):
    """Either side of every LDS threshold of the launchers (sc.LDS_SHAPES says which), after the small maps above: a
    limit pinned by the first call's size would refuse these."""
    sc.run_case(bk, sc.lds_cases()[k])


def test_rollout_sim_map_past_the_limit_is_unsupported(bk):
    for case in sc.unsupported_cases():
        sc.run_unsupported(bk, case)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', POLICY_CASES, ids=lambda c: c['name'])
def test_rollout_sim_policy_step(bk, case, precision):
    sc.run_policy_case(bk, case, planner(bk, case['starts'].shape[1], precision), precision)


def test_policy_step_at_its_fp32_map_limit(bk):
    """88 x 116 = 10 208 cells, the documented limit of the on-chip simulator under GNNPP_PREC_FP32: the one-launch path
    is taken (GNNPP_OK) and equals the separate launches."""
    case = sc.policy_map_cases()[0]
    assert case['grids'].shape[1:] == sc.POLICY_MAP_FITS
    sc.run_policy_case(bk, case, planner(bk, 10, 'fp32'), 'fp32')
    assert not planner(bk, 10, 'fp32').range_exceeded()


def test_policy_step_past_its_fp32_map_limit(bk):
    """83 x 123 = 10 209 cells: gnnpp_rollout_policy_step answers GNNPP_ERR_UNSUPPORTED with nothing written, and
    BatchedRollout.step falls back to gnnpp_policy_fwd + gnnpp_rollout_step with the separate route's results."""
    from gnn_pathplanning_amd._native import ERR_UNSUPPORTED
    from gnn_pathplanning_amd.rollout import BatchedRollout
    case = sc.policy_map_cases()[1]
    assert case['grids'].shape[1:] == sc.POLICY_MAP_TOO_LARGE
    net = planner(bk, 10, 'fp32')
    enc, taps, gb, aw, ab, K = net.policy_pointers()
    st = sc.SimState(bk, case, logits=True)
    st.r.currentstep, st.r.grow = 1, 0
    everything = sc.OUTPUTS['step'] + ('logits', 'pos', 'reached', 'start_step', 'end_step', 'done')
    got = st.call('step', fn=lambda r, s: bk.lib.gnnpp_rollout_policy_step(r, enc, taps, gb, aw, ab, K, net._prec(), s),
                  want_rc=ERR_UNSUPPORTED, poison=everything)
    for k in everything:
        assert (np.isnan(got[k]) if got[k].dtype.kind == 'f' else got[k] == sc.POISON).all(), k
    a = BatchedRollout(case['grids'], case['starts'], case['goals'], case['maxstep'], bk.dev)
    b = BatchedRollout(case['grids'], case['starts'], case['goals'], case['maxstep'], bk.dev)
    with torch.no_grad():
        for t in range(3):
            a.step(net)
            assert a._state_step == a.t
            if t == 0:
                b.observe(); b.gso(0)
            net.addGSO(b.S)
            b.move(logits=net.forward_logits(b.obs))
            b.observe(); b.gso()
            for name in ('pos', 'obs', 'S', 'radius', 'connected', 'reached', 'start_step', 'end_step', 'done', 'stats',
                         'flags', 'choice_count'):
                assert torch.equal(getattr(a, name), getattr(b, name)), (t, name)
