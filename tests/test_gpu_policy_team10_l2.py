"""GPU (-m gpu): the second packed layer of the one-launch policy kernel in its constant-team-size form (10 agents; key
TUNE_POLICY_CP_TEAM, default on) against the run-time form of the same kernel (key = 0), BIT FOR BIT.  The constant form
orders L2's 160 columns by image rows, drops the six (tap, tile) units that read nothing but the zero row, pools the y-pair
of a window register-wise and stores L3's input fragments from another lane map: a unit dropped wrongly, an accumulator
started at the wrong tap, a pooled value in the wrong dword or a moved input cell changes logits."""
import numpy as np
import pytest
import torch

from gnn_pathplanning_amd import _native
from oracle import policy_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the GPU box'
    _native.lib()                      # fail loudly if libgnnpp.so is missing
    return torch.device('cuda:0')


def _net(n, k, dev, sd):
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet

    class Cfg:
        num_agents, nGraphFilterTaps, device = n, k, dev
    net = DecentralPlannerNet(Cfg()).to(dev).eval()
    net.load_state_dict(sd)
    return net


def _obs(kind, B, N, seed):
    obs = orc.synth_obs(B, N, seed=seed)
    g = torch.Generator().manual_seed(seed)
    if kind == 'binary':
        return obs                                                 # {0, 1}: the one-plane L0
    if kind == 'real':
        return obs * torch.randn(obs.shape, generator=g)           # three planes
    assert kind == 'dense'
    return torch.randn(obs.shape, generator=g)                     # every pixel set: no cell of L2's input is zero by luck


def _both(net, obs_d, L):
    """logits with key 21 = 1, 0, 1"""
    outs = []
    try:
        for team in (1, 0, 1):
            assert L.gnnpp_set_tuning(_native.TUNE_POLICY_CP_TEAM, team) == 0
            assert L.gnnpp_get_tuning(_native.TUNE_POLICY_CP_TEAM) == team
            outs.append(net.forward_logits(obs_d).clone())
    finally:
        L.gnnpp_set_tuning(_native.TUNE_POLICY_CP_TEAM, 1)
    return outs


@pytest.mark.parametrize('B', [3, 5])
@pytest.mark.parametrize('K', [2, 3, 4])
@pytest.mark.parametrize('kind', ['binary', 'real', 'dense'])
def test_team10_l2_is_bit_identical(dev, B, K, kind):
    L = _native.lib()
    N = 10
    sd = orc.init_state_dict(K, seed=70 + K)
    net = _net(N, K, dev, sd)
    obs = _obs(kind, B, N, seed=31 + K + B)
    S = torch.from_numpy(orc.synth_gso_geometric(B, N, 20, seed=K + B)).float()
    net.addGSO(S.to(dev))
    outs = _both(net, obs.to(dev), L)
    assert torch.isfinite(outs[0]).all() and outs[0].abs().max().item() > 0
    assert torch.equal(outs[0], outs[1]), (outs[0] - outs[1]).abs().max().item()
    assert torch.equal(outs[0], outs[2])
    want = torch.stack(orc.policy_forward(sd, S, obs), 0)
    assert (outs[0].cpu() - want).abs().max().item() <= TOL * max(1.0, want.abs().max().item())


def test_team10_l2_isolated_agents(dev):
    """agents 3, 8 and 9 without neighbours (8 and 9 share the tail tile of the row-wise order)"""
    L = _native.lib()
    B, N, K = 5, 10, 3
    sd = orc.init_state_dict(K, seed=77)
    net = _net(N, K, dev, sd)
    obs = _obs('real', B, N, seed=41)
    S = torch.from_numpy(orc.synth_gso_geometric(B, N, 20, seed=4)).float()
    for a in (3, 8, 9):
        S[:, a, :] = 0
        S[:, :, a] = 0
    net.addGSO(S.to(dev))
    outs = _both(net, obs.to(dev), L)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), (outs[0] - outs[1]).abs().max().item()
    want = torch.stack(orc.policy_forward(sd, S, obs), 0)
    assert (outs[0].cpu() - want).abs().max().item() <= TOL * max(1.0, want.abs().max().item())


@pytest.mark.parametrize('N', [9, 11])
def test_other_team_sizes_keep_the_run_time_form(dev, N):
    """N = 9 and N = 11 never take the constant form: the key changes nothing, the oracle still agrees."""
    L = _native.lib()
    B, K = 3, 3
    sd = orc.init_state_dict(K, seed=62)
    net = _net(N, K, dev, sd)
    obs = _obs('real', B, N, seed=N)
    S = torch.from_numpy(orc.synth_gso_geometric(B, N, 20, seed=N)).float()
    net.addGSO(S.to(dev))
    outs = _both(net, obs.to(dev), L)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    want = torch.stack(orc.policy_forward(sd, S, obs), 0)
    assert (outs[0].cpu() - want).abs().max().item() <= TOL * max(1.0, want.abs().max().item())


def test_team10_l2_with_simulator_tail(dev):
    """The kernel with the simulator step behind it (BatchedRollout.step) at N = 10: one step, logits and next state under
    both values of the key."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    L = _native.lib()
    B, N, W = 5, 10, 20
    rng = np.random.default_rng(29)
    grids, starts, goals = [], [], []
    for _ in range(B):
        g = (rng.random((W, W)) < 0.08).astype(np.uint8)
        free = np.argwhere(g == 0)
        idx = rng.choice(len(free), size=2 * N, replace=False)
        grids.append(g); starts.append(free[idx[:N]]); goals.append(free[idx[N:]])
    grids, starts, goals = np.stack(grids), np.stack(starts), np.stack(goals)
    net = _net(N, 3, dev, orc.init_state_dict(3, seed=19))
    got = []
    try:
        for team in (1, 0):
            assert L.gnnpp_set_tuning(_native.TUNE_POLICY_CP_TEAM, team) == 0
            env = BatchedRollout(grids, starts, goals, 9, dev, tie_mode='hashed', seed=7)
            env.step(net)
            assert env._logits is not None and env._state_step == env.t            # the one-launch path was taken
            got.append((env._logits.clone(), env.pos.clone(), env.obs.clone(), env.S.clone()))
    finally:
        L.gnnpp_set_tuning(_native.TUNE_POLICY_CP_TEAM, 1)
    assert torch.isfinite(got[0][0]).all()
    for a, b in zip(got[0], got[1]):
        assert torch.equal(a, b)
