"""GPU (-m gpu): the packed one-launch policy kernel with the team size as a compile-time constant (10 agents; key
TUNE_POLICY_CP_TEAM, default on) against the two forms it must equal BIT FOR BIT: the packed kernel with a run-time team
size (TUNE_POLICY_CP_TEAM = 0) and the agents-on-columns kernel (TUNE_POLICY_CP = 0).  The constant-N form drops the 21
(tap, tile) units of its first packed layer that hold nothing but zeros; a unit dropped wrongly -- or an accumulator
started at the wrong tap -- changes logits, first of all those that depend on the image border."""
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
        return obs
    if kind == 'real':
        return obs * torch.randn(obs.shape, generator=g)
    border = torch.zeros(obs.shape[-2:])
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = 1.0          # image rows 0 and 10, columns 0 and 10
    if kind == 'border':
        return torch.randn(obs.shape, generator=g) * border
    assert kind == 'border_binary'
    return (torch.rand(obs.shape, generator=g) < 0.6).float() * border


def _forms(net, obs_d, L):
    """logits of (constant-N packed, run-time-N packed, agents on columns, constant-N packed again)"""
    outs = []
    try:
        for cp, team in ((1, 1), (1, 0), (0, 1), (1, 1)):
            assert L.gnnpp_set_tuning(_native.TUNE_POLICY_CP, cp) == 0
            assert L.gnnpp_set_tuning(_native.TUNE_POLICY_CP_TEAM, team) == 0
            assert L.gnnpp_get_tuning(_native.TUNE_POLICY_CP_TEAM) == team
            outs.append(net.forward_logits(obs_d).clone())
    finally:
        L.gnnpp_set_tuning(_native.TUNE_POLICY_CP, 1)
        L.gnnpp_set_tuning(_native.TUNE_POLICY_CP_TEAM, 1)
    return outs


@pytest.mark.parametrize('K', [2, 3, 4])
@pytest.mark.parametrize('kind', ['binary', 'real', 'border', 'border_binary', 'isolated'])
def test_team10_form_is_bit_identical(dev, K, kind):
    """N = 10, B = 3: {0, 1} observations (one-plane L0), real-valued ones (three planes), observations that live on the
    image border only, a GSO with an isolated agent; against both other forms and the oracle."""
    L = _native.lib()
    B, N = 3, 10
    sd = orc.init_state_dict(K, seed=50 + K)
    net = _net(N, K, dev, sd)
    obs = _obs('real' if kind == 'isolated' else kind, B, N, seed=17 + K)
    S = torch.from_numpy(orc.synth_gso_geometric(B, N, 20, seed=K)).float()
    if kind == 'isolated':
        S[:, 3, :] = 0
        S[:, :, 3] = 0
    net.addGSO(S.to(dev))
    outs = _forms(net, obs.to(dev), L)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), (outs[0] - outs[1]).abs().max().item()       # constant N == run-time N
    assert torch.equal(outs[0], outs[2]), (outs[0] - outs[2]).abs().max().item()       # ... == agents on columns
    assert torch.equal(outs[0], outs[3])
    want = torch.stack(orc.policy_forward(sd, S, obs), 0)
    assert (outs[0].cpu() - want).abs().max().item() <= TOL * max(1.0, want.abs().max().item())


@pytest.mark.parametrize('B,N', [(5, 9), (5, 11), (5, 12), (1, 10), (513, 10)])
def test_team10_dispatch(dev, B, N):
    """Other team sizes never take the constant-N form: the key changes nothing.  B = 1 and B = 513 at N = 10: the
    first and the last workgroup, a grid past one round of the device."""
    L = _native.lib()
    sd = orc.init_state_dict(3, seed=61)
    net = _net(N, 3, dev, sd)
    obs = _obs('real' if N % 2 else 'binary', B, N, seed=B + N)
    net.addGSO(torch.from_numpy(orc.synth_gso_geometric(B, N, 20, seed=N)).float().to(dev))
    outs = _forms(net, obs.to(dev), L)
    assert torch.isfinite(outs[0]).all()
    for o in outs[1:]:
        assert torch.equal(outs[0], o), (outs[0] - o).abs().max().item()


def test_team10_form_with_simulator_tail(dev):
    """The kernel with the simulator step behind it (BatchedRollout.step: policy + move + graph + observation in one
    launch) at N = 10: one step, logits and next state under both values of the key."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    L = _native.lib()
    B, N, W = 5, 10, 20
    rng = np.random.default_rng(23)
    grids, starts, goals = [], [], []
    for _ in range(B):
        g = (rng.random((W, W)) < 0.08).astype(np.uint8)
        free = np.argwhere(g == 0)
        idx = rng.choice(len(free), size=2 * N, replace=False)
        grids.append(g); starts.append(free[idx[:N]]); goals.append(free[idx[N:]])
    grids, starts, goals = np.stack(grids), np.stack(starts), np.stack(goals)
    net = _net(N, 3, dev, orc.init_state_dict(3, seed=9))
    got = []
    try:
        for team in (1, 0):
            assert L.gnnpp_set_tuning(_native.TUNE_POLICY_CP_TEAM, team) == 0
            env = BatchedRollout(grids, starts, goals, 9, dev, tie_mode='hashed', seed=5)
            env.step(net)
            assert env._logits is not None and env._state_step == env.t            # the one-launch path was taken
            got.append((env._logits.clone(), env.pos.clone(), env.obs.clone(), env.S.clone()))
    finally:
        L.gnnpp_set_tuning(_native.TUNE_POLICY_CP_TEAM, 1)
    assert torch.isfinite(got[0][0]).all()
    for a, b in zip(got[0], got[1]):
        assert torch.equal(a, b)
