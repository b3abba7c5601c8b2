"""GPU (-m gpu): the first conv layer of the one-launch policy kernel with (window, agent) pairs on its MFMA columns (a
compile-time team of ten, one-plane tiles; key TUNE_POLICY_CP_TEAM_L0, 1 = this form) against the same kernel with agents
on L0's columns (key = 0), BIT FOR BIT.  The packed form addresses the pixels per (tile, lane), walks sixteen positions per
wave instead of 24 / 28, stores every tile before the layer's barrier and holds nothing in registers: a wrong address, a
column stored into another cell, a store that overtakes another wave's pixel read or a dropped position changes logits."""
import numpy as np
import pytest
import torch

from gnn_pathplanning_amd import _native
from oracle import policy_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-4
KEY = _native.TUNE_POLICY_CP_TEAM_L0


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


def _both(net, obs_d, L):
    """logits with key 22 = 1, 0, 1"""
    outs = []
    try:
        for l0 in (1, 0, 1):
            assert L.gnnpp_set_tuning(KEY, l0) == 0 and L.gnnpp_get_tuning(KEY) == l0
            outs.append(net.forward_logits(obs_d).clone())
    finally:
        L.gnnpp_set_tuning(KEY, 1)
    return outs


def _run(dev, B, N, K, obs, seed):
    L = _native.lib()
    sd = orc.init_state_dict(K, seed=40 + seed)
    net = _net(N, K, dev, sd)
    S = torch.from_numpy(orc.synth_gso_geometric(B, N, 20, seed=seed)).float()
    net.addGSO(S.to(dev))
    return sd, S, _both(net, obs.to(dev), L)


def _oracle_agrees(sd, S, obs, got):
    want = torch.stack(orc.policy_forward(sd, S, obs), 0)
    return (got.cpu() - want).abs().max().item() <= TOL * max(1.0, want.abs().max().item())


@pytest.mark.parametrize('B', [1, 2, 3])
@pytest.mark.parametrize('K', [2, 3, 4])
def test_team10_l0_is_bit_identical(dev, B, K):
    obs = orc.synth_obs(B, 10, seed=17 + K + B)                       # random {0, 1}: one-plane tiles
    sd, S, outs = _run(dev, B, 10, K, obs, seed=K + B)
    assert torch.isfinite(outs[0]).all() and outs[0].abs().max().item() > 0
    assert torch.equal(outs[0], outs[1]), (outs[0] - outs[1]).abs().max().item()
    assert torch.equal(outs[0], outs[2])
    if B == 3 and K == 3:
        assert _oracle_agrees(sd, S, obs, outs[0])


@pytest.mark.parametrize('kind', ['zeros', 'ones', 'bf16'])
def test_team10_l0_constant_and_dense_pixels(dev, kind):
    """all zero, all one, and any bf16 value in every pixel (still one plane; no window's maximum is a zero by luck)"""
    B, K = 3, 3
    shape = (B, 10, 3, 11, 11)
    obs = {'zeros': torch.zeros(shape), 'ones': torch.ones(shape),
           'bf16': torch.randn(shape, generator=torch.Generator().manual_seed(5)).bfloat16().float()}[kind]
    sd, S, outs = _run(dev, B, 10, K, obs, seed=9)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert _oracle_agrees(sd, S, obs, outs[0])


def test_one_pixel_that_is_not_bf16_takes_the_three_plane_path(dev):
    """a single pixel with low mantissa bits: the tile of its graph needs all three planes, b3_l0_generic under both values
    of the key; the other graphs stay one-plane"""
    B, K = 3, 3
    obs = orc.synth_obs(B, 10, seed=23)
    obs[1, 7, 2, 10, 10] = 1.0 + 2.0 ** -20
    sd, S, outs = _run(dev, B, 10, K, obs, seed=3)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert _oracle_agrees(sd, S, obs, outs[0])


@pytest.mark.parametrize('N', [9, 11])
def test_other_team_sizes_do_not_take_the_packed_l0(dev, N):
    B, K = 3, 3
    obs = orc.synth_obs(B, N, seed=N)
    sd, S, outs = _run(dev, B, N, K, obs, seed=N)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert _oracle_agrees(sd, S, obs, outs[0])


def test_key_21_still_forces_the_run_time_form(dev):
    L = _native.lib()
    B, K = 2, 3
    obs = orc.synth_obs(B, 10, seed=4)
    _, _, outs = _run(dev, B, 10, K, obs, seed=6)
    try:
        assert L.gnnpp_set_tuning(_native.TUNE_POLICY_CP_TEAM, 0) == 0
        _, _, runtime = _run(dev, B, 10, K, obs, seed=6)
    finally:
        L.gnnpp_set_tuning(_native.TUNE_POLICY_CP_TEAM, 1)
    assert torch.equal(outs[0], runtime[0]) and torch.equal(runtime[0], runtime[1])


def test_team10_l0_nan_and_inf_pixels(dev):
    """A NaN or an Inf whose low half is clear is one bf16: its graph stays one-plane and takes the packed L0.  (The pool's
    maximum and the clamp do not hand a NaN on -- as in the word path --, so the logits may well be finite.)  Both forms
    agree on which logits are NaN, which are Inf, and on every other value, element by element."""
    B, K = 3, 3
    obs = orc.synth_obs(B, 10, seed=12)
    obs[1, 4, 1, 5, 6] = float('nan')
    obs[2, 9, 0, 10, 0] = float('inf')
    assert not (obs.numpy().view(np.uint32) & 0xffff).any()
    clean = _run(dev, B, 10, K, orc.synth_obs(B, 10, seed=12), seed=2)[2][0]
    _, _, outs = _run(dev, B, 10, K, obs, seed=2)
    a, b = outs[0], outs[1]
    assert not torch.equal(a[:, 1], clean[:, 1]) and not torch.equal(a[:, 2], clean[:, 2])     # the pixels were read
    assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.isinf(), b.isinf())
    assert torch.equal(a[~a.isnan()], b[~b.isnan()])


def test_team10_l0_with_simulator_tail(dev):
    """The kernel with the simulator step behind it (BatchedRollout.step) at N = 10: one step, logits and next state under
    both values of the key."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    L = _native.lib()
    B, N, W = 3, 10, 20
    rng = np.random.default_rng(43)
    grids, starts, goals = [], [], []
    for _ in range(B):
        g = (rng.random((W, W)) < 0.08).astype(np.uint8)
        free = np.argwhere(g == 0)
        idx = rng.choice(len(free), size=2 * N, replace=False)
        grids.append(g); starts.append(free[idx[:N]]); goals.append(free[idx[N:]])
    grids, starts, goals = np.stack(grids), np.stack(starts), np.stack(goals)
    net = _net(N, 3, dev, orc.init_state_dict(3, seed=21))
    got = []
    try:
        for l0 in (1, 0):
            assert L.gnnpp_set_tuning(KEY, l0) == 0
            env = BatchedRollout(grids, starts, goals, 9, dev, tie_mode='hashed', seed=7)
            env.step(net)
            assert env._logits is not None and env._state_step == env.t            # the one-launch path was taken
            got.append((env._logits.clone(), env.pos.clone(), env.obs.clone(), env.S.clone()))
    finally:
        L.gnnpp_set_tuning(KEY, 1)
    assert torch.isfinite(got[0][0]).all()
    for a, b in zip(got[0], got[1]):
        assert torch.equal(a, b)
