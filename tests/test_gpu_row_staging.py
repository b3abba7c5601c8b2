"""GPU: the row-wise staging of the packed one-plane pixel image (csrc/encoder_kernel_b3.hip: one work item = one image
row of one channel of one agent, stored as six dwords) against the three-plane word path of the same library
(GNNPP_TUNE_ENCODER_ONE_PLANE = 0: element-wise loads and word scatter, which row staging does not touch) -- bit for bit --
and against the CPU oracle within the parity tolerance of tests/test_gpu_parity.py (1e-4, relative to the largest
expected magnitude where that exceeds 1: the bf16-valued observations are not confined to {0, 1}).

Shapes: the smallest at which a row can go wrong -- a one-agent tile (most threads idle), odd N * 363 (graphs 1 and 2
start at sources that are not 16-byte aligned), both sides of the column-packing limit (12 | 13), a full 16-agent tile
(528 rows: the third trip), the stand-alone encoder's full + ragged tiles and its latency tiles."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gnn_pathplanning_amd._native import (TUNE_ENCODER_CP_TILE as ENC_CP_TILE,  # noqa: E402
                                          TUNE_ENCODER_ONE_PLANE as ONE_PLANE)

TOL = 1e-4
NOT_BF16 = 1.0 + 2.0 ** -20            # low 16 bits set: a tile that holds it needs all three planes


def _pixels(kind, B, N, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'binary':
        return (torch.rand(B, N, 3, 11, 11, generator=g) < 0.3).float()
    if kind == 'ones':
        return torch.ones(B, N, 3, 11, 11)
    x = torch.randn(B, N, 3, 11, 11, generator=g) * 3.0
    x = (x.view(torch.int32) & -65536).view(torch.float32)               # exactly one bf16 each, both signs
    x[torch.rand(x.shape, generator=g) < 0.2] = 0.0
    x[torch.rand(x.shape, generator=g) < 0.02] = -0.0
    return x


def _gso(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    S = torch.rand(B, N, N, generator=g) * (torch.rand(B, N, N, generator=g) < min(1.0, 6.0 / N))
    S = (S + S.transpose(1, 2)) * 0.2
    S.diagonal(dim1=1, dim2=2).zero_()
    return S.contiguous()


_nets = {}


def _net(N):
    """One planner per team size for the whole module (the weights never change)."""
    if N not in _nets:
        from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
        from oracle import policy_oracle as orc
        dev = torch.device('cuda:0')

        class Cfg:
            num_agents, nGraphFilterTaps, device = N, 3, dev
        sd = orc.init_state_dict(3)
        net = DecentralPlannerNet(Cfg()).to(dev).eval()
        net.load_state_dict(sd)
        _nets[N] = (net, sd)
    return _nets[N]


def _with_knobs(knobs, fn):
    from gnn_pathplanning_amd import _native
    L = _native.lib()
    old = {k: L.gnnpp_get_tuning(k) for k in knobs}
    try:
        for k, v in knobs.items():
            assert L.gnnpp_set_tuning(k, v) == 0
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        return out.cpu().clone()
    finally:
        for k, v in old.items():
            L.gnnpp_set_tuning(k, v)


def _logits(net, obs, one_plane=1):
    return _with_knobs({ONE_PLANE: one_plane}, lambda: torch.stack(list(net(obs))))     # [N, B, 5]


def _features(net, obs, tile, one_plane=1):
    return _with_knobs({ONE_PLANE: one_plane, ENC_CP_TILE: tile}, lambda: net.encode(obs))   # [1, M, 128]


def _close(got, want):
    err = (got.double() - want.double()).abs().max().item()
    bound = TOL * max(1.0, want.abs().max().item())
    print('max |error| = %.3g (bound %.3g)' % (err, bound))
    assert err <= bound, (err, bound)


@pytest.mark.parametrize('kind', ['binary', 'bf16'])
@pytest.mark.parametrize('N', [1, 7, 10, 12, 13, 16])
def test_fused_row_staging_equals_three_plane_path(kind, N):
    from oracle import policy_oracle as orc
    B = 3
    net, sd = _net(N)
    obs, S = _pixels(kind, B, N, seed=100 + N), _gso(B, N, seed=N)
    net.addGSO(S.cuda())
    rows = _logits(net, obs.cuda())
    words = _logits(net, obs.cuda(), one_plane=0)
    assert rows.shape == (N, B, 5) and torch.isfinite(rows).all() and rows.abs().max() > 0
    assert torch.equal(rows, words)
    _close(rows, torch.stack(orc.policy_forward(sd, S, obs)))


@pytest.mark.parametrize('kind', ['binary', 'bf16'])
@pytest.mark.parametrize('M,tile', [(16 + 5, 16), (3, 0)], ids=['full+ragged', 'latency'])
def test_encoder_row_staging_equals_three_plane_path(kind, M, tile):
    """tile: GNNPP_TUNE_ENCODER_CP_TILE (16 = 16-agent tiles: one full, one of five agents; 0 = the heuristic, which gives
    three agents one latency tile each)."""
    from oracle import policy_oracle as orc
    net, sd = _net(10)
    obs = _pixels(kind, 1, M, seed=200 + M)
    rows = _features(net, obs.cuda(), tile)
    words = _features(net, obs.cuda(), tile, one_plane=0)
    assert rows.shape == (1, M, 128) and torch.isfinite(rows).all() and rows.abs().max() > 0
    assert torch.equal(rows, words)
    _close(rows, orc.policy_features(sd, obs).transpose(1, 2))


# (agent, flat element of the agent's [3][11][11]) of graph 1 at N = 10: the tile's first pixel, its last pixel, and a
# pixel of row slot 300 = agent 9, channel 0, y = 3: rows 256 .. 329 are the second trip of threads 0 .. 73
@pytest.mark.parametrize('agent,elem', [(0, 0), (9, 362), (9, 3 * 11 + 5)], ids=['first', 'last', 'second-trip'])
def test_one_inexact_pixel_flips_its_tile_only(agent, elem):
    B, N = 3, 10
    assert 256 <= agent * 33 + elem // 11 < N * 33 or (agent, elem) == (0, 0)
    net, _ = _net(N)
    base = _pixels('bf16', B, N, seed=31)
    net.addGSO(_gso(B, N, seed=N).cuda())
    want_all_bf16 = _logits(net, base.cuda())
    obs = base.clone()
    obs[1, agent].view(-1)[elem] = NOT_BF16
    got = _logits(net, obs.cuda())
    words = _logits(net, obs.cuda(), one_plane=0)
    assert torch.equal(got[:, 1], words[:, 1])                     # the tile took (or equals) the three-plane path
    assert not torch.equal(got[:, 1], want_all_bf16[:, 1])         # (the pixel is seen at all)
    assert torch.equal(got[:, 0], want_all_bf16[:, 0]) and torch.equal(got[:, 2], want_all_bf16[:, 2])


@pytest.mark.parametrize('kind', ['binary', 'bf16'])
@pytest.mark.parametrize('neighbours', [float('nan'), NOT_BF16], ids=['nan', 'inexact'])
def test_nothing_outside_the_tensor_is_read(kind, neighbours):
    """The observations are a slice of a larger buffer (five floats in: not 16-byte aligned) whose other elements are
    NaN / not bf16: no tile may use a neighbour's pixel.  (Row staging reads the tile's rows and nothing else, so the
    neighbours cannot reach the one-plane decision either; both paths giving the same bits, the logits are what shows.)"""
    pad = 5
    for N, run in ((10, 'logits'), (16 + 5, 'features')):
        B = 3 if run == 'logits' else 1
        net, _ = _net(10)
        obs = _pixels(kind, B, N, seed=300 + N)
        buf = torch.full((pad + obs.numel() + pad,), neighbours).cuda()
        inside = buf[pad:pad + obs.numel()].view(obs.shape)
        inside.copy_(obs)
        assert inside.is_contiguous() and inside.data_ptr() % 16 != 0
        if run == 'logits':
            net.addGSO(_gso(B, N, seed=N).cuda())
            plain, sliced = _logits(net, obs.cuda()), _logits(net, inside)
        else:
            plain, sliced = _features(net, obs.cuda(), 16), _features(net, inside, 16)
        assert torch.isfinite(plain).all()
        assert torch.equal(plain, sliced)


@pytest.mark.parametrize('N', [10, 16])
def test_all_ones_image_exposes_no_pad(N):
    """Every border pixel set: a pad or slack dword of the packed image that is read but no longer zeroed would show.  A
    launch over the whole chip with huge pixels runs first, so that the LDS does not happen to hold zeros."""
    from oracle import policy_oracle as orc
    B = 3
    net, sd = _net(N)
    net.addGSO(_gso(512, N, seed=1).cuda())
    _logits(net, torch.full((512, N, 3, 11, 11), -3.0e38).cuda())
    obs, S = _pixels('ones', B, N, seed=0), _gso(B, N, seed=N)
    net.addGSO(S.cuda())
    rows = _logits(net, obs.cuda())
    words = _logits(net, obs.cuda(), one_plane=0)
    assert torch.isfinite(rows).all()
    assert torch.equal(rows, words)
    _close(rows, torch.stack(orc.policy_forward(sd, S, obs)))
