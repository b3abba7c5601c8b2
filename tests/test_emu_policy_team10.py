"""CPU: the constant-team-size form of the packed one-launch policy kernel (csrc/encoder_kernel_b3.hip, NFIX = 10).

(i) Which (tap, tile) units of its first packed layer hold nothing but zeros, recomputed here from the layout rule
alone -- column c = pos * N + n, tiles of 16 consecutive columns, a tap (dy, dx) leaves the 5x5 image at y + dy or
x + dx outside 0 .. 4 -- for teams of 1 .. 12 agents; the kernel's static_assert states the same counts for N = 10.
(ii) Lane emulator: the form against the run-time-N packed kernel and the agents-on-columns kernel of the same library,
bit for bit, on observations that live on the image border (where a unit dropped wrongly would show)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

from gnn_pathplanning_amd._native import TUNE_POLICY_CP, TUNE_POLICY_CP_TEAM  # noqa: E402

TAPS = [(t // 3 - 1, t % 3 - 1) for t in range(9)]


def _tiles(N):
    return (25 * N + 15) // 16


def _leaves(pos, dy, dx):
    y, x = divmod(pos, 5)
    return not (0 <= y + dy <= 4 and 0 <= x + dx <= 4)


def empty_units(N):
    """{(tap, tile)}: every existing column of the tile leaves the image under the tap"""
    out = set()
    for tap, (dy, dx) in enumerate(TAPS):
        for tile in range(_tiles(N)):
            cols = [c for c in range(16 * tile, 16 * tile + 16) if c < 25 * N]
            assert cols
            if all(_leaves(c // N, dy, dx) for c in cols):
                out.add((tap, tile))
    return out


def empty_units_by_flags(N):
    """The same set the way cp_layer1 states it per lane: four border bits per column (all four for a column that does
    not exist), a tap's mask of the borders it crosses; a unit is empty when every lane of the tile is redirected."""
    out = set()
    for tap, (dy, dx) in enumerate(TAPS):
        tmask = (1 if dy < 0 else 0) | (2 if dy > 0 else 0) | (4 if dx < 0 else 0) | (8 if dx > 0 else 0)
        for tile in range(_tiles(N)):
            fl = []
            for c in range(16 * tile, 16 * tile + 16):
                y, x = divmod(c // N, 5)
                fl.append(15 if c >= 25 * N else (y == 0) | (y == 4) << 1 | (x == 0) << 2 | (x == 4) << 3)
            if tmask and all(f & tmask for f in fl):
                out.add((tap, tile))
    return out


@pytest.mark.parametrize('N', range(1, 13))
def test_empty_units_of_every_team_size(N):
    e = empty_units(N)
    assert e == empty_units_by_flags(N)
    assert not any(tap == 4 for tap, _ in e)                       # the centre tap never leaves the image
    for tap, tile in e:                                            # an empty unit is empty under every tap that crosses
        dy, dx = TAPS[tap]                                         # the same borders and more
        for tap2, (dy2, dx2) in enumerate(TAPS):
            if (dy2 == dy or dy == 0) and (dx2 == dx or dx == 0):
                assert (tap2, tile) in e or (dy2, dx2) == (0, 0)


def test_team_of_ten():
    """18 units through the rows -- tiles 0, 1, 2 (columns 0 .. 47 of row 0's 0 .. 49) under the three dy = -1 taps, tiles
    13, 14, 15 (columns 208 .. 249 of row 4's 200 .. 249) under the three dy = +1 taps -- and three through the columns:
    tile 15's ten existing columns are position (4, 4) alone, tile 12 is positions (3, 4) and (4, 0)."""
    e = empty_units(10)
    rows = {(tap, tile) for tap in (0, 1, 2) for tile in (0, 1, 2)} | {(tap, tile) for tap in (6, 7, 8) for tile in (13, 14, 15)}
    assert len(rows) == 18 and rows <= e
    assert {u for u in e if u[0] % 3 == 1} == {u for u in rows if u[0] % 3 == 1}       # dx = 0: the rows alone
    assert e - rows == {(2, 15), (5, 15), (8, 12)}
    assert len(e) == 21
    # per wave (tiles w, w + 4, w + 8, w + 12): 32 / 30 / 30 / 31 of 36 units, every tap keeps at least two tiles,
    # every tile at least one tap
    live = [[(tap, w + 4 * i) not in e for i in range(4)] for w in range(4) for tap in range(9)]
    assert [sum(sum(r) for r in live[9 * w:9 * w + 9]) for w in range(4)] == [32, 30, 30, 31]
    assert min(sum(r) for r in live) >= 2
    assert all(any((tap, tile) not in e for tap in range(9)) for tile in range(16))


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'):
        pytest.skip('host clang++ from ROCm not present')
    import emu_lib
    return emu_lib, emu_lib.load()


@pytest.mark.parametrize('K,kind', [(3, 'border'), (2, 'border_binary'), (4, 'real')])
def test_emu_team10_form_is_bit_identical(emu, K, kind):
    import torch
    from oracle import policy_oracle as orc
    el, lib = emu
    B, N = 2, 10
    sd_t = orc.init_state_dict(K, seed=80 + K)
    sd = {k: v.numpy() for k, v in sd_t.items()}
    enc = el.pack_encoder(lib, sd)
    filt = el.pack_filter(lib, sd['GFL.0.weight'])
    gb = el.f32(sd['GFL.0.bias'].reshape(-1))
    aw, ab = el.f32(sd['actionsMLP.0.weight']), el.f32(sd['actionsMLP.0.bias'])
    g = torch.Generator().manual_seed(K)
    shape = orc.synth_obs(B, N, seed=K).shape
    border = torch.zeros(shape[-2:])
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = 1.0
    if kind == 'border':
        obs_t = torch.randn(shape, generator=g) * border
    elif kind == 'border_binary':
        obs_t = (torch.rand(shape, generator=g) < 0.6).float() * border
    else:
        obs_t = orc.synth_obs(B, N, seed=K) * torch.randn(shape, generator=g)
    S_t = torch.from_numpy(orc.synth_gso_geometric(B, N, 12, seed=K)).float()
    S_t[:, 3, :] = 0                                               # an isolated agent
    S_t[:, :, 3] = 0
    obs, S = el.f32(obs_t.numpy()), el.f32(S_t.numpy())
    outs = []
    try:
        for cp, team in ((1, 1), (1, 0), (0, 1)):
            assert lib.gnnpp_set_tuning(TUNE_POLICY_CP, cp) == 0 and lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM, team) == 0
            assert lib.gnnpp_get_tuning(TUNE_POLICY_CP_TEAM) == team
            logits = np.full((N, B, 5), np.nan, dtype=np.float32)
            ws = np.zeros((B * N, 128), dtype=np.float32)
            assert lib.gnnpp_policy_fwd(el.ptr(obs), el.ptr(S), el.ptr(enc), el.ptr(filt), el.ptr(gb), el.ptr(aw),
                                        el.ptr(ab), el.ptr(ws), el.ptr(logits), B, N, K, 1, 0, 0, None, None) == 0
            assert not ws.any()                                    # the one-launch kernel ran
            outs.append(logits)
    finally:
        lib.gnnpp_set_tuning(TUNE_POLICY_CP, 1)
        lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM, 1)
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))
    with torch.no_grad():
        want = torch.stack(orc.policy_forward(sd_t, S_t, obs_t), 0).numpy()
    assert np.abs(outs[0] - want).max() <= 1e-4 * max(1.0, np.abs(want).max())
    assert lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM, 2) == -1
