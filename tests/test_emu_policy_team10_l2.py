"""CPU: the constant-team-size form of the SECOND packed layer of the one-launch policy kernel (csrc/encoder_kernel_b3.hip,
cp_layer2_fixed, ten agents).

(i) The census of its row-wise column order, recomputed here from the per-lane rule alone: which (tap, tile) units read
nothing but the zero row (the kernel's static_assert names six), that no live unit is dropped, that the order holds every
(agent, y, x) once, that every unit reads sixteen distinct LDS slots, and that the pooled values land once each in the
dwords the run-time form writes.
(ii) Lane emulator: the form against the run-time-N packed kernel of the same library, bit for bit, without and with the
simulator tail behind the policy (gnnpp_policy_fwd, gnnpp_rollout_policy_step)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

from gnn_pathplanning_amd._native import TUNE_POLICY_CP_TEAM  # noqa: E402

N = 10
TAPS = [(t // 3 - 1, t % 3 - 1) for t in range(9)]


def col(t, j):
    """(agent, y, x) of column j of tile t: eight row tiles 2 y + g of four agents each, two tail tiles for agents 8, 9"""
    if t < 8:
        return 4 * (t & 1) + (j >> 2), t >> 1, j & 3
    return 8 + ((j >> 2) & 1), 2 * (t - 8) + (j >> 3), j & 3


def wave_tiles(pair):
    return [2 * i + pair for i in range(4)] + [8 + pair]


def rot(n, fixed=True):
    return 10 if fixed and n == 9 else 4 * (n & 3) + (n >> 2)


def cell(y, x, n, fixed=True):
    """(row, slot) of input cell (y, x) of agent n in L1's output layout"""
    row = (19 if x == 4 else 12 + (n >> 2)) if y == 4 else (15 + (n & 3) if x == 4 else n)
    return row, (4 * (y & 3) + (x & 3) + rot(n, fixed)) & 15


def source(tap, t, j):
    """the 5x5 input cell lane j of unit (tap, t) multiplies, or None: the zero row"""
    n, y, x = col(t, j)
    yy, xx = y + TAPS[tap][0], x + TAPS[tap][1]
    assert yy <= 4 and xx <= 4                                      # a 4x4 output never leaves the input downwards
    return None if yy < 0 or xx < 0 else (n, yy, xx)


def test_order_holds_every_output_once():
    seen = [col(t, j) for t in range(10) for j in range(16)]
    assert sorted(seen) == [(n, y, x) for n in range(N) for y in range(4) for x in range(4)]


def test_census_of_the_row_wise_order():
    empty = {(tap, t) for tap in range(9) for t in range(10) if all(source(tap, t, j) is None for j in range(16))}
    assert empty == {(tap, t) for tap in (0, 1, 2) for t in (0, 1)}             # the kernel's static_assert: six
    # no live unit dropped: every product that touches a real cell belongs to a unit outside `empty`, and the products
    # of the kept units are exactly those of the convolution (each (agent, output, tap) with its source inside, once)
    kept = [(source(tap, t, j), col(t, j), tap) for tap in range(9) for t in range(10) if (tap, t) not in empty
            for j in range(16) if source(tap, t, j) is not None]
    want = [((n, y + dy, x + dx), (n, y, x), tap) for n in range(N) for y in range(4) for x in range(4)
            for tap, (dy, dx) in enumerate(TAPS) if y + dy >= 0 and x + dx >= 0]
    assert sorted(kept) == sorted(want)
    zero_products = 160 * 9 - len(want)
    assert zero_products == N * 23 and len(want) == N * 121                     # 23 of 144 per agent
    # per wave: 42 of 45 units, both pairs drop the same ones, every tap keeps >= 2 units and ends on the tail tile,
    # tile 0 starts at tap 3 and every other tile at tap 0
    for pair in range(2):
        live = [[(tap, t) not in empty for t in wave_tiles(pair)] for tap in range(9)]
        assert sum(map(sum, live)) == 42 and min(map(sum, live)) >= 2 and all(r[4] for r in live)
        assert [min(tap for tap in range(9) if live[tap][i]) for i in range(5)] == [3, 0, 0, 0, 0]
    # 6 units x 2 channel-tile pairs x 12 MFMAs
    assert len(empty) * 2 * 12 == 144 and 2160 - 144 == 2016 and 7308 - 144 == 7164


def test_one_agent_per_tile_has_no_empty_unit():
    """the run-time form's order (a tile = one agent's 16 positions): no unit is all zeros, whatever the tap"""
    for tap, (dy, dx) in enumerate(TAPS):
        assert any(y + dy >= 0 and x + dx >= 0 for y in range(4) for x in range(4))


def test_reads_are_conflict_free_and_cells_do_not_collide():
    for tap, (dy, dx) in enumerate(TAPS):
        for t in range(10):
            slots = set()
            for j in range(16):
                n, y, x = col(t, j)
                slots.add((4 * ((y + dy) & 3) + ((x + dx) & 3) + rot(n)) & 15)       # a redirected lane keeps its slot
            assert len(slots) == 16, (tap, t)
    cells = [cell(y, x, n) for n in range(N) for y in range(5) for x in range(5)]
    assert len(set(cells)) == 250 and max(r for r, _ in cells) <= 19
    # the run-time form's rotation would put two lanes of a tail tile on one slot: that is why agent 9 moves
    n0, y0, x0 = col(8, 4)
    n1, y1, x1 = col(8, 8)
    assert (n0, n1) == (9, 8) and cell(y0, x0, n0, fixed=False)[1] == cell(y1, x1, n1, fixed=False)[1]
    assert all(cell(y, x, n) == cell(y, x, n, fixed=False) for n in range(9) for y in range(5) for x in range(5))


def test_pooled_values_land_once_each():
    """(window, agent, dword) each lane writes, per wave pair: row tiles -- lane (agent, x) of tile pair Y holds window
    (Y, x >> 1), channel tile x & 1 = dwords 2 (x & 1), + 1; tail tile -- window (pair, x >> 1), dword 2 (x & 1) + (j >> 3).
    Every lane's value is the max over the four positions of ITS window, and nothing is written twice."""
    written = []
    for pair in range(2):
        for j in range(16):
            x = j & 3
            for Y in range(2):
                n, y, xx = col(2 * (2 * Y) + pair, j)
                n2, y2, _ = col(2 * (2 * Y + 1) + pair, j)
                assert (n2, y2) == (n, y + 1) and y == 2 * Y and xx == x       # the register-wise partner: same lane, next row
                pn, py, px = col(2 * (2 * Y) + pair, j ^ 1)
                assert (pn, py, px) == (n, y, x ^ 1)                           # the quad_perm partner
                for d in (0, 1):
                    written.append((2 * Y + (x >> 1), n, 2 * (x & 1) + d))
            n, y, xx = col(8 + pair, j)
            assert col(8 + pair, j ^ 8) == (n, y ^ 1, xx) and col(8 + pair, j ^ 1) == (n, y, xx ^ 1) and y >> 1 == pair
            written.append((2 * pair + (x >> 1), n, 2 * (x & 1) + (j >> 3)))
    assert sorted(written) == [(w, n, d) for w in range(4) for n in range(N) for d in range(4)]


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'):
        pytest.skip('host clang++ from ROCm not present')
    import emu_lib
    return emu_lib, emu_lib.load()


def _obs(kind, B, n, seed):
    import torch
    from oracle import policy_oracle as orc
    obs = orc.synth_obs(B, n, seed=seed)
    g = torch.Generator().manual_seed(seed)
    if kind == 'binary':
        return obs
    if kind == 'real':
        return obs * torch.randn(obs.shape, generator=g)
    assert kind == 'dense'
    return torch.randn(obs.shape, generator=g)


@pytest.mark.parametrize('B,n,K,kind,isolated',
                         [(B, 10, K, kind, ()) for B in (3, 5) for K in (2, 3, 4) for kind in ('binary', 'real')] +
                         [(3, 10, 4, 'dense', ()), (3, 10, 3, 'real', (3, 8, 9)), (3, 9, 3, 'real', ()), (3, 11, 3, 'real', ())])
def test_emu_team10_l2_is_bit_identical(emu, B, n, K, kind, isolated):
    import torch
    from oracle import policy_oracle as orc
    el, lib = emu
    sd_t = orc.init_state_dict(K, seed=90 + K)
    sd = {k: v.numpy() for k, v in sd_t.items()}
    enc = el.pack_encoder(lib, sd)
    filt = el.pack_filter(lib, sd['GFL.0.weight'])
    gb = el.f32(sd['GFL.0.bias'].reshape(-1))
    aw, ab = el.f32(sd['actionsMLP.0.weight']), el.f32(sd['actionsMLP.0.bias'])
    obs_t = _obs(kind, B, n, seed=K + B)
    S_t = torch.from_numpy(orc.synth_gso_geometric(B, n, 12, seed=K)).float()
    for a in isolated:
        S_t[:, a, :] = 0
        S_t[:, :, a] = 0
    obs, S = el.f32(obs_t.numpy()), el.f32(S_t.numpy())
    outs = []
    try:
        for team in (1, 0):
            assert lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM, team) == 0
            logits = np.full((n, B, 5), np.nan, dtype=np.float32)
            ws = np.zeros((B * n, 128), dtype=np.float32)
            assert lib.gnnpp_policy_fwd(el.ptr(obs), el.ptr(S), el.ptr(enc), el.ptr(filt), el.ptr(gb), el.ptr(aw),
                                        el.ptr(ab), el.ptr(ws), el.ptr(logits), B, n, K, 1, 0, 0, None, None) == 0
            assert not ws.any()                                    # the one-launch kernel ran
            outs.append(logits)
    finally:
        lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM, 1)
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    with torch.no_grad():
        want = torch.stack(orc.policy_forward(sd_t, S_t, obs_t), 0).numpy()
    assert np.abs(outs[0] - want).max() <= 1e-4 * max(1.0, np.abs(want).max())


def test_emu_team10_l2_with_simulator_tail(emu):
    """The kernel with the simulator step behind it (gnnpp_rollout_policy_step: policy + move + graph + observation in one
    launch) at N = 10: one step from the same state under both values of the key; logits, positions, observations, GSO
    and every other buffer of the episode byte for byte (tests/rollout_sim_cases.py holds the state between sentinels)."""
    import filter_f64_cases as fc
    import rollout_sim_cases as sc
    from oracle import policy_oracle as orc
    el, lib = emu
    bk = fc.EmuBackend(lib)
    B, K = 3, 3
    grids, starts, goals, actions = sc._random(31, B, N, 20, 20, 0.08, T=1)
    case = sc._case('team10 l2 tail', grids, starts, goals, actions, maxstep=[50, 50, 50], radius=6.0, grow=0)
    sd = {k: v.numpy() for k, v in orc.init_state_dict(K, seed=93).items()}
    enc = el.pack_encoder(lib, sd)
    filt = el.pack_filter(lib, sd['GFL.0.weight'])
    gb = el.f32(sd['GFL.0.bias'].reshape(-1))
    aw, ab = el.f32(sd['actionsMLP.0.weight']), el.f32(sd['actionsMLP.0.bias'])

    def policy_step(r, stream):
        return lib.gnnpp_rollout_policy_step(r, el.ptr(enc), el.ptr(filt), el.ptr(gb), el.ptr(aw), el.ptr(ab), K, 0, stream)

    got = []
    try:
        for team in (1, 0):
            assert lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM, team) == 0
            st = sc.SimState(bk, case, logits=True)
            st.r.grow, st.r.currentstep = 0, 0
            st.call('observe')
            start = st.call('gso')
            st.r.currentstep = 1
            got.append(st.call('step', fn=policy_step, poison=sc.OUTPUTS['move'] + ('connected', 'logits')))
    finally:
        lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM, 1)
    assert np.isfinite(got[0]['logits']).all() and np.abs(got[0]['logits']).max() > 0
    assert (got[0]['pos'] != start['pos']).any() and start['S'].any()           # agents moved, the graph has edges
    sc.same_bytes(('team10 l2 tail',), got[0], got[1])
