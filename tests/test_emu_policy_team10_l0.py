"""CPU: the first conv layer of the one-launch policy kernel with (window, agent) pairs on its MFMA columns
(csrc/encoder_kernel_b3.hip, b3_l0_stream_fixed: a compile-time team of ten, one-plane tiles; key TUNE_POLICY_CP_TEAM_L0).

(i) The form restated from its per-lane rule alone -- column order, the five read addresses of a (tile, lane), the v_perm
selectors, the store cells -- and held against the rule it replaces: every (agent, position) exactly once, every B fragment
dword the one b3_l0_stream builds (and the one the word path defines: k-slot by k-slot from the padded image), every
stored byte in the cell cp_layer1 reads, no store in front of the pixels' end, and the LDS bank census the kernel's
static_assert states.
(ii) Lane emulator: key = 1 against key = 0 of the same library, bit for bit, without and with the simulator tail."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

from gnn_pathplanning_amd._native import TUNE_POLICY_CP_TEAM, TUNE_POLICY_CP_TEAM_L0  # noqa: E402

N = 10
CHAN, AGENT, ROW = 73, 231, 6                  # kPkChan, kPkAgent (dwords), dwords per padded image row
PK_BYTES = 16 * AGENT * 4
REGION, CP_ROW, FRAG = 25 * 3 * 1024, 3072, 1024
L1IN = REGION - (16 + 1) * CP_ROW              # cp_geom(10): T1 = 16 rows and the row of zeros


def column(t, j):
    """(window, agent) of column j of tile t; the six columns behind 250 read window 0 of the absent agents 10 .. 15"""
    c = 16 * t + j
    return (c // N, c % N) if c < 25 * N else (0, c - 25 * N + N)


def wave_tiles(v):
    return [v + 4 * i for i in range(4)]


def role(q):
    """dword offsets of the five reads a (+ 7: e) | b | c | d | f (+ 1: g) of lane group q"""
    return [q * CHAN + o for o in (0, 1, 1, 6, 12)] if q < 3 else [13, CHAN + 13, 2 * CHAN + 13, 0, 0]


def reads_fixed(t, j, q, oy):
    """the seven dwords (roles a b c d e f g) lane (q, j) of tile t requests for half-window oy"""
    w, n = column(t, j)
    base = n * AGENT + 2 * (w // 5) * ROW + w % 5
    a = [base + r + oy * ROW for r in role(q)]
    return [a[0], a[1], a[2], a[3], a[0] + 7, a[4], a[4] + 1]


def reads_parent(win, agent, q, oy):
    """b3_l0_stream: lane (q, agent) on window win"""
    ab = agent * AGENT
    pb = ab + q * CHAN
    adr = [pb, pb + 1, pb + 1, pb + 6, pb + 12] if q < 3 else [ab + 13, ab + CHAN + 13, ab + 2 * CHAN + 13, ab, ab]
    off = (2 * (win // 5) + oy) * ROW + win % 5
    return [off + adr[0], off + adr[1], off + adr[2], off + adr[3], off + adr[0] + 7, off + adr[4], off + adr[4] + 1]


def perm(hi, lo, sel):
    b = int(lo).to_bytes(4, 'little') + int(hi).to_bytes(4, 'little')
    return int.from_bytes(bytes(b[(sel >> (8 * i)) & 0xff] for i in range(4)), 'little')


def fragment(img, dd, q, ox):
    """the four dwords of a position's B fragment from the seven requested dwords (both forms share this code)"""
    d = [int(img[x]) for x in dd]
    selA = ((0x03020100, 0x05040302) if q < 3 else (0x05040100, 0x07060302))[ox]
    selC = ((0x05040302, 0x07060504) if q < 3 else (0x01000100, 0x03020302))[ox]
    selD = ((0x03020100, 0x05040302) if q < 3 else (0x01000100, 0x03020302))[ox]
    return [perm(d[1], d[0], selA), perm(d[3], d[2], 0x07060302 if ox else 0x05040100), perm(d[4], d[3], selC),
            perm(d[6], d[5], selD)]


@pytest.fixture(scope='module')
def image():
    """a packed pixel image of 16 agents: every halfword of the ten agents' padded 12x12 images distinct and non-zero
    (pads included: an address off by one dword cannot hide behind equal values), the absent agents' images zero"""
    img = np.zeros(16 * AGENT, dtype=np.uint32)
    pad = np.zeros((N, 3, 12, 12), dtype=np.uint32)
    pad[:] = 1 + np.arange(N * 3 * 144, dtype=np.uint32).reshape(N, 3, 12, 12)
    assert pad.max() < 65536
    for n in range(N):
        for ch in range(3):
            for y in range(12):
                for c in range(ROW):
                    img[n * AGENT + ch * CHAN + y * ROW + c] = pad[n, ch, y, 2 * c] | (pad[n, ch, y, 2 * c + 1] << 16)
    return img, pad


def test_columns_hold_every_agent_and_window_once():
    cols = [column(t, j) for t in range(16) for j in range(16)]
    real = [c for c in cols if c[1] < N]
    assert sorted(real) == [(w, n) for w in range(25) for n in range(N)] and len(cols) - len(real) == 6
    assert [c for c in cols if c[1] >= N] == [(0, n) for n in range(10, 16)]          # tile 15, j >= 10: zero images
    assert sorted(t for v in range(4) for t in wave_tiles(v)) == list(range(16))     # four tiles per wave
    # every (agent, position): a lane walks the four positions (oy, ox) of its window
    pos = sorted((n, 2 * (w // 5) + oy, 2 * (w % 5) + ox) for w, n in real for oy in range(2) for ox in range(2))
    assert pos == [(n, y, x) for n in range(N) for y in range(10) for x in range(10)]
    # 64 (tile, position) fragments x 6 MFMAs instead of 100 x 6
    assert 16 * 4 * 6 == 384 and 7164 - (600 - 384) == 6948
    # the divisions of the kernel's address set-up as multiply-shift
    assert all((c * 205) >> 11 == c // 10 for c in range(256)) and all((w * 52) >> 8 == w // 5 for w in range(26))


def test_every_fragment_dword_is_the_parent_rules(image):
    img, pad = image
    for t in range(16):
        for j in range(16):
            w, n = column(t, j)
            for q in range(4):
                for oy in range(2):
                    dd = reads_fixed(t, j, q, oy)
                    assert max(dd) < 16 * AGENT
                    if n >= N:
                        assert not any(img[x] for x in dd)                             # columns 250 ..: zeros
                        continue
                    assert dd == reads_parent(w, n, q, oy)                             # the same seven dwords
                    for ox in range(2):
                        got = fragment(img, dd, q, ox)
                        # the word path's definition, k-slot e of lane group q at position (Y, X) of the padded image:
                        # q < 3: channel q, tap (e / 3, e % 3); q = 3: the (2, 2) taps of channels 0 .. 2, then five
                        # weightless slots that hold channel 0 at (Y, X)
                        Y, X = 2 * (w // 5) + oy, 2 * (w % 5) + ox
                        if q < 3:
                            half = [pad[n, q, Y + e // 3, X + e % 3] for e in range(8)]
                        else:
                            half = [pad[n, e, Y + 2, X + 2] for e in range(3)] + [pad[n, 0, Y, X]] * 5
                        want = [int(half[2 * i]) | (int(half[2 * i + 1]) << 16) for i in range(4)]
                        assert got == want, (t, j, q, oy, ox)


def test_store_cells_are_what_cp_layer1_reads():
    stored = {}
    for t in range(16):
        for lane in range(64):
            q, j = lane >> 4, lane & 15
            w, n = column(t, j)
            if 16 * t + j >= 25 * N:
                continue                                                               # not stored
            for p in range(3):
                at = L1IN + t * CP_ROW + p * FRAG + lane * 16
                u = w * N + n                                                          # cp_layer1: cell u = pos * N + n
                assert at == L1IN + (u >> 4) * CP_ROW + p * FRAG + q * 256 + (u & 15) * 16       # b3_store_window's cell
                assert at not in stored
                stored[at] = (w, n, q, p)
    assert len(stored) == 250 * 4 * 3
    # nothing is written where pixels are still read, and nothing into the row of zeros behind the sixteen rows
    assert min(stored) >= PK_BYTES and L1IN >= PK_BYTES and max(stored) + 16 <= L1IN + 16 * CP_ROW == REGION - CP_ROW


def test_lds_bank_census():
    """what the kernel's static_assert states: lanes per bank (64 banks of one dword) of each of a half-window's seven
    dword accesses; no two lanes of an access share a dword, so every lane beyond a bank's first is a conflict"""
    worst, per_half = 0, []
    for t in range(16):
        for oy in range(2):
            doubled = 0
            for r in range(7):
                dws = [reads_fixed(t, lane & 15, lane >> 4, oy)[r] for lane in range(64)]
                assert len(set(dws)) == 64
                cnt = np.bincount([x & 63 for x in dws], minlength=64)
                worst = max(worst, int(cnt.max()))
                doubled += int((cnt[cnt > 1] - 1).sum())
            per_half.append(doubled)
    assert (worst, max(per_half), sum(per_half)) == (3, 115, 3030)
    # b3_l0_stream (sixteen agents of one window on the columns): 2 lanes at most, 43 doubled lanes per half-window
    for win in (0, 7, 24):
        doubled = 0
        for r in range(7):
            cnt = np.bincount([reads_parent(win, lane & 15, lane >> 4, 1)[r] & 63 for lane in range(64)], minlength=64)
            assert cnt.max() <= 2
            doubled += int((cnt[cnt > 1] - 1).sum())
        assert doubled == 43


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'):
        pytest.skip('host clang++ from ROCm not present')
    import emu_lib
    return emu_lib, emu_lib.load()


def _obs(kind, B, n, seed):
    import torch
    from oracle import policy_oracle as orc
    obs = orc.synth_obs(B, n, seed=seed)                                # {0, 1}: one-plane tiles
    if kind == 'binary':
        return obs
    if kind == 'zeros':
        return torch.zeros_like(obs)
    if kind == 'ones':
        return torch.ones_like(obs)
    g = torch.Generator().manual_seed(seed)
    if kind == 'bf16':                                                  # any bf16 value in every pixel: still one plane
        return torch.randn(obs.shape, generator=g).bfloat16().float()
    assert kind == 'real'                                               # three planes: b3_l0_generic under both values
    return obs * torch.randn(obs.shape, generator=g)


def _policy(el, lib, sd, obs_t, S_t, B, n, K, keys):
    enc = el.pack_encoder(lib, sd)
    filt = el.pack_filter(lib, sd['GFL.0.weight'])
    gb = el.f32(sd['GFL.0.bias'].reshape(-1))
    aw, ab = el.f32(sd['actionsMLP.0.weight']), el.f32(sd['actionsMLP.0.bias'])
    obs, S = el.f32(obs_t.numpy()), el.f32(S_t.numpy())
    outs = []
    try:
        for team, l0 in keys:
            assert lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM, team) == 0 and lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM_L0, l0) == 0
            assert lib.gnnpp_get_tuning(TUNE_POLICY_CP_TEAM_L0) == l0
            logits = np.full((n, B, 5), np.nan, dtype=np.float32)
            ws = np.zeros((B * n, 128), dtype=np.float32)
            assert lib.gnnpp_policy_fwd(el.ptr(obs), el.ptr(S), el.ptr(enc), el.ptr(filt), el.ptr(gb), el.ptr(aw),
                                        el.ptr(ab), el.ptr(ws), el.ptr(logits), B, n, K, 1, 0, 0, None, None) == 0
            assert not ws.any()                                    # the one-launch kernel ran
            outs.append(logits)
    finally:
        lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM, 1)
        lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM_L0, 1)
    return outs


def test_key_is_a_switch(emu):
    _, lib = emu
    assert lib.gnnpp_get_tuning(TUNE_POLICY_CP_TEAM_L0) == 1
    assert lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM_L0, 2) == -1 and lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM_L0, -1) == -1
    assert lib.gnnpp_get_tuning(TUNE_POLICY_CP_TEAM_L0) == 1


@pytest.mark.parametrize('B,n,K,kind',
                         [(B, 10, K, 'binary') for B, K in ((1, 3), (2, 2), (3, 4))] +
                         [(2, 10, 3, 'zeros'), (2, 10, 3, 'ones'), (3, 10, 3, 'bf16'), (2, 10, 3, 'real'),
                          (2, 9, 3, 'binary'), (2, 11, 3, 'binary')])
def test_emu_team10_l0_is_bit_identical(emu, B, n, K, kind):
    import torch
    from oracle import policy_oracle as orc
    el, lib = emu
    sd_t = orc.init_state_dict(K, seed=50 + K)
    sd = {k: v.numpy() for k, v in sd_t.items()}
    obs_t = _obs(kind, B, n, seed=K + B)
    S_t = torch.from_numpy(orc.synth_gso_geometric(B, n, 12, seed=K)).float()
    # key 22 = 1 | key 22 = 0 | key 21 = 0 (the whole run-time form, whatever key 22 says)
    outs = _policy(el, lib, sd, obs_t, S_t, B, n, K, [(1, 1), (1, 0), (0, 1)])
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))
    with torch.no_grad():
        want = torch.stack(orc.policy_forward(sd_t, S_t, obs_t), 0).numpy()
    assert np.abs(outs[0] - want).max() <= 1e-4 * max(1.0, np.abs(want).max())


def test_emu_team10_l0_nan_and_inf_pixels(emu):
    """a NaN or an Inf whose low half is clear IS one bf16: the tile stays one-plane, and both forms treat it alike (the
    pool's maximum and the clamp do not hand a NaN on, as in the word path: the logits may well be finite)"""
    import torch
    from oracle import policy_oracle as orc
    el, lib = emu
    B, K = 3, 3
    sd = {k: v.numpy() for k, v in orc.init_state_dict(K, seed=58).items()}
    obs_t = _obs('binary', B, N, seed=8)
    obs_t[1, 4, 1, 5, 6] = float('nan')
    obs_t[2, 9, 0, 10, 0] = float('inf')
    assert not (obs_t.numpy().view(np.uint32) & 0xffff).any()
    S_t = torch.from_numpy(orc.synth_gso_geometric(B, N, 12, seed=2)).float()
    a, b = _policy(el, lib, sd, obs_t, S_t, B, N, K, [(1, 1), (1, 0)])
    clean = _policy(el, lib, sd, _obs('binary', B, N, seed=8), S_t, B, N, K, [(1, 1)])[0]
    assert not np.array_equal(a[:, 1], clean[:, 1]) and not np.array_equal(a[:, 2], clean[:, 2])   # the pixels were read
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))
    assert np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_emu_team10_l0_with_simulator_tail(emu):
    """The kernel with the simulator step behind it (gnnpp_rollout_policy_step) at N = 10: one step from the same state under
    both values of the key; logits, positions, observations, GSO and every other buffer of the episode byte for byte."""
    import filter_f64_cases as fc
    import rollout_sim_cases as sc
    from oracle import policy_oracle as orc
    el, lib = emu
    bk = fc.EmuBackend(lib)
    B, K = 3, 3
    grids, starts, goals, actions = sc._random(37, B, N, 20, 20, 0.08, T=1)
    case = sc._case('team10 l0 tail', grids, starts, goals, actions, maxstep=[50, 50, 50], radius=6.0, grow=0)
    sd = {k: v.numpy() for k, v in orc.init_state_dict(K, seed=95).items()}
    enc = el.pack_encoder(lib, sd)
    filt = el.pack_filter(lib, sd['GFL.0.weight'])
    gb = el.f32(sd['GFL.0.bias'].reshape(-1))
    aw, ab = el.f32(sd['actionsMLP.0.weight']), el.f32(sd['actionsMLP.0.bias'])

    def policy_step(r, stream):
        return lib.gnnpp_rollout_policy_step(r, el.ptr(enc), el.ptr(filt), el.ptr(gb), el.ptr(aw), el.ptr(ab), K, 0, stream)

    got = []
    try:
        for l0 in (1, 0):
            assert lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM_L0, l0) == 0
            st = sc.SimState(bk, case, logits=True)
            st.r.grow, st.r.currentstep = 0, 0
            st.call('observe')
            start = st.call('gso')
            st.r.currentstep = 1
            got.append(st.call('step', fn=policy_step, poison=sc.OUTPUTS['move'] + ('connected', 'logits')))
    finally:
        lib.gnnpp_set_tuning(TUNE_POLICY_CP_TEAM_L0, 1)
    assert np.isfinite(got[0]['logits']).all() and np.abs(got[0]['logits']).max() > 0
    assert (got[0]['pos'] != start['pos']).any() and start['S'].any()           # agents moved, the graph has edges
    sc.same_bytes(('team10 l0 tail',), got[0], got[1])
