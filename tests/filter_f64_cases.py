"""The graph-filter kernels against a float64 statement: the case matrix and its runner, shared by
tests/test_gpu_filter_f64.py (libgnnpp.so on the MI355X) and tests/test_emu_filter_f64.py (the same HIP sources on
the host emulation of tests/emu/, a reduced matrix).  A plain helper module, not a conftest.

Every case is a call of the C ABI with a name that says which kernel (and template) it reaches under the default
precision.  It runs under each precision (GNNPP_PREC_FP32 = bf16x3, _FP32_MFMA, _SPLIT_F16) and at each input scale,
and its result is held to the float64 statement of the same call with the fp32 statement (numpy, CPU) as the
yardstick (f64_yardstick.gap).  The split-f16 contraction keeps 22 significand bits of every operand and rounds its
products like fp32: it is held to the same yardstick, with no extra allowance.

lsigf_kernel's plan (gnnpp_api.hip lsigf_plan) is restated here (`plan`) so that a case can name the template
<RTW, NW, NG == 8, H2> it reaches: rt_total = ceil(gpw N / 16) row tiles, split over nsplit workgroups, over
NW / MTP row-tile chunks of a workgroup (MTP = 8 output tiles, 4 when F <= 64): RTW = ceil(tiles / chunks).  Rows per
workgroup are at most 112 = 7 tiles, so NW = 16 with MTP = 8 reaches RTW 1..4 and NW = 8 reaches 1..7.
"""
import ctypes

import numpy as np

from f64_yardstick import gap

PRECS = (0, 1, 2)                 # GNNPP_PREC_FP32 (bf16x3) | GNNPP_PREC_FP32_MFMA | GNNPP_PREC_SPLIT_F16
PREC_NAMES = {0: 'fp32', 1: 'fp32mfma', 2: 'splitf16'}
SCALES = (1e-6, 1e-3, 1.0, 1e3)


# ---- backends --------------------------------------------------------------------------------------------------------
class Buf:
    def __init__(self, get, ptr, keep):
        self.get, self.ptr, self._keep = get, ptr, keep


class EmuBackend:
    """Host arrays; the emulated library runs synchronously."""

    def __init__(self, lib):
        self.lib, self.stream = lib, None

    def put(self, a, offset=0):
        flat = np.zeros(a.size + offset, a.dtype)
        flat[offset:] = np.ravel(a)
        view = flat[offset:].reshape(a.shape)
        return Buf(lambda: view.copy(), ctypes.c_void_p(view.ctypes.data), flat)

    def empty(self, shape, dtype=np.float32):
        return self.put(np.full(shape, np.nan, dtype))

    def sync(self):
        pass


class TorchBackend:
    """Device tensors on `dev`, the library's calls on the current stream."""

    def __init__(self, lib, dev):
        import torch
        from gnn_pathplanning_amd import _native
        self.lib, self.dev, self.torch = lib, dev, torch
        self.stream = _native.stream_ptr(dev)

    def put(self, a, offset=0):
        t = self.torch
        flat = t.zeros(a.size + offset, dtype=t.from_numpy(np.zeros(1, a.dtype)).dtype, device=self.dev)
        flat[offset:] = t.from_numpy(np.ascontiguousarray(a).ravel()).to(self.dev)
        view = flat[offset:].view(a.shape)
        return Buf(lambda: (t.cuda.synchronize(self.dev), view.cpu().numpy())[1], ctypes.c_void_p(view.data_ptr()),
                   flat)

    def empty(self, shape, dtype=np.float32):
        return self.put(np.full(shape, np.nan, dtype))

    def sync(self):
        self.torch.cuda.synchronize(self.dev)


class Knobs:
    """with Knobs(lib, {key: value}): set, and restore the previous values on the way out."""

    def __init__(self, lib, knobs):
        self.lib, self.knobs, self.saved = lib, dict(knobs), {}

    def __enter__(self):
        try:
            for k, v in self.knobs.items():
                self.saved[k] = self.lib.gnnpp_get_tuning(k)
                assert self.lib.gnnpp_set_tuning(k, v) == 0, (k, v)
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.lib.gnnpp_set_tuning(k, v)
        return False


# ---- lsigf_kernel's plan, restated -------------------------------------------------------------------------------
def plan(B, N, G, F, K, forced_gpw=0, forced_nw=0, forced_split=0):
    """(gpw, nsplit, nw, rtw) of lsigf_plan for one 128-feature chunk (LDS budget assumed to fit)."""
    F = min(F, 128)
    NG, MT = (G + 15) // 16, (F + 15) // 16
    zs = 16 * max(NG, MT) + 8
    Ns = (N + 3) & ~3

    def smem(g):
        rows = max(g * N, 8)
        lists = rows * Ns + ((rows + 15) & ~15) if K > 1 else 0
        return 2 * rows * zs * 4 + rows * Ns * 4 + lists

    best, best_cost = 1, 1e30
    for g in range(1, min(112 // N, B) + 1):
        if smem(g) > 160 * 1024:
            break
        rt, wgs = (g * N + 15) // 16, (B + g - 1) // g
        cost = ((wgs + 255) // 256) * (1.0 + rt)
        if cost < best_cost - 1e-9:
            best, best_cost = g, cost
    if 0 < forced_gpw <= 112 // N and forced_gpw <= B and smem(forced_gpw) <= 160 * 1024:
        best = forced_gpw
    rt_total = (best * N + 15) // 16
    grid = (B + best - 1) // best
    nsplit = 1
    if best == 1 and rt_total >= 2:
        groups = (grid + 7) // 8
        if forced_split >= 2:
            nsplit = min(forced_split, rt_total)
        elif forced_split == 0 and grid <= 128 and rt_total >= 4:
            room = 256 // (8 * groups)
            nsplit = 2 if room < 2 else min(room, rt_total)
    tiles = (rt_total + nsplit - 1) // nsplit
    mtp = 8 if MT > 4 else 4
    nw = 16 if best * N > 24 else 8
    if forced_nw in (8, 16):
        nw = forced_nw
    chunks = nw // mtp
    return best, nsplit, nw, (tiles + chunks - 1) // chunks


# ---- the statements ----------------------------------------------------------------------------------------------
def lsigf_statement(h, S, x, bias, relu, dt, transposed=False):
    """y [B,F,Nin] = bias + sum_e sum_k W_{e,k} . (x0 S_e^k) in dtype dt; x [B,G,Nin] is zero-padded to N nodes,
    S [B,E,N,N] or [E,N,N] (rounded to fp32 first, as the kernels load it); bias [F], [F,N] or None."""
    F, E, K, G = h.shape
    S = np.asarray(S, np.float32).astype(dt)
    if S.ndim == 3:
        S = S[None]
    if transposed:
        S = np.swapaxes(S, -1, -2)
    N = S.shape[-1]
    B, _, Nin = x.shape
    z0 = np.zeros((B, G, N), dt)
    z0[:, :, :Nin] = x
    h = h.astype(dt)
    y = np.zeros((B, F, N), dt)
    for e in range(E):
        z = z0
        for k in range(K):
            if k:
                z = z @ S[:, e]
            y += np.einsum('fg,bgn->bfn', h[:, e, k], z)
    if bias is not None:
        y += bias.astype(dt).reshape(F, -1)
    if relu:
        y = np.maximum(y, 0)
    return y[:, :, :Nin]


def tap_signals(S, x, K, E, dt):
    """z_{e,k} [E*K, B*N, G] node-major (the zs layout of gnnpp_lsigf_fwd_save)."""
    S = np.asarray(S, np.float32).astype(dt)
    if S.ndim == 3:
        S = S[None]
    B, G, N = x.shape
    out = []
    for e in range(E):
        z = x.astype(dt)
        for k in range(K):
            if k:
                z = z @ S[:, e]
            out.append(z.transpose(0, 2, 1).reshape(B * N, G))
    return np.stack(out)


def head_statement(h, S, x_nm, bias, aw, ab, dt):
    """logits [N,B,5] of gnnpp_filter_head_fwd: act_b + act_w . relu(lsigf(x) + bias)."""
    y = lsigf_statement(h, S, x_nm.transpose(0, 2, 1), bias, True, dt)          # [B,F,N]
    return (np.einsum('af,bfn->nba', aw.astype(dt), y) + ab.astype(dt)).astype(dt)


# ---- inputs ------------------------------------------------------------------------------------------------------
def make_inputs(seed, B, N, G, F, K, E, Nin=None, s_batched=True, bias=None, scale=1.0, tap_scale=1.0,
                tap_spread=False):
    """Taps h ~ N(0, 1 / (G K E)) x tap_scale (tap_spread: each tap times 10^u, u uniform over [-3, 2]); x ~ N(0, 1) x
    scale, signed; S: sparse (20 %) uniform weights over a ~sqrt(N) degree normalisation, no self loops."""
    g = np.random.default_rng(seed)
    Nin = N if Nin is None else Nin
    h = g.standard_normal((F, E, K, G)) / np.sqrt(G * K * E) * tap_scale
    if tap_spread:
        h *= 10.0 ** g.uniform(-3, 2, (F, E, K, 1))
    h = h.astype(np.float32)
    x = (g.standard_normal((B, G, Nin)) * scale).astype(np.float32)
    shape = (B, E, N, N) if s_batched else (E, N, N)
    S = (g.random(shape) < 0.2) * g.random(shape) / max(1.0, np.sqrt(0.2 * N))
    for idx in np.ndindex(*shape[:-2]):
        np.fill_diagonal(S[idx], 0)
    b = None
    if bias == 'feat':
        b = (g.standard_normal(F) * scale).astype(np.float32)
    elif bias == 'node':
        b = (g.standard_normal((F, N)) * scale).astype(np.float32)
    return h, S.astype(np.float32), x, b


def pack(bk, h):
    F, E, K, G = h.shape
    hb = bk.put(np.ascontiguousarray(h, np.float32))
    packed = bk.put(np.zeros(bk.lib.gnnpp_filter_packed_floats(G, F, K, E), np.float32))
    assert bk.lib.gnnpp_filter_pack(hb.ptr, packed.ptr, G, F, K, E, bk.stream) == 0
    packed._keep = (packed._keep, hb)
    return packed


def check(name, got, want64, ref32, scale=None):
    ok, rep = gap(got, want64, ref32, scale)
    assert ok, '%s: %s' % (name, {k: '%.3g' % v for k, v in rep.items()})
    return rep


# ---- one lsigf call ----------------------------------------------------------------------------------------------
def run_lsigf(bk, c, prec, scale):
    """One gnnpp_lsigf_fwd (or _fwd_save with c['save']) call of case `c` at input scale `scale`: the output (and the
    tap signals) against float64.  Returns the report of y."""
    B, N, G, F, K, E = c['B'], c['N'], c['G'], c['F'], c['K'], c['E']
    Nin = c.get('Nin', N)
    h, S, x, b = make_inputs(c['seed'], B, N, G, F, K, E, Nin, c.get('batched', True), c.get('bias'), scale,
                             c.get('tap_scale', 1.0), c.get('tap_spread', False))
    xnm, ynm, relu = c.get('x_nm', 0), c.get('y_nm', 0), c.get('relu', 0)
    S_dev = bk.put(S.astype(np.float64) if c.get('f64') else S, offset=c.get('s_offset', 0))
    x_in = np.ascontiguousarray(x.transpose(0, 2, 1)) if xnm else x
    xb = bk.put(x_in)
    packed = pack(bk, h)
    bb = bk.put(b) if b is not None else None
    y = bk.empty((B, N, F) if ynm else (B, F, Nin))
    flag = bk.put(np.zeros(1, np.int32))
    save = c.get('save', False)
    with Knobs(bk.lib, c.get('knobs', {})):
        if save:
            zs = bk.empty((E * K, B * N, G))
            rc = bk.lib.gnnpp_lsigf_fwd_save(xb.ptr, S_dev.ptr, packed.ptr, bb.ptr if bb else None, y.ptr, zs.ptr, B, N,
                                             Nin, G, F, K, E, int(bool(c.get('f64'))), int(c.get('batched', True)), 0,
                                             xnm, ynm, relu, int(c.get('bias') == 'node'), prec, flag.ptr, bk.stream)
        else:
            rc = bk.lib.gnnpp_lsigf_fwd(xb.ptr, S_dev.ptr, packed.ptr, bb.ptr if bb else None, y.ptr, B, N, Nin, G,
                                        F, K, E, int(bool(c.get('f64'))), int(c.get('batched', True)), xnm, ynm, relu,
                                        int(c.get('bias') == 'node'), prec, flag.ptr, bk.stream)
        assert rc == 0, (c['name'], rc)
        bk.sync()
    assert flag.get()[0] == 0, c['name']
    got = y.get()
    if ynm:
        got = got.transpose(0, 2, 1)[:, :, :Nin]
    want = lsigf_statement(h, S, x, b, relu, np.float64)
    ref = lsigf_statement(h, S, x, b, relu, np.float32)
    name = '%s/%s/scale=%g' % (c['name'], PREC_NAMES[prec], scale)
    rep = check(name, got, want, ref)
    if save:
        xp = np.zeros((B, G, N), np.float32)
        xp[:, :, :Nin] = x
        check(name + '/zs', zs.get(), tap_signals(S, xp, K, E, np.float64), tap_signals(S, xp, K, E, np.float32))
    return rep


def run_input_grad(bk, c, scale, masked):
    """gnnpp_lsigf_input_grad (exact fp32 whatever the precision): dx = sum_k W_k^T dy (S^T)^k, [B,G,N], optionally
    node-major with a ReLU mask."""
    B, N, G, F, K, E = c['B'], c['N'], c['G'], c['F'], c['K'], c['E']
    h, S, _, _ = make_inputs(c['seed'], B, N, G, F, K, E, s_batched=c.get('batched', True))
    g = np.random.default_rng(c['seed'] + 1)
    dy = (g.standard_normal((B, F, N)) * scale).astype(np.float32)
    ht = np.ascontiguousarray(h.transpose(3, 1, 2, 0))                           # [G,E,K,F]
    nm = c.get('x_nm', 0)
    mask = (g.random((B, N, G)) < 0.6).astype(np.float32) if masked else None
    packed_t = pack(bk, ht)
    S_dev = bk.put(S.astype(np.float64) if c.get('f64') else S)
    dyb = bk.put(np.ascontiguousarray(dy.transpose(0, 2, 1)) if nm else dy)
    mb = bk.put(mask) if masked else None
    dx = bk.empty((B, N, G) if nm else (B, G, N))
    rc = bk.lib.gnnpp_lsigf_input_grad(dyb.ptr, S_dev.ptr, packed_t.ptr, mb.ptr if mb else None, dx.ptr, B, N, G, F,
                                       K, E, int(bool(c.get('f64'))), int(c.get('batched', True)), nm, bk.stream)
    assert rc == 0, (c['name'], rc)
    got = dx.get()
    if nm:
        got = got.transpose(0, 2, 1)
    want = lsigf_statement(ht, S, dy, None, 0, np.float64, transposed=True)
    ref = lsigf_statement(ht, S, dy, None, 0, np.float32, transposed=True)
    if masked:
        m = mask.transpose(0, 2, 1) > 0
        want, ref = want * m, ref * m
    return check('%s/input_grad/mask=%d/scale=%g' % (c['name'], masked, scale), got, want, ref)


def run_head(bk, c, prec, scale):
    """gnnpp_filter_head_fwd: logits [N,B,5] against float64; asserts the schedule gnnpp_filter_head_mode names."""
    B, N, K, E = c['B'], c['N'], c['K'], 1
    h, S, x, b = make_inputs(c['seed'], B, N, 128, 128, K, E, bias='feat', scale=scale,
                             tap_scale=c.get('tap_scale', 1.0))
    g = np.random.default_rng(c['seed'] + 2)
    aw = (g.standard_normal((5, 128)) / 8).astype(np.float32)
    ab = (g.standard_normal(5) * scale).astype(np.float32)
    x_nm = np.ascontiguousarray(x.transpose(0, 2, 1))
    f64 = c.get('f64', 0)
    S_dev = bk.put(S[:, 0].astype(np.float64) if f64 else S[:, 0], offset=c.get('s_offset', 0))
    packed = pack(bk, h)
    xb, bb, awb, abb = bk.put(x_nm), bk.put(b), bk.put(aw), bk.put(ab)
    logits = bk.empty((N, B, 5))
    flag = bk.put(np.zeros(1, np.int32))
    with Knobs(bk.lib, c.get('knobs', {})):
        mode = bk.lib.gnnpp_filter_head_mode(B, N, K, prec)
        if 'modes' in c:
            assert mode == c['modes'][prec], (c['name'], prec, mode)
        rc = bk.lib.gnnpp_filter_head_fwd(xb.ptr, S_dev.ptr, packed.ptr, bb.ptr, awb.ptr, abb.ptr, logits.ptr, B, N,
                                          128, 128, K, E, f64, prec, flag.ptr, bk.stream)
        assert rc == 0, (c['name'], rc)
        bk.sync()
    assert flag.get()[0] == 0, c['name']
    want = head_statement(h, S, x_nm, b, aw, ab, np.float64)
    ref = head_statement(h, S, x_nm, b, aw, ab, np.float32)
    return mode, check('%s/mode=%d/%s/scale=%g' % (c['name'], mode, PREC_NAMES[prec], scale), logits.get(), want, ref)
