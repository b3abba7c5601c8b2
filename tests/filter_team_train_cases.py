"""Training the team filter on neighbour lists (gnnpp_team_lists_transpose, gnnpp_lsigf_team_lists_fwd_save,
gnnpp_lsigf_team_lists_input_grad: csrc/lsigf_team_train_kernel.hip): the runner shared by
tests/test_emu_filter_team_train.py (host emulation) and tests/test_gpu_filter_team_train.py (MI355X).  A plain helper
module, not a conftest.

Inputs, pack, statements and yardstick are those of tests/filter_f64_cases.py, the S variants those of
tests/filter_team_cases.py: every result is held to the float64 statement of the same call with the fp32 numpy statement
as the measure (f64_yardstick.gap).  A result is compared to another output of the kernels only where include/gnnpp.h
states a byte equality: the transposed lists against gnnpp_team_lists_from_dense of the transposed S, y of the saving
forward against gnnpp_lsigf_team_lists_fwd, dx against that call on the transposed arguments.  Blocks are handed over
filled with 0xFF bytes, workspaces, zs and outputs with NaN."""
import ctypes

import numpy as np

import filter_f64_cases as fc
import filter_team_cases as tc
import rollout_lists_cases as lc
from f64_yardstick import MAX_K, RMS_K, gap
from gnn_pathplanning_amd._native import ERR_ARG, ERR_UNSUPPORTED

MIN_WEIGHT = 2.0 ** -10           # every non-zero weight is at least this: from_dense never drops an edge as a zero


# ---- graphs ----------------------------------------------------------------------------------------------------------
def graph(seed, graphs, N, kind):
    """S [graphs,N,N] float32: 20 % non-zeros with signed weights of 0.25 .. 1 over a ~sqrt(N) normalisation, no self
    loops, NOT symmetric.  kind: 'unsym', 'sym' (the upper triangle mirrored), 'full_empty'
    (filter_team_cases.shape_s: column 3 with N entries, column 5 empty), 'full_row' (row 3 % N with N entries)."""
    g = np.random.default_rng(seed)
    shape = (graphs, N, N)
    S = (g.random(shape) < 0.2) * (0.25 + 0.75 * g.random(shape)) * g.choice([-1.0, 1.0], shape)
    S = S / max(1.0, np.sqrt(0.2 * N))
    for i in range(graphs):
        np.fill_diagonal(S[i], 0)
    S = S.astype(np.float32)
    if kind == 'full_row':
        S[:, 3 % N, :] = ((0.25 + g.random((graphs, N))) / np.sqrt(N)).astype(np.float32)
    elif kind == 'sym':                                   # (the mirrored upper triangle: a sum S + S^T could nearly cancel)
        U = np.triu(S, 1)
        S = U + np.swapaxes(U, -1, -2)
    elif kind != 'unsym':
        S = tc.shape_s(S, kind, seed)
    nz = np.abs(S[S != 0])
    assert nz.size == 0 or nz.min() >= MIN_WEIGHT, (kind, N, float(nz.min()))
    return S


def transpose(bk, lists, graphs, N, fill=0xFF):
    nbytes = bk.lib.gnnpp_team_lists_bytes(graphs, N)
    out = bk.put(np.full(nbytes, fill, np.uint8))
    assert bk.lib.gnnpp_team_lists_transpose(lists.ptr, out.ptr, nbytes, graphs, N, bk.stream) == 0
    bk.sync()
    return out


def run_transpose(bk, c):
    """gnnpp_team_lists_transpose of the lists of S == gnnpp_team_lists_from_dense of S^T over cnt and the first
    roundup4(cnt) entries of every column; also against numpy's columns of S^T; twice: the input again; two calls: the
    same bytes."""
    graphs, N = c['graphs'], c['N']
    S = graph(c['seed'], graphs, N, c.get('s', 'unsym'))
    St = np.ascontiguousarray(np.swapaxes(S, -1, -2))
    if c.get('s') == 'full_empty':
        assert (np.count_nonzero(S[:, :, 3 % N], axis=1) == N).all()
    if c.get('s') == 'full_row':
        assert (np.count_nonzero(S[:, 3 % N, :], axis=1) == N).all()
    lists = lc.filter_lists(bk, S, N)
    want = lc.filter_lists(bk, St, N)
    got, again = transpose(bk, lists, graphs, N), transpose(bk, lists, graphs, N)
    name = c['name']
    assert got.get().tobytes() == again.get().tobytes(), name
    lc.same_lists(name, got.get(), want.get(), graphs, N)
    lc.check_block(name, got.get(), lc.lists_of_dense(St))
    back = transpose(bk, got, graphs, N)
    lc.same_lists(name + '/twice', back.get(), lists.get(), graphs, N)


def run_transpose_errors(bk):
    """The codes, and the output block (pre-filled with 0xFF) untouched."""
    graphs, N = 2, 17
    lists = lc.filter_lists(bk, graph(3, graphs, N, 'unsym'), N)
    need = bk.lib.gnnpp_team_lists_bytes(graphs, N)
    off = lambda buf, n: ctypes.c_void_p(buf.ptr.value + n)                    # noqa: E731

    def call(out, src=lists.ptr, dst=None, nbytes=need, graphs=graphs, N=N):
        return bk.lib.gnnpp_team_lists_transpose(src, out.ptr if dst is None else dst(out), nbytes, graphs, N, bk.stream)

    table = (('in place', dict(dst=lambda o: lists.ptr)), ('NULL lists', dict(src=None)),
             ('NULL lists_t', dict(dst=lambda o: None)), ('misaligned lists', dict(src=off(lists, 8))),
             ('misaligned lists_t', dict(dst=lambda o: off(o, 4))), ('short block', dict(nbytes=need - 1)),
             ('graphs = 0', dict(graphs=0)), ('N = 0', dict(N=0)), ('N = 1025', dict(N=1025, nbytes=1 << 30)))
    before = lists.get().tobytes()
    for name, kw in table:
        out = bk.put(np.full(need + 16, 0xFF, np.uint8))
        assert call(out, **kw) == ERR_ARG, name
        bk.sync()
        assert (out.get() == 0xFF).all() and lists.get().tobytes() == before, name
    out = bk.put(np.full(need, 0xFF, np.uint8))
    assert call(out) == 0                                                       # ... and exactly the bytes it asks for
    bk.sync()
    assert bk.lib.gnnpp_version() == 330


# ---- forward with taps, input gradient ------------------------------------------------------------------------------
def _filter_inputs(c):
    """h, S (fp32, [B,E,N,N] | [E,N,N]), x [B,G,N], b of case c: filter_team_cases.inputs with this module's graphs."""
    B, N, E = c['B'], c['N'], c['E']
    batched = c.get('batched', True)
    h, _, x, b = tc.inputs(dict(c, s=None), 1.0)
    graphs = (B if batched else 1) * E
    S = graph(c['seed'] + 11, graphs, N, c.get('s', 'unsym')).reshape((B, E, N, N) if batched else (E, N, N))
    return h, S, x, b


def run_save(bk, c, prec):
    """gnnpp_lsigf_team_lists_fwd_save: y's bytes are gnnpp_lsigf_team_lists_fwd's; y and every zs[e K + k] against
    float64; the floats behind zs stay NaN."""
    B, N, G, F, K, E = c['B'], c['N'], c['G'], c['F'], c['K'], c['E']
    batched, relu, per_node = c.get('batched', True), c.get('relu', 0), int(c.get('bias') == 'node')
    h, S, x, b = _filter_inputs(c)
    xb, packed = bk.put(np.ascontiguousarray(x.transpose(0, 2, 1))), fc.pack(bk, h)
    bb = bk.put(b) if b is not None else None
    lists = lc.filter_lists(bk, S, N) if K > 1 else None
    lp = lists.ptr if lists is not None else None
    y0, y1 = bk.empty((B, N, F)), bk.empty((B, N, F))
    rows = E * K * B * N
    zs = bk.empty((rows + 3, G))                                                # (three rows the call does not own)
    ws, nbytes = tc.workspace(bk, B, N, G, K, E, batched)
    assert bk.lib.gnnpp_lsigf_team_lists_fwd(xb.ptr, lp, packed.ptr, bb.ptr if bb else None, y0.ptr, ws.ptr, nbytes, B,
                                             N, G, F, K, E, int(batched), relu, per_node, prec, bk.stream) == 0
    ws, nbytes = tc.workspace(bk, B, N, G, K, E, batched)
    assert bk.lib.gnnpp_lsigf_team_lists_fwd_save(xb.ptr, lp, packed.ptr, bb.ptr if bb else None, y1.ptr, zs.ptr, ws.ptr,
                                                  nbytes, B, N, G, F, K, E, int(batched), relu, per_node, prec,
                                                  bk.stream) == 0
    bk.sync()
    name = '%s/%s' % (c['name'], fc.PREC_NAMES[prec])
    a0, a1, z = y0.get(), y1.get(), zs.get()
    assert np.isfinite(a0).all() and a0.tobytes() == a1.tobytes(), name
    assert np.isnan(ws.get()).all(), name                                       # the workspace is not written
    assert np.isnan(z[rows:]).all() and np.isfinite(z[:rows]).all(), name
    fc.check(name + '/y', a1.transpose(0, 2, 1), fc.lsigf_statement(h, S, x, b, relu, np.float64),
             fc.lsigf_statement(h, S, x, b, relu, np.float32))
    z = z[:rows].reshape(E * K, B * N, G)
    w64, w32 = fc.tap_signals(S, x, K, E, np.float64), fc.tap_signals(S, x, K, E, np.float32)
    for t in range(E * K):
        fc.check('%s/zs[%d]' % (name, t), z[t], w64[t], w32[t])


def run_input_grad(bk, c):
    """gnnpp_lsigf_team_lists_input_grad on the transposed lists: dx's bytes are gnnpp_lsigf_team_lists_fwd's on (dy,
    lists_t, packed_t, G := F, F := G) at GNNPP_PREC_FP32_MFMA; dx against the float64 statement sum_k (S^k dy) h_k.  On
    an unsymmetric S the same statement on S instead of S^T is far outside the allowance (checked here, on the CPU)."""
    B, N, G, F, K, E = c['B'], c['N'], c['G'], c['F'], c['K'], c['E']
    batched = c.get('batched', True)
    h, S, _, _ = _filter_inputs(c)
    dy = np.random.default_rng(c['seed'] + 1).standard_normal((B, F, N)).astype(np.float32)
    ht = np.ascontiguousarray(h.transpose(3, 1, 2, 0))                           # [G,E,K,F]
    want = fc.lsigf_statement(ht, S, dy, None, 0, np.float64, transposed=True)
    ref = fc.lsigf_statement(ht, S, dy, None, 0, np.float32, transposed=True)
    if K > 1 and c.get('s', 'unsym') != 'sym':
        _, rep = gap(fc.lsigf_statement(ht, S, dy, None, 0, np.float64), want, ref)
        floor = 8 * 2.0 ** -24 * rep['scale']
        assert rep['rms'] > 100 * (RMS_K * rep['rms32'] + floor) and rep['max'] > 100 * (MAX_K * rep['max32'] + floor), \
            (c['name'], rep)
    graphs = (B if batched else 1) * E
    lists_t = transpose(bk, lc.filter_lists(bk, S, N), graphs, N) if K > 1 else None
    lp = lists_t.ptr if lists_t is not None else None
    dyb, packed_t = bk.put(np.ascontiguousarray(dy.transpose(0, 2, 1))), fc.pack(bk, ht)
    dx0, dx1 = bk.empty((B, N, G)), bk.empty((B, N, G))
    ws, nbytes = tc.workspace(bk, B, N, F, K, E, batched)
    assert bk.lib.gnnpp_lsigf_team_lists_fwd(dyb.ptr, lp, packed_t.ptr, None, dx0.ptr, ws.ptr, nbytes, B, N, F, G, K, E,
                                             int(batched), 0, 0, 1, bk.stream) == 0
    ws, nbytes = tc.workspace(bk, B, N, F, K, E, batched)
    assert bk.lib.gnnpp_lsigf_team_lists_input_grad(dyb.ptr, lp, packed_t.ptr, dx1.ptr, ws.ptr, nbytes, B, N, G, F, K, E,
                                                    int(batched), bk.stream) == 0
    bk.sync()
    a0, a1 = dx0.get(), dx1.get()
    assert np.isfinite(a0).all() and a0.tobytes() == a1.tobytes(), c['name']
    return fc.check(c['name'] + '/input_grad', a1.transpose(0, 2, 1), want, ref)


def run_train_errors(bk):
    """The saving forward's and the input gradient's error table: the code; y, zs and the workspace untouched."""
    B, N, G, F, K, E = 1, 20, 24, 24, 3, 1
    c = dict(name='errors', seed=5, B=B, N=N, G=G, F=F, K=K, E=E)
    h, S, x, _ = _filter_inputs(c)
    xb, packed = bk.put(np.ascontiguousarray(x.transpose(0, 2, 1))), fc.pack(bk, h)
    lists = lc.filter_lists(bk, S, N)
    big = bk.lib.gnnpp_lsigf_team_workspace_bytes(B, 1024, 128, K, E, 1)
    need = bk.lib.gnnpp_lsigf_team_workspace_bytes(B, N, G, K, E, 1)
    off = lambda buf, n: ctypes.c_void_p(buf.ptr.value + n)                    # noqa: E731

    def save(y, zs, ws, nbytes, lp=lists.ptr, N=N, G=G, F=F, prec=0, x=xb.ptr, yp=True, zp=True):
        return bk.lib.gnnpp_lsigf_team_lists_fwd_save(x, lp, packed.ptr, None, y.ptr if yp else None,
                                                      zs.ptr if zp else None, ws.ptr, nbytes, B, N, G, F, K, E, 1, 0, 0,
                                                      prec, bk.stream)

    def grad(y, zs, ws, nbytes, lp=lists.ptr, N=N, G=G, F=F, x=xb.ptr, yp=True):
        return bk.lib.gnnpp_lsigf_team_lists_input_grad(x, lp, packed.ptr, y.ptr if yp else None, ws.ptr, nbytes, B, N, G,
                                                        F, K, E, 1, bk.stream)

    table = (('NULL lists at K = 3', save, dict(lp=None), big, ERR_ARG), ('NULL zs', save, dict(zp=False), big, ERR_ARG),
             ('NULL y', save, dict(yp=False), big, ERR_ARG), ('NULL x', save, dict(x=None), big, ERR_ARG),
             ('misaligned lists', save, dict(lp=off(lists, 8)), big, ERR_ARG), ('N = 1025', save, dict(N=1025), big, ERR_ARG),
             ('short workspace', save, {}, need - 1, ERR_ARG), ('precision 3', save, dict(prec=3), big, ERR_ARG),
             ('G = 129', save, dict(G=129), big, ERR_UNSUPPORTED), ('F = 129', save, dict(F=129), big, ERR_UNSUPPORTED),
             ('split-f16', save, dict(prec=2), big, ERR_UNSUPPORTED),
             ('grad: NULL lists', grad, dict(lp=None), big, ERR_ARG), ('grad: NULL dx', grad, dict(yp=False), big, ERR_ARG),
             ('grad: NULL dy', grad, dict(x=None), big, ERR_ARG), ('grad: misaligned lists', grad, dict(lp=off(lists, 4)), big, ERR_ARG),
             ('grad: N = 1025', grad, dict(N=1025), big, ERR_ARG), ('grad: short workspace', grad, {}, need - 1, ERR_ARG),
             ('grad: G = 129', grad, dict(G=129), big, ERR_UNSUPPORTED), ('grad: F = 129', grad, dict(F=129), big, ERR_UNSUPPORTED))
    for name, fn, kw, nbytes, code in table:
        y, zs = bk.empty((B, N, 129)), bk.empty((E * K, B * N, 129))
        ws = bk.put(np.full(big // 4, np.nan, np.float32))
        assert fn(y, zs, ws, nbytes, **kw) == code, name
        bk.sync()
        assert np.isnan(y.get()).all() and np.isnan(zs.get()).all() and np.isnan(ws.get()).all(), name
    y, zs = bk.empty((B, N, F)), bk.empty((E * K, B * N, G))
    ws = bk.put(np.full(need // 4, np.nan, np.float32))
    assert save(y, zs, ws, need) == 0 and grad(y, zs, ws, need) == 0            # exactly the bytes they ask for
    bk.sync()
    assert np.isfinite(y.get()).all() and bk.lib.gnnpp_version() == 330


# ---- cases -----------------------------------------------------------------------------------------------------------
TRANSPOSE_CASES = [dict(name='N%d/%s/g%d' % (N, s, g), seed=100 + i, graphs=g, N=N, s=s) for i, (N, g, s) in enumerate([
    (1, 2, 'unsym'), (2, 2, 'unsym'), (5, 2, 'unsym'), (5, 1, 'full_empty'), (17, 2, 'unsym'), (17, 1, 'full_empty'),
    (17, 2, 'full_row'), (65, 2, 'unsym'), (65, 1, 'full_row'), (130, 2, 'unsym'), (130, 2, 'full_empty'),
    (130, 1, 'full_row'), (130, 4, 'sym')])]
GPU_TRANSPOSE_CASES = [dict(name='N1024/%s/g2' % s, seed=120 + i, graphs=2, N=1024, s=s)
                       for i, s in enumerate(('unsym', 'full_empty', 'full_row'))]


def _fc(i, N, K, E, G, F, B=2, **kw):
    name = 'N%d/K%dE%d/G%dF%d/%s' % (N, K, E, G, F, '/'.join('%s=%s' % kv for kv in sorted(kw.items())) or 'plain')
    return dict(name=name, seed=200 + i, B=B, N=N, K=K, E=E, G=G, F=F, **kw)


# K = 1 .. 4, E = 1, 2, the three (G, F), N = 17, 113, 130, shared and batched S, the three bias forms, ReLU on and off
FILTER_CASES = [
    _fc(0, 17, 1, 1, 8, 12, bias='feat'), _fc(1, 17, 2, 2, 8, 12, bias='node', relu=1),
    _fc(2, 17, 3, 1, 20, 128, batched=False, s='full_empty'), _fc(3, 17, 4, 2, 128, 128, bias='feat', relu=1),
    _fc(4, 17, 3, 1, 5, 7, bias='feat'),                                          # (rows of zs that are not 16-byte aligned)
    _fc(5, 113, 2, 1, 128, 128, bias='feat', relu=1), _fc(6, 113, 4, 1, 8, 12, batched=False, bias='node'),
    _fc(7, 113, 3, 2, 20, 128, s='full_row'),
    _fc(8, 130, 1, 2, 20, 128, relu=1), _fc(9, 130, 2, 1, 8, 12, s='full_empty', bias='node'),
    _fc(10, 130, 3, 1, 128, 128, bias='feat', relu=1), _fc(11, 130, 4, 2, 128, 128, batched=False, bias='feat'),
    _fc(12, 130, 3, 1, 128, 128, s='sym'),
]
EMU_FILTER_CASES = [FILTER_CASES[i] for i in (0, 1, 2, 4, 6, 9)] + [_fc(13, 130, 3, 1, 128, 128, B=1, bias='feat', relu=1)]
GPU_FILTER_CASES = [_fc(20, 1024, 3, 1, 128, 128, bias='feat', relu=1), _fc(21, 1024, 3, 2, 20, 128, batched=False)]
