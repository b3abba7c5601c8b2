"""The team graph filter (gnnpp_lsigf_team_fwd, gnnpp_filter_head_team_fwd: graphs of up to 1024 nodes spread over
workgroups, csrc/lsigf_team_kernel.hip) against a float64 statement: the runner shared by tests/test_emu_filter_team.py
(host emulation) and tests/test_gpu_filter_team.py (MI355X).  A plain helper module, not a conftest.

Inputs, pack, statements, yardstick and backends are those of tests/filter_f64_cases.py, unchanged: a result is held to
the float64 statement of the same call with the fp32 numpy statement as the measure (f64_yardstick.gap), never to
anything the kernels produce.  The workspace is handed over filled with NaN bytes: a list entry or tap signal read
before it was written shows."""

import numpy as np

import filter_f64_cases as fc
from gnn_pathplanning_amd._native import ERR_ARG, ERR_UNSUPPORTED  # noqa: F401 (the tests' names)

PRECS = (0, 1)                    # GNNPP_PREC_FP32 (bf16x3) | GNNPP_PREC_FP32_MFMA   (split-f16: GNNPP_ERR_UNSUPPORTED)


def shape_s(S, kind, seed):
    """S variants: None / 'unsym' (make_inputs' S, which is not symmetric), 'sym' (S + S^T), 'full_empty' (column 3
    with N non-zeros, the diagonal included, and column 5 with none)."""
    if kind in (None, 'unsym'):
        return S
    S = S.copy()
    if kind == 'sym':
        return (S + np.swapaxes(S, -1, -2)).astype(np.float32)
    assert kind == 'full_empty', kind
    g = np.random.default_rng(seed + 7)
    N = S.shape[-1]
    S[..., :, 3 % N] = (0.25 + g.random(S.shape[:-1])) / np.sqrt(N)
    if N > 5:
        S[..., :, 5] = 0
    return S.astype(np.float32)


def workspace(bk, B, N, G, K, E, batched):
    nbytes = bk.lib.gnnpp_lsigf_team_workspace_bytes(B, N, G, K, E, int(batched))
    assert nbytes >= 16 and nbytes % 16 == 0, nbytes
    return bk.put(np.full(nbytes // 4, np.nan, np.float32)), nbytes


def inputs(c, scale):
    B, N, G, F, K, E = c['B'], c['N'], c['G'], c['F'], c['K'], c['E']
    h, S, x, b = fc.make_inputs(c['seed'], B, N, G, F, K, E, None, c.get('batched', True), c.get('bias'), scale,
                                c.get('tap_scale', 1.0))
    return h, shape_s(S, c.get('s'), c['seed']), x, b


def run_team(bk, c, prec, scale, twice=False):
    """One gnnpp_lsigf_team_fwd call of case `c`: y [B,N,F] against float64.  twice: a second call into a fresh output
    and workspace must give the same bytes."""
    B, N, G, F, K, E = c['B'], c['N'], c['G'], c['F'], c['K'], c['E']
    batched, relu = c.get('batched', True), c.get('relu', 0)
    h, S, x, b = inputs(c, scale)
    S_dev = bk.put(S.astype(np.float64) if c.get('f64') else S)
    xb = bk.put(np.ascontiguousarray(x.transpose(0, 2, 1)))
    packed = fc.pack(bk, h)
    bb = bk.put(b) if b is not None else None
    outs = []
    for _ in range(2 if twice else 1):
        y = bk.empty((B, N, F))
        ws, nbytes = workspace(bk, B, N, G, K, E, batched)
        rc = bk.lib.gnnpp_lsigf_team_fwd(xb.ptr, S_dev.ptr if K > 1 or not c.get('null_s') else None, packed.ptr,
                                         bb.ptr if bb else None, y.ptr, ws.ptr, nbytes, B, N, G, F, K, E,
                                         int(bool(c.get('f64'))), int(batched), relu, int(c.get('bias') == 'node'), prec,
                                         bk.stream)
        assert rc == 0, (c['name'], rc)
        bk.sync()
        outs.append(y.get())
    if twice:
        assert outs[0].tobytes() == outs[1].tobytes(), c['name']
    want = fc.lsigf_statement(h, S, x, b, relu, np.float64)
    ref = fc.lsigf_statement(h, S, x, b, relu, np.float32)
    name = '%s/%s/scale=%g' % (c['name'], fc.PREC_NAMES[prec], scale)
    return fc.check(name, outs[0].transpose(0, 2, 1), want, ref)


def run_team_head(bk, c, prec, scale):
    """gnnpp_filter_head_team_fwd: logits [N,B,5] against float64 (S batched, ReLU, bias per feature or none)."""
    B, N, G, F, K, E = c['B'], c['N'], c['G'], c['F'], c['K'], c['E']
    h, S, x, b = inputs(dict(c, batched=True), scale)
    g = np.random.default_rng(c['seed'] + 2)
    aw = (g.standard_normal((5, F)) / np.sqrt(F / 2.0)).astype(np.float32)
    ab = (g.standard_normal(5) * scale).astype(np.float32)
    x_nm = np.ascontiguousarray(x.transpose(0, 2, 1))
    S_dev = bk.put(S.astype(np.float64) if c.get('f64') else S)
    packed = fc.pack(bk, h)
    xb, awb, abb = bk.put(x_nm), bk.put(aw), bk.put(ab)
    bb = bk.put(b) if b is not None else None
    logits = bk.empty((N, B, 5))
    ws, nbytes = workspace(bk, B, N, G, K, E, True)
    rc = bk.lib.gnnpp_filter_head_team_fwd(xb.ptr, S_dev.ptr, packed.ptr, bb.ptr if bb else None, awb.ptr, abb.ptr,
                                           logits.ptr, ws.ptr, nbytes, B, N, G, F, K, E, int(bool(c.get('f64'))), prec,
                                           bk.stream)
    assert rc == 0, (c['name'], rc)
    bk.sync()
    want = fc.head_statement(h, S, x_nm, b, aw, ab, np.float64)
    ref = fc.head_statement(h, S, x_nm, b, aw, ab, np.float32)
    return fc.check('%s/head/%s/scale=%g' % (c['name'], fc.PREC_NAMES[prec], scale), logits.get(), want, ref)


def run_errors(bk):
    """The error table: the code, and output + workspace (pre-filled with NaN) untouched."""
    B, N, G, F, K, E = 1, 120, 128, 128, 3, 1
    c = dict(seed=5, B=B, N=N, G=G, F=F, K=K, E=E)
    h, S, x, _ = inputs(c, 1.0)
    S_dev, xb, packed = bk.put(S), bk.put(np.ascontiguousarray(x.transpose(0, 2, 1))), fc.pack(bk, h)
    big = bk.lib.gnnpp_lsigf_team_workspace_bytes(B, 1024, 128, K, E, 1)

    def call(y, ws, nbytes, N=N, G=G, prec=0):
        return bk.lib.gnnpp_lsigf_team_fwd(xb.ptr, S_dev.ptr, packed.ptr, None, y.ptr if y else None, ws.ptr, nbytes,
                                           B, N, G, F, K, E, 0, 1, 0, 0, prec, bk.stream)

    need = bk.lib.gnnpp_lsigf_team_workspace_bytes(B, N, G, K, E, 1)
    table = (('N=1025', dict(N=1025), big, ERR_ARG), ('G=129', dict(G=129), big, ERR_UNSUPPORTED),
             ('split-f16', dict(prec=2), big, ERR_UNSUPPORTED), ('short workspace', {}, need - 1, ERR_ARG))
    for name, kw, nbytes, code in table:
        y = bk.empty((B, 1025, F))
        ws = bk.put(np.full(big // 4, np.nan, np.float32))
        assert call(y, ws, nbytes, **kw) == code, name
        bk.sync()
        assert np.isnan(y.get()).all() and np.isnan(ws.get()).all(), name
    ws = bk.put(np.full(big // 4, np.nan, np.float32))
    assert call(None, ws, big) == ERR_ARG
    bk.sync()
    assert np.isnan(ws.get()).all()
    assert bk.lib.gnnpp_lsigf_team_workspace_bytes(B, 1025, G, K, E, 1) == 0
    # ... and the call itself works with exactly the bytes it asks for
    y = bk.empty((B, N, F))
    ws = bk.put(np.full(need // 4, np.nan, np.float32))
    assert call(y, ws, need) == 0
    bk.sync()
    assert np.isfinite(y.get()).all()
