"""GPU (-m gpu): the graph-filter kernels (the inference hot path bench.py measures) against a float64 statement of
the same call, with the fp32 CPU statement as the yardstick (tests/f64_yardstick.py; runner and statements in
tests/filter_f64_cases.py).  Every case runs under each precision (GNNPP_PREC_FP32 = bf16x3, _FP32_MFMA, _SPLIT_F16)
at input scales 1e-6, 1e-3, 1 and 1e3; a case's name says which kernel / template it reaches under the default
precision (the small-graph and pipeline kernels serve GNNPP_PREC_FP32 only: under the other two those cases run on
lsigf_kernel).  lsigf_kernel's <RTW, NW> is asserted against a restatement of its plan (filter_f64_cases.plan).

Covered: lsigf_kernel RTW 1..7 at NW 8 and RTW 1..4 at NW 16 (the most a 112-row workgroup has), NG == 8 and
run-time NG (G = 1, 17, 100), F = 1 .. 257 (F > 128 in 128-wide chunks, per-node bias, tap signals of chunk 0 only),
E = 1..3, K = 1..5, N = 1 .. 112, Nin < N, shared / batched / fp64 / unaligned (s_vec4 off) S, both layouts, ReLU,
the n-way split (heuristic and forced 2 .. rt_total); lsigf_small_b3_kernel (32- / 48-row workgroups, N = 1 .. 16,
ragged last workgroup); lsigf_pipe_b3_kernel (persistent grid 0 and 7, EVERY graph checked); policy_filter_kernel in
modes 0..3 through gnnpp_filter_head_fwd (logits); gnnpp_lsigf_fwd_save's tap signals; gnnpp_lsigf_input_grad with
and without the ReLU mask in both layouts; torch.ops.gnnpp.lsigf_backward (dh, dx, db) against float64 autograd,
cotangents down to 1e-6; the module API (graphML.LSIGF / BatchLSIGF)."""
import numpy as np
import pytest
import torch

import filter_f64_cases as fc
from f64_yardstick import gap
from gnn_pathplanning_amd._native import (TUNE_FILTER_GPW, TUNE_FILTER_PIPE_GRID,
                                          TUNE_FILTER_PLANE_ALIAS, TUNE_FILTER_SMALL,
                                          TUNE_FILTER_SMALL_ROWS, TUNE_FILTER_SPLIT,
                                          TUNE_FILTER_WAVES)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def bk(dev):
    from gnn_pathplanning_amd import _native
    return fc.TorchBackend(_native.lib(), dev)


def _cases():
    C = []
    # ---- lsigf_kernel <RTW, NW, NG 8>: N = 16 graphs, gpw forced: rt_total = gpw row tiles; B = 2 gpw + 1 (ragged)
    for r in range(1, 8):
        C.append(dict(name='lsigf<rtw%d,nw8,ng8>/gpw%d' % (r, r), seed=100 + r, B=2 * r + 1, N=16, G=128, F=128, K=3,
                      E=1, bias='feat', knobs={TUNE_FILTER_GPW: r, TUNE_FILTER_WAVES: 8}, expect=(8, r)))
    for g, r in ((2, 1), (4, 2), (6, 3), (7, 4)):
        C.append(dict(name='lsigf<rtw%d,nw16,ng8>/gpw%d' % (r, g), seed=110 + g, B=2 * g + 3, N=16, G=128, F=128,
                      K=2, E=1, bias='feat', x_nm=1, y_nm=1, relu=1, knobs={TUNE_FILTER_GPW: g, TUNE_FILTER_WAVES: 16},
                      expect=(16, r)))
    # F <= 64 (4 output tiles: two row-tile chunks per 8 waves)
    C.append(dict(name='lsigf<rtw3,nw8,ng8>/F33/gpw6', seed=120, B=13, N=16, G=128, F=33, K=3, E=1, bias='feat',
                  knobs={TUNE_FILTER_GPW: 6, TUNE_FILTER_WAVES: 8}, expect=(8, 3)))
    # ---- G, F, E, K sweep (run-time NG for G != 128; F > 128: chunks)
    for i, (G, F, E, K, bias) in enumerate(((1, 5, 1, 2, 'feat'), (17, 1, 2, 3, None), (100, 33, 3, 1, 'feat'),
                                            (128, 129, 1, 4, 'node'), (128, 257, 2, 2, 'node'),
                                            (17, 257, 1, 5, 'feat'), (128, 128, 3, 5, 'feat'),
                                            (100, 129, 1, 3, 'node'))):
        C.append(dict(name='lsigf<%s>/G%dF%dE%dK%d/%s' % ('ng8' if G == 128 else 'ng-runtime', G, F, E, K, bias),
                      seed=130 + i, B=17, N=12, G=G, F=F, K=K, E=E, bias=bias))
    # ---- N sweep (heuristic plan); N = 112 at narrow G and F
    for i, N in enumerate((1, 2, 3, 5, 16, 17, 64, 100)):
        C.append(dict(name='lsigf<auto>/N%d' % N, seed=150 + i, B=[1, 17, 100, 128][i % 4], N=N, G=128, F=128, K=3,
                      E=1, bias='feat', relu=i % 2))
    C.append(dict(name='lsigf<ng-runtime>/N112/G16F16', seed=160, B=3, N=112, G=16, F=16, K=3, E=1, bias='node'))
    # ---- layouts, GSO forms, padding
    C.append(dict(name='lsigf<auto>/Nin<N/sharedS/f64S/relu', seed=170, B=17, N=20, Nin=13, G=128, F=128, K=3, E=2,
                  bias='node', batched=False, f64=1, relu=1))
    C.append(dict(name='lsigf<auto>/nodemajor/s_offset', seed=171, B=17, N=16, G=128, F=128, K=4, E=1, bias='feat',
                  x_nm=1, y_nm=1, s_offset=1))
    C.append(dict(name='lsigf<auto>/featmajor-in/nodemajor-out/s_offset/f64S', seed=172, B=5, N=36, G=128, F=128,
                  K=2, E=1, y_nm=1, s_offset=1, f64=1))
    C.append(dict(name='lsigf<auto>/tap_spread', seed=173, B=17, N=10, G=128, F=128, K=5, E=1, bias='feat',
                  tap_spread=True))
    C.append(dict(name='lsigf<auto>/tap_scale1e-3', seed=174, B=17, N=10, G=128, F=128, K=3, E=1, tap_scale=1e-3))
    C.append(dict(name='lsigf<auto>/tap_scale1e2', seed=175, B=17, N=10, G=128, F=128, K=3, E=1, tap_scale=1e2))
    # ---- the n-way split: N = 100 (7 row tiles), B = 13 (not a multiple of 8)
    C.append(dict(name='lsigf<nsplit-heuristic>/N100', seed=180, B=13, N=100, G=128, F=128, K=3, E=1, bias='feat',
                  x_nm=1, y_nm=1, relu=1))
    for s in range(2, 8):
        C.append(dict(name='lsigf<nsplit%d>/N100' % s, seed=180 + s, B=13, N=100, G=128, F=128, K=3, E=1,
                      bias='feat', knobs={TUNE_FILTER_SPLIT: s}))
    # ---- the training form: tap signals (chunk 0 of F = 257 included)
    C.append(dict(name='lsigf_save<auto>/E2K3', seed=190, B=17, N=12, G=128, F=128, K=3, E=2, bias='feat',
                  save=True))
    C.append(dict(name='lsigf_save<auto>/F257/Nin<N', seed=191, B=5, N=20, Nin=15, G=128, F=257, K=2, E=1,
                  bias='node', save=True))
    # ---- lsigf_small_b3_kernel (FILTER_SMALL = 2)
    for i, N in enumerate((1, 4, 5, 8, 9, 12, 13, 16)):
        rows = (32, 48)[i % 2]
        C.append(dict(name='small_b3<rows%d>/N%d' % (rows, N), seed=200 + i, B=37, N=N, G=128, F=128, K=3, E=1,
                      bias='feat', x_nm=1, y_nm=1, relu=i % 2, f64=i % 3 == 0,
                      knobs={TUNE_FILTER_SMALL: 2, TUNE_FILTER_SMALL_ROWS: rows}))
    # ---- lsigf_pipe_b3_kernel (FILTER_SMALL = 3): every graph checked
    for i, (N, pg) in enumerate(((10, 0), (10, 7), (3, 7), (16, 0))):
        C.append(dict(name='pipe_b3<grid%d>/N%d' % (pg, N), seed=220 + i, B=1037, N=N, G=128, F=128, K=3 - i % 2,
                      E=1, bias='feat', x_nm=1, y_nm=1, knobs={TUNE_FILTER_SMALL: 3, TUNE_FILTER_PIPE_GRID: pg}))
    return C


LSIGF = _cases()


@pytest.mark.parametrize('case', [c for c in LSIGF if 'expect' in c], ids=lambda c: c['name'])
def test_plan_restatement_names_the_template(case):
    c = case
    k = c['knobs']
    _, _, nw, rtw = fc.plan(c['B'], c['N'], c['G'], c['F'], c['K'], k.get(TUNE_FILTER_GPW, 0), k.get(TUNE_FILTER_WAVES, 0),
                            k.get(TUNE_FILTER_SPLIT, 0))
    assert (nw, rtw) == c['expect']


def test_plan_reaches_every_split():
    got = {fc.plan(13, 100, 128, 128, 3, forced_split=s)[1] for s in range(2, 8)}
    assert got == set(range(2, 8)) and fc.plan(13, 100, 128, 128, 3)[1] == 7


@pytest.mark.parametrize('scale', fc.SCALES)
@pytest.mark.parametrize('prec', fc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('case', LSIGF, ids=lambda c: c['name'])
def test_lsigf_f64(bk, case, prec, scale):
    fc.run_lsigf(bk, case, prec, scale)


HEAD = []
for _i, _N in enumerate((17, 33, 64, 65, 100)):
    for _alias in (1, 0):
        HEAD.append(dict(name='policy_filter/N%d/alias%d' % (_N, _alias), seed=300 + 2 * _i + _alias, B=3 + _i % 2,
                         N=_N, K=(3, 2, 4, 3, 1)[_i], f64=_i % 2, s_offset=_alias and _i == 2,
                         knobs={TUNE_FILTER_PLANE_ALIAS: _alias}))
# two workgroups per graph of 100: the bf16x3 planes only fit aliased onto the dead z buffer (mode 3)
HEAD.append(dict(name='policy_filter/N100/alias1/nsplit2', seed=320, B=3, N=100, K=3,
                 knobs={TUNE_FILTER_PLANE_ALIAS: 1, TUNE_FILTER_SPLIT: 2}, modes={0: 3, 1: 1, 2: 0}))


@pytest.mark.parametrize('scale', fc.SCALES)
@pytest.mark.parametrize('prec', fc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('case', HEAD, ids=lambda c: c['name'])
def test_filter_head_f64(bk, case, prec, scale):
    mode, _ = fc.run_head(bk, case, prec, scale)
    # split-f16 -> mode 0, fp32 MFMA -> 1, bf16x3 -> 2 (own plane buffer) or 3 (planes on the dead z buffer: only with
    # PLANE_ALIAS), or 1 where neither fits
    allowed = {2: {0}, 1: {1}, 0: {1, 2, 3} if case['knobs'][TUNE_FILTER_PLANE_ALIAS] else {1, 2}}[prec]
    assert mode in allowed, (case['name'], prec, mode)


def test_filter_head_cases_reach_every_mode(bk):
    seen = set()
    for c in HEAD:
        with fc.Knobs(bk.lib, c['knobs']):
            for prec in fc.PRECS:
                seen.add(bk.lib.gnnpp_filter_head_mode(c['B'], c['N'], c['K'], prec))
    assert seen == {0, 1, 2, 3}, seen


GRAD = [dict(name='input_grad<auto>/N12K3', seed=400, B=17, N=12, G=128, F=128, K=3, E=1),
        dict(name='input_grad<auto>/N100K2/E2/f64S', seed=401, B=5, N=100, G=128, F=128, K=2, E=2, f64=1),
        dict(name='input_grad<ng-runtime>/G33F65/sharedS', seed=402, B=9, N=20, G=33, F=65, K=4, E=1, batched=False)]


@pytest.mark.parametrize('scale', (1e-6, 1e-3, 1.0, 1e3))
@pytest.mark.parametrize('nm,masked', [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize('case', GRAD, ids=lambda c: c['name'])
def test_input_grad_f64(bk, case, nm, masked, scale):
    fc.run_input_grad(bk, dict(case, x_nm=nm), scale, masked)


def _backward_statement(h, S, x, b, dy, relu, dt):
    h, x, b = (torch.from_numpy(a).to(dt).requires_grad_(True) for a in (h, x, b))
    S = torch.from_numpy(S).to(dt)
    F, E, K, G = h.shape
    z0, yy = x, 0
    for e in range(E):
        z = z0
        for k in range(K):
            if k:
                z = z @ S[:, e]
            yy = yy + torch.einsum('fg,bgn->bfn', h[:, e, k], z)
    yy = yy + b
    if relu:
        yy = torch.relu(yy)
    dh, dx, db = torch.autograd.grad(yy, (h, x, b), torch.from_numpy(dy).to(dt))
    return dh.numpy(), dx.numpy(), db.numpy()


@pytest.mark.parametrize('dscale', (1e-6, 1e-3, 1.0))
@pytest.mark.parametrize('prec', fc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('N,K,E,relu', [(12, 3, 1, 1), (50, 2, 2, 0), (100, 4, 1, 1)])
def test_lsigf_backward_f64(dev, N, K, E, relu, prec, dscale):
    """torch.ops.gnnpp.lsigf_backward: dh, dx, db against float64 autograd of the same statement (S rounded to fp32)."""
    import gnn_pathplanning_amd.ops  # noqa: F401
    B, G, F = 6, 128, 128
    h, S, x, b = fc.make_inputs(500 + N + K, B, N, G, F, K, E, bias='feat')
    b = b.reshape(F, 1)
    dy = (np.random.default_rng(N).standard_normal((B, F, N)) * dscale).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    dh, dx, db = torch.ops.gnnpp.lsigf_backward(t(h), t(S), t(x), t(b), t(dy), bool(relu), prec, 7)
    torch.cuda.synchronize()
    w64 = _backward_statement(h, S, x, b, dy, relu, torch.float64)
    w32 = _backward_statement(h, S, x, b, dy, relu, torch.float32)
    for name, got, a, r in zip(('dh', 'dx', 'db'), (dh, dx, db), w64, w32):
        fc.check('lsigf_backward/N%d/%s/%s/dscale=%g' % (N, name, fc.PREC_NAMES[prec], dscale), got.cpu().numpy(),
                 a, r)


@pytest.mark.parametrize('scale', fc.SCALES)
@pytest.mark.parametrize('prec', fc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('batched', (0, 1))
def test_module_api_f64(dev, batched, prec, scale):
    """graphML.LSIGF (shared S) / BatchLSIGF (per-sample fp64 S) without autograd: the module path to the kernels."""
    from gnn_pathplanning_amd import graphML as gml
    B, N, G, F, K, E = 9, 20, 128, 128, 3, 1
    h, S, x, b = fc.make_inputs(600 + batched, B, N, G, F, K, E, s_batched=bool(batched), bias='feat', scale=scale)
    b = b.reshape(F, 1)
    with torch.no_grad():
        if batched:
            y = gml.BatchLSIGF(torch.from_numpy(h).to(dev), torch.from_numpy(S.astype(np.float64)).to(dev),
                               torch.from_numpy(x).to(dev), torch.from_numpy(b).to(dev), precision=prec)
        else:
            y = gml.LSIGF(torch.from_numpy(h).to(dev), torch.from_numpy(S).to(dev), torch.from_numpy(x).to(dev),
                          torch.from_numpy(b).to(dev), precision=prec)
    ok, rep = gap(y.cpu().numpy(), fc.lsigf_statement(h, S, x, b, 0, np.float64),
                  fc.lsigf_statement(h, S, x, b, 0, np.float32))
    assert ok, rep
