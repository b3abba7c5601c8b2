"""The differentiable graph-filter API of graphML.py against float64: the case list and the statements, shared by
tests/test_filter_autograd_cases.py (CPU: the statements agree with an independent formulation, and every wrong
variant of the operation is far outside the yardstick on every case it applies to) and
tests/test_gpu_filter_autograd_f64.py (the MI355X).  A plain helper module, not a conftest.

A case names an entry point (LSIGF, BatchLSIGF, GraphFilter, GraphFilterBatch, GraphFilterBatchGSO,
forward_node_major, `apply` = _LSIGFFunction.apply with fold bits, matrixPowersBatch) and the route the call must
take through _LSIGFFunction / matrixPowersBatch:

    lds              forward gnnpp_lsigf_fwd_save, dx the transposed filter, dh gnnpp_gemm_kmajor (feature-major) or
                     gnnpp_gemm_kmajor_multi (node-major)
    dense            _lsigf_large / _lsigf_large_backward: N > 112, or the forward launch answers GNNPP_ERR_UNSUPPORTED
    mixed-dx         forward LDS-resident, dx through _dense_dx (the transposed filter, input width F, does not fit)
    powers-own-gemm  matrixPowersBatch on fp32 GSOs: one gnnpp_gemm_kmajor per power >= 2
    powers-bmm       matrixPowersBatch on fp64 GSOs: torch.bmm

`expected_calls` turns the route into the number of calls of graphML._lsigf_large, ._lsigf_large_backward,
._LSIGFFunction._dense_dx and _native.gemm_kmajor that one forward + backward makes; the device test counts them.

The statement (`statement`) is written once and run in torch.float64 and torch.float32 on the CPU: zero-pad
x [B,G,Nin] to N nodes; z_{e,0} = x, z_{e,k} = z_{e,k-1} S_e; y = sum_{e,k} h[:,e,k,:] z_{e,k} + b (b [F,1], [F,N] or
None); optional ReLU; cut to Nin; S rounded to fp32 first (the reference's S.float()); dh, dx, db by
torch.autograd.grad for the case's cotangent.  The pre-powered family: P_{e,k} = S_e^k as a chain of products in the
statement's dtype, y = b + sum_{e,k} h[:,e,k,:] (x P_{e,k}).  The ReLU's mask is the float64 statement's, handed to
the fp32 statement, so that a pre-activation within roundoff of 0 cannot inflate the yardstick; the CPU test keeps every
pre-activation 8 allowances away from 0.

GSOs (`make_gso`): per row a forward and a backward ring edge and one random edge with independent weights (sparse,
S - S^T of the size of S, a return path to every node), rows scaled to sums in [0.7, 1]; generated in float64, so the
entries of an fp64 GSO are not fp32 numbers.  Taps ~ N(0, 1 / (G K E)), x and the cotangent ~ N(0, 1)
(filter_f64_cases.make_inputs).
"""
import functools

import numpy as np
import torch

import filter_f64_cases as fc
from f64_yardstick import MAX_K, ULP, ULPS

ROUTES = ('lds', 'dense', 'mixed-dx', 'powers-own-gemm', 'powers-bmm')
FILTER_ROUTES = ROUTES[:3]
NODE_MAJOR = ('forward_node_major', 'apply')
PRE_POWERED = ('GraphFilterBatchGSO',)
WRONG = ('adjoint_S', 'drop_last_tap', 'edge1_missing_dx', 'absent_nodes', 'short_chain', 'db_summed')
# the tensors a wrong variant must show in
WRONG_SHOWS = {'adjoint_S': ('dx',), 'drop_last_tap': ('y', 'dh'), 'edge1_missing_dx': ('dx',),
               'absent_nodes': ('y', 'dx'), 'short_chain': ('y',), 'db_summed': ('db',)}


# ---- the case list ---------------------------------------------------------------------------------------------------
def _case(entry, route, edge, **kw):
    c = dict(entry=entry, route=route, B=3, G=24, F=40, K=3, E=1, bias=None, batched=entry not in ('LSIGF', 'GraphFilter'),
             f64=False, relu=False, fold=0, prec=None, dscale=1.0, needs='hxb', dy_view=False, retain=False, then=None)
    c.update(kw)
    c.setdefault('Nin', c['N'])
    c['name'] = '%s-%s-%s' % (entry, route, edge)
    return c


def _cases():
    C = []
    add = lambda *a, **k: C.append(_case(*a, **k))                                               # noqa: E731
    # ---- dense by size: N = 113 and 130 at G = 24, F = 40
    add('BatchLSIGF', 'dense', 'N113-K3E1-featbias', N=113, bias='feat')
    add('BatchLSIGF', 'dense', 'N130-K4E2-nobias', N=130, K=4, E=2)
    add('BatchLSIGF', 'dense', 'N113-K1E2-featbias', N=113, K=1, E=2, bias='feat')
    add('BatchLSIGF', 'dense', 'N113-K3E2-f64S', N=113, E=2, f64=True)
    add('LSIGF', 'dense', 'N130-K3E1-sharedS-featbias', N=130, bias='feat')
    add('GraphFilter', 'dense', 'N113-K4E2-sharedS-Nin112-nodebias', N=113, Nin=112, K=4, E=2, bias='node')
    add('GraphFilterBatch', 'dense', 'N130-K3E1-Nin1-featbias', N=130, Nin=1, bias='feat')
    add('GraphFilterBatch', 'dense', 'N113-K3E2-Nin112-nodebias', N=113, Nin=112, E=2, bias='node')
    add('GraphFilterBatch', 'dense', 'N130-K4E1-f64S-featbias', N=130, K=4, f64=True, bias='feat')
    add('GraphFilterBatch', 'dense', 'N130-K1E1-Nin129-nodebias', N=130, Nin=129, K=1, bias='node')
    add('forward_node_major', 'dense', 'N113-K3E2-relu-featbias', N=113, E=2, relu=True, bias='feat')
    add('forward_node_major', 'dense', 'N130-K4E1-sharedS-norelu-featbias', N=130, K=4, batched=False, bias='feat')
    add('forward_node_major', 'dense', 'N113-K3E1-relu-nodebias', N=113, relu=True, bias='node', seed=11012)
    # ---- dense by refusal of the forward launch (and the 112-node graph that must stay LDS-resident)
    add('BatchLSIGF', 'dense', 'N50-G512F16-featbias', B=2, N=50, G=512, F=16, bias='feat')
    add('GraphFilterBatch', 'dense', 'N50-G512F16-Nin37-nodebias', B=2, N=50, Nin=37, G=512, F=16, bias='node')
    add('BatchLSIGF', 'dense', 'N112-G128F128-featbias', B=2, N=112, G=128, F=128, bias='feat')
    add('forward_node_major', 'dense', 'N112-G128F128-K2-relu', B=2, N=112, G=128, F=128, K=2, relu=True, bias='feat',
        seed=14016)
    add('BatchLSIGF', 'lds', 'N112-G16F16-featbias', B=2, N=112, G=16, F=16, bias='feat')
    # ---- mixed: N = 50, G = 16, F = 512
    mixed = dict(B=2, N=50, G=16, F=512)
    add('BatchLSIGF', 'mixed-dx', 'N50-G16F512-featbias', bias='feat', **mixed)
    add('GraphFilterBatch', 'mixed-dx', 'N50-G16F512-Nin37-E2-nodebias', Nin=37, E=2, bias='node', **mixed)
    add('LSIGF', 'mixed-dx', 'N50-G16F512-sharedS-K2', K=2, **mixed)
    add('apply', 'mixed-dx', 'N50-G16F512-fold0-relu', relu=True, bias='feat', seed=9021, **mixed)
    add('apply', 'mixed-dx', 'N50-G16F512-fold1-relu-maskeddy', relu=True, fold=1, bias='feat', seed=10022, **mixed)
    add('apply', 'mixed-dx', 'N50-G16F512-fold2-relu-input', fold=2, bias='feat', **mixed)
    add('apply', 'mixed-dx', 'N50-G16F512-fold3-E2', relu=True, fold=3, E=2, bias='feat', seed=15024, **mixed)
    # ---- LDS-resident, where no float64 case existed
    add('GraphFilterBatch', 'lds', 'N20-Nin13-E2-G128F128-featbias', N=20, Nin=13, E=2, G=128, F=128, bias='feat')
    add('GraphFilterBatch', 'lds', 'N20-Nin13-nodebias', N=20, Nin=13, bias='node')
    add('GraphFilter', 'lds', 'N20-Nin13-sharedS-K4-nodebias', N=20, Nin=13, K=4, bias='node')
    add('LSIGF', 'lds', 'N12-sharedS-G128F128-featbias', N=12, G=128, F=128, bias='feat')
    add('BatchLSIGF', 'lds', 'N1-K3-featbias', N=1, bias='feat')
    add('BatchLSIGF', 'lds', 'N16-featbias', N=16, bias='feat')
    add('BatchLSIGF', 'lds', 'N17-E2-nobias', N=17, E=2)
    add('BatchLSIGF', 'lds', 'N12-G128F160-two-chunks-nodebias', N=12, G=128, F=160, bias='node')
    add('BatchLSIGF', 'lds', 'N12-K1E2-featbias', N=12, K=1, E=2, bias='feat')
    add('BatchLSIGF', 'lds', 'N12-B1-K4-featbias', B=1, N=12, K=4, bias='feat')
    add('BatchLSIGF', 'lds', 'N12-f64S-K4-featbias', N=12, K=4, f64=True, bias='feat')
    add('forward_node_major', 'lds', 'N12-relu-G128F128-featbias', N=12, G=128, F=128, relu=True, bias='feat',
        seed=9036)
    # ---- forward precisions 0 / 1 / 2 (the gradient launches are exact fp32 whatever the precision)
    for p in (0, 1, 2):
        add('BatchLSIGF', 'lds', 'N20-G128F128-%s' % fc.PREC_NAMES[p], N=20, G=128, F=128, bias='feat', prec=p)
        add('BatchLSIGF', 'mixed-dx', 'N50-G16F512-K2-%s' % fc.PREC_NAMES[p], K=2, bias='feat', prec=p, **mixed)
    # ---- cotangent scales, the gradient bookkeeping: one case per route
    per_route = (('lds', dict(N=20, Nin=13, E=2, bias='node')), ('dense', dict(N=113, Nin=112, E=2, bias='node')),
                 ('mixed-dx', dict(Nin=37, E=2, bias='node', **mixed)))
    for route, kw in per_route:
        for ds in (1e-6, 1e3):
            add('GraphFilterBatch', route, 'dy-scale%g' % ds, dscale=ds, **kw)
        for needs in 'hxb':
            add('GraphFilterBatch', route, 'only-%s-requires-grad' % needs, needs=needs, **kw)
        add('GraphFilterBatch', route, 'noncontiguous-dy', dy_view=True, **kw)
        add('GraphFilterBatch', route, 'backward-twice', retain=True, **kw)
    for needs in 'hxb':
        add('forward_node_major', 'lds', 'N12-relu-only-%s-requires-grad' % needs, N=12, relu=True, bias='feat', needs=needs)
    # ---- the pre-powered family
    for N, K, E, dim in ((5, 1, 1, 3), (5, 2, 2, 4), (17, 3, 1, 3), (17, 4, 2, 4), (100, 4, 1, 3), (100, 3, 2, 4),
                         (113, 3, 1, 4), (113, 4, 2, 4)):
        add('matrixPowersBatch', 'powers-own-gemm', 'N%d-K%dE%d-%dD' % (N, K, E, dim), B=2, N=N, K=K, E=E, dim=dim)
    for N, K, E, dim in ((5, 1, 1, 3), (17, 2, 2, 4), (17, 4, 1, 3), (100, 4, 1, 4), (113, 3, 2, 4)):
        add('matrixPowersBatch', 'powers-bmm', 'N%d-K%dE%d-%dD-f64S' % (N, K, E, dim), B=2, N=N, K=K, E=E, dim=dim,
            f64=True)
    add('matrixPowersBatch', 'powers-own-gemm', 'N17-K2E1-3D-transposed-view', B=2, N=17, K=2, dim=3, s_view=True)
    add('matrixPowersBatch', 'powers-own-gemm', 'N17-K4E2-4D-transposed-view', B=2, N=17, K=4, E=2, dim=4, s_view=True)
    add('matrixPowersBatch', 'powers-bmm', 'N17-K4E1-3D-transposed-view-f64S', B=2, N=17, K=4, dim=3, s_view=True,
        f64=True)
    add('GraphFilterBatchGSO', 'powers-own-gemm', 'N10-K3E2-then-lds', N=10, E=2, bias='feat', then='lds')
    add('GraphFilterBatchGSO', 'powers-own-gemm', 'N120-K3E2-then-dense', N=120, E=2, bias='feat', then='dense')
    add('GraphFilterBatchGSO', 'powers-bmm', 'N10-K3E2-f64S-then-lds', N=10, E=2, bias='feat', f64=True, then='lds')
    for i, c in enumerate(C):        # (the seeds given above: ReLU cases whose pre-activations all keep 8 allowances from 0)
        c.setdefault('seed', 7000 + i)
    return C


CASES = _cases()


def case_id(c):
    return c['name']


def call_key(c):
    """Everything that makes the call, without the name and the seed."""
    return tuple(sorted((k, str(v)) for k, v in c.items() if k not in ('name', 'seed')))


def filter_route(c):
    """The route of the filter call itself (`then` for the pre-powered modules, whose `route` is the powers')."""
    return c['then'] if c['entry'] in PRE_POWERED else c['route']


def expected_calls(c, needs=None):
    """(_lsigf_large, _lsigf_large_backward, _dense_dx, gemm_kmajor) calls of one forward + backward of a filter case."""
    needs = c['needs'] if needs is None else needs
    E, K = (c['E'] * c['K'], 2) if c['entry'] in PRE_POWERED else (c['E'], c['K'])
    chain = E * (K - 1)
    fm_dh = int(c['entry'] not in NODE_MAJOR and 'h' in needs)
    dx = int('x' in needs)
    route = filter_route(c)
    if route == 'lds':
        return 0, 0, 0, fm_dh
    if route == 'dense':
        return 1, 1, 0, chain + 1 + int('h' in needs) + dx * (1 + chain)
    assert route == 'mixed-dx'
    return 0, dx, dx, fm_dh + dx * (1 + chain)


def powers_gemms(c):
    """gemm_kmajor calls of matrixPowersBatch on the case's GSO."""
    return max(c['K'] - 2, 0) if c['route'] == 'powers-own-gemm' else 0


# ---- inputs ----------------------------------------------------------------------------------------------------------
def make_gso(g, shape):
    """float64 GSOs [..., N, N]: see the module docstring."""
    N = shape[-1]
    S = np.zeros(shape, np.float64)
    r = np.arange(N)
    for idx in np.ndindex(*shape[:-2]):
        M = S[idx]
        for cols in ((r + 1) % N, (r - 1) % N, g.integers(0, N, N)):
            M[r, cols] += g.uniform(0.3, 1.0, N)
        M *= (g.uniform(0.7, 1.0, N) / M.sum(1))[:, None]
    return S


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = next(c for c in CASES if c['name'] == name)
    g = np.random.default_rng(c['seed'])
    B, N, E = c['B'], c['N'], c['E']
    if c['entry'] == 'matrixPowersBatch':
        return dict(S=make_gso(g, (B, N, N) if c['dim'] == 3 else (B, E, N, N)))
    G, F, K, Nin = c['G'], c['F'], c['K'], c['Nin']
    h, _, x, b = fc.make_inputs(c['seed'], B, N, G, F, K, E, Nin, bias=c['bias'])
    if c['fold'] & 2:
        x = np.maximum(x, 0)                                 # the output of a ReLU, exact zeros among its entries
    if c['bias'] == 'feat':
        b = b.reshape(F, 1)
    S = make_gso(g, (B, E, N, N) if c['batched'] else (E, N, N))
    dy = (g.standard_normal((B, F, Nin)) * c['dscale']).astype(np.float32)
    return dict(h=h, S=S, x=x, b=b, dy=dy)


def inputs(c):
    """h [F,E,K,G], x [B,G,Nin], b [F,1] | [F,N] | None, dy [B,F,Nin] (fp32), S [B,E,N,N] | [E,N,N] (float64: a case
    without `f64` hands S.astype(float32) to the device).  Cached: do not write into them."""
    return _inputs(c['name'])


# ---- the statement ---------------------------------------------------------------------------------------------------
def statement(c, dt, mask=None, dy=None):
    """dict(y, pre, dh, dx, db) of the case in torch dtype dt (numpy arrays; db None without a bias).  mask: the ReLU's
    0 / 1 mask [B,F,N] to use instead of the statement's own; dy: another cotangent than the case's."""
    inp = inputs(c)
    leaf = lambda a: None if a is None else torch.from_numpy(a).to(dt).requires_grad_(True)      # noqa: E731
    h, x, b = leaf(inp['h']), leaf(inp['x']), leaf(inp['b'])
    S = torch.from_numpy(inp['S'].astype(np.float32)).to(dt)
    if S.dim() == 3:
        S = S[None]
    F, E, K, G = h.shape
    N, Nin = S.shape[-1], x.shape[2]
    xp = torch.nn.functional.pad(x, (0, N - Nin))
    y = 0
    for e in range(E):
        z = xp
        P = torch.eye(N, dtype=dt).expand(S.shape[0], N, N)
        for k in range(K):
            if k and c['entry'] in PRE_POWERED:
                P = P @ S[:, e]
                z = xp @ P
            elif k:
                z = z @ S[:, e]
            y = y + torch.einsum('fg,bgn->bfn', h[:, e, k], z)
    if b is not None:
        y = y + b
    pre = y
    if c['relu']:
        y = torch.relu(y) if mask is None else y * torch.from_numpy(mask).to(dt)
    y = y[:, :, :Nin]
    leaves = [t for t in (h, x, b) if t is not None]
    cot = torch.from_numpy(inp['dy'] if dy is None else dy).to(dt)
    grads = list(torch.autograd.grad(y, leaves, cot))
    dh, dx = grads[0].numpy(), grads[1].numpy()
    if c['fold'] & 2:
        dx = dx * (inp['x'] > 0)                             # the ReLU below, folded into this filter's dx
    return dict(y=y.detach().numpy(), pre=pre.detach().numpy(), dh=dh, dx=dx,
                db=grads[2].numpy() if b is not None else None)


@functools.lru_cache(maxsize=None)
def _statements(name):
    c = next(c for c in CASES if c['name'] == name)
    w64 = statement(c, torch.float64)
    mask = (w64['pre'] > 0).astype(np.float64) if c['relu'] else None
    dy = None
    if c['fold'] & 1:                                        # the caller vouches: the cotangent is masked already
        dy = (inputs(c)['dy'] * mask[:, :, :c['Nin']]).astype(np.float32)
        w64 = statement(c, torch.float64, dy=dy)
    return w64, statement(c, torch.float32, mask, dy), mask, dy


def statements(c):
    """(float64 statement, fp32 statement, the ReLU mask [B,F,N] or None, the cotangent a fold-bit-0 caller passes or
    None) of a filter case.  Cached."""
    return _statements(c['name'])


def powers_statement(S, K, dt):
    """[..., K, N, N]: S^0 .. S^(K-1) as a chain of products in numpy dtype dt (K = 0 gives the identity, like K = 1)."""
    S = np.asarray(S).astype(dt)
    P = [np.broadcast_to(np.eye(S.shape[-1], dtype=dt), S.shape).copy()]
    for k in range(1, K):
        P.append(np.matmul(P[-1], S) if k > 1 else S.copy())
    return np.stack(P, -3)


def allowed_error(rep):
    """The largest error f64_yardstick.gap allows on a tensor with report `rep`."""
    return MAX_K * rep['max32'] + ULPS * ULP * rep['scale']


# ---- an independent formulation, and the wrong variants ---------------------------------------------------------------
def applies(c, wrong):
    """Does the wrong variant change the result of the case at all?"""
    if c['entry'] == 'matrixPowersBatch':
        return wrong == 'short_chain' and c['K'] >= 3
    E, K, N, Nin = c['E'], c['K'], c['N'], c['Nin']
    return {'adjoint_S': K > 1 and Nin > 1,                # (one node: only diagonal entries of the powers are read)
            'drop_last_tap': True, 'edge1_missing_dx': E > 1,
            'absent_nodes': Nin < N and K >= 3, 'short_chain': c['entry'] in PRE_POWERED and K >= 3,
            'db_summed': c['bias'] == 'node'}[wrong]


def explicit(c, wrong=None):
    """The same operation in numpy float64 as einsums over explicit matrix powers (numpy.linalg.matrix_power), every
    gradient by its formula, not by autograd:
        y = b + sum_{e,k} h_{e,k} (x P_{e,k}),  dh_{e,k} = sum_{b,n} dy (x P_{e,k})^T,  dx = sum_{e,k} h_{e,k}^T dy P_{e,k}^T.
    wrong: one of WRONG -- S in place of S^T in the adjoint; the last tap dropped; edge feature 1 left out of the dx sum;
    the missing nodes absent from the graph (S[:Nin,:Nin]) instead of zero rows; the last power one product short; a
    per-node bias gradient summed over the nodes."""
    inp = inputs(c)
    _, _, mask, dy_masked = statements(c)
    h, x = inp['h'].astype(np.float64), inp['x'].astype(np.float64)
    S = inp['S'].astype(np.float32).astype(np.float64)
    if S.ndim == 3:
        S = S[None]
    F, E, K, G = h.shape
    B, N, Nin = x.shape[0], S.shape[-1], x.shape[2]
    if wrong == 'absent_nodes':
        S = S.copy()
        S[..., Nin:, :] = 0
        S[..., :, Nin:] = 0
    P = [[np.linalg.matrix_power(S[:, e], k) for k in range(K)] for e in range(E)]
    if wrong == 'short_chain':
        for e in range(E):
            P[e][K - 1] = P[e][K - 2]
    taps = range(K - 1) if wrong == 'drop_last_tap' else range(K)
    xp = np.zeros((B, G, N))
    xp[:, :, :Nin] = x
    y = np.zeros((B, F, N))
    for e in range(E):
        for k in taps:
            y += np.einsum('fg,bgn->bfn', h[:, e, k], xp @ P[e][k])
    if inp['b'] is not None:
        y += inp['b'].astype(np.float64)
    dyp = np.zeros((B, F, N))
    dyp[:, :, :Nin] = inp['dy'] if dy_masked is None else dy_masked
    if c['relu']:
        y, dyp = y * mask, dyp * mask
    dh, dx = np.zeros(h.shape), np.zeros((B, G, N))
    for e in range(E):
        for k in taps:
            dh[:, e, k] = np.einsum('bfn,bgn->fg', dyp, xp @ P[e][k])
            if not (wrong == 'edge1_missing_dx' and e == 1):
                back = P[e][k] if wrong == 'adjoint_S' else np.swapaxes(P[e][k], -1, -2)
                dx += np.einsum('fg,bfn->bgn', h[:, e, k], dyp) @ back
    dx = dx[:, :, :Nin]
    if c['fold'] & 2:
        dx = dx * (inp['x'] > 0)
    db = None
    if c['bias'] == 'feat':
        db = dyp.sum((0, 2)).reshape(F, 1)
    elif c['bias'] == 'node':
        db = dyp.sum(0)
        if wrong == 'db_summed':
            db = np.broadcast_to(db.sum(1, keepdims=True), db.shape)
    return dict(y=y[:, :, :Nin], dh=dh, dx=dx, db=db)


def explicit_powers(S, K, wrong=None):
    """[..., K, N, N] by numpy.linalg.matrix_power in float64; wrong = 'short_chain': the last power one product short."""
    S = np.asarray(S, np.float64)
    P = [np.linalg.matrix_power(S, k) for k in range(max(K, 1))]
    if wrong == 'short_chain':
        P[K - 1] = P[K - 2]
    return np.stack(P, -3)

