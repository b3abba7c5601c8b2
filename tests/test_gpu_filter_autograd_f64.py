"""GPU (-m gpu): the public, differentiable graph-filter API of graphML.py -- LSIGF, BatchLSIGF, GraphFilter,
GraphFilterBatch, GraphFilterBatchGSO, forward_node_major, _LSIGFFunction.apply with its fold bits, matrixPowersBatch --
on every route of _LSIGFFunction (LDS-resident, dense, mixed) and of the pre-powered family, against the float64
statement of the same call (tests/filter_autograd_cases.py: the case list, the statements, the routes), with the fp32 CPU
statement as the yardstick (tests/f64_yardstick.py, factors unchanged, per tensor, scale = max |want|).
tests/test_filter_autograd_cases.py shows on the CPU that each listed mistake misses every case it applies to by more
than 1000 x what the yardstick allows.

Per case: the entry point runs on the device; the route is asserted by counting the calls of graphML._lsigf_large,
._lsigf_large_backward, ._LSIGFFunction._dense_dx and _native.gemm_kmajor through wrappers that call through unchanged;
y, dh, dx and db are held to float64 (the split-f16 forward to the same yardstick); exact zeros (a ReLU's, a folded
mask's, a per-node bias gradient's columns beyond Nin) are asserted bit for bit; every input lives between NaN margins
and the whole buffer must keep its bits; every call is made twice for the same bytes.  matrixPowersBatch: powers 0 and 1
bit for bit, the others through the same yardstick (fp32 GSOs) or within 8 N 2^-53 max |P_k| of numpy float64 (fp64
GSOs: another summation order of an N-term float64 dot product).  This surface has no emulation twin: the emulation
drives the C ABI, and the launches underneath have their emulation tests."""
import numpy as np
import pytest
import torch

import filter_autograd_cases as fa
from f64_yardstick import gap

pytestmark = pytest.mark.gpu
MARGIN = 64                                  # elements of NaN on either side of every input


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


class Placed:
    """A numpy array inside a larger device buffer: NaN margins on both sides, the bits of all of it remembered."""

    def __init__(self, a, dev):
        t = torch.from_numpy(np.ascontiguousarray(a))
        n = t.numel()
        self.flat = torch.full((n + 2 * MARGIN,), float('nan'), dtype=t.dtype, device=dev)
        self.flat[MARGIN:MARGIN + n] = t.reshape(-1).to(dev)
        self.view = self.flat[MARGIN:MARGIN + n].view(t.shape)
        self.bits = self._bits().clone()

    def _bits(self):
        return self.flat.view(torch.int32 if self.flat.element_size() == 4 else torch.int64)

    def intact(self):
        return torch.equal(self._bits(), self.bits)


class Calls:
    """Counts the calls of the four functions that tell the routes apart; the wrappers call through unchanged."""
    KEYS = ('large', 'large_bwd', 'dense_dx', 'gemm')

    def __init__(self, monkeypatch):
        from gnn_pathplanning_amd import _native
        from gnn_pathplanning_amd import graphML as gml
        self.n = dict.fromkeys(self.KEYS, 0)

        def wrap(key, fn):
            def counted(*a, **k):
                self.n[key] += 1
                return fn(*a, **k)
            return counted
        monkeypatch.setattr(gml, '_lsigf_large', wrap('large', gml._lsigf_large))
        monkeypatch.setattr(gml, '_lsigf_large_backward', wrap('large_bwd', gml._lsigf_large_backward))
        monkeypatch.setattr(gml._LSIGFFunction, '_dense_dx', staticmethod(wrap('dense_dx', gml._LSIGFFunction._dense_dx)))
        monkeypatch.setattr(_native, 'gemm_kmajor', wrap('gemm', _native.gemm_kmajor))

    def take(self):
        got = tuple(self.n[k] for k in self.KEYS)
        self.n = dict.fromkeys(self.KEYS, 0)
        return got


def _bytes(t):
    return None if t is None else t.detach().cpu().numpy().tobytes()


def _all_plus_zero(a):
    return not np.ascontiguousarray(a, np.float32).view(np.int32).any()


def _hold(name, route, got, want64, ref32):
    ok, rep = gap(got, want64, ref32)
    print('RATIO %s %s rms %.3g (fp32 statement %.3g: x %.2f) max %.3g (%.3g: x %.2f) scale %.3g'
          % (route, name, rep['rms'], rep['rms32'], rep['rms'] / max(rep['rms32'], 1e-300), rep['max'], rep['max32'],
             rep['max'] / max(rep['max32'], 1e-300), rep['scale']))
    assert ok, '%s: %s' % (name, {k: '%.3g' % v for k, v in rep.items()})


def _run(c, T, needs, calls):
    """One forward + backward of the case through its entry point, with the tensors of `needs` requiring grad.
    Returns dict(y, dh, dx, db) as device tensors in the statement's feature-major layout (None where no gradient came
    back) and the calls counted."""
    from gnn_pathplanning_amd import graphML as gml
    leaf = lambda k: None if T[k] is None else T[k].view.detach().requires_grad_(k in needs)     # noqa: E731
    h, x, b = leaf('h'), leaf('x'), leaf('b')
    S, entry, prec = T['S'].view, c['entry'], c['prec']
    G, F, K, E = c['G'], c['F'], c['K'], c['E']
    calls.take()
    if entry == 'LSIGF':
        y = gml.LSIGF(h, S, x, b, precision=prec)
    elif entry == 'BatchLSIGF':
        y = gml.BatchLSIGF(h, S, x, b, precision=prec)
    elif entry == 'apply':
        y = gml._LSIGFFunction.apply(h, S, x, b, c['batched'], None, True, c['relu'], prec, None, c['fold'])
    else:
        cls = {'GraphFilter': gml.GraphFilter, 'GraphFilterBatch': gml.GraphFilterBatch,
               'GraphFilterBatchGSO': gml.GraphFilterBatchGSO,
               'forward_node_major': gml.GraphFilterBatch if c['batched'] else gml.GraphFilter}[entry]
        gf = cls(G, F, K, E, bias=b is not None, precision=prec)
        gf.weight = torch.nn.Parameter(h, requires_grad='h' in needs)
        if b is not None:
            gf.bias = torch.nn.Parameter(b, requires_grad='b' in needs)
        h, b = gf.weight, gf.bias
        gf.addGSO(S)
        if entry == 'GraphFilterBatchGSO':
            assert calls.take() == (0, 0, 0, fa.powers_gemms(c)), c['name']
            assert gf.SK.dtype == (torch.float64 if c['f64'] else torch.float32)
            assert gf.SK.shape == (c['B'], E, K, c['N'], c['N'])
        y = gf.forward_node_major(x, relu=c['relu']) if entry == 'forward_node_major' else gf(x)
    y.backward(T['dy'], retain_graph=c['retain'])
    counted = calls.take()
    leaves = dict(dh=h, dx=x, db=b)
    out = {k: None if t is None or t.grad is None else t.grad.clone() for k, t in leaves.items()}
    if c['retain']:                          # a second backward over the retained graph doubles .grad, exactly
        y.backward(T['dy'])
        for k, t in leaves.items():
            if out[k] is not None:
                assert _bytes(t.grad) == _bytes(out[k] * 2), (c['name'], k)
    out['y'] = y.detach()
    if entry in fa.NODE_MAJOR:
        out['y'] = out['y'].permute(0, 2, 1)
        out['dx'] = None if out['dx'] is None else out['dx'].permute(0, 2, 1)
    return {k: None if v is None else v.contiguous() for k, v in out.items()}, counted


def _place_inputs(c, dev):
    inp = fa.inputs(c)
    _, _, _, dy_masked = fa.statements(c)
    nm = c['entry'] in fa.NODE_MAJOR
    turn = (lambda a: a.transpose(0, 2, 1)) if nm else (lambda a: a)
    T = dict(h=Placed(inp['h'], dev), x=Placed(turn(inp['x']), dev), b=None if inp['b'] is None else Placed(inp['b'], dev),
             S=Placed(inp['S'] if c['f64'] else inp['S'].astype(np.float32), dev))
    dy = turn(inp['dy'] if dy_masked is None else dy_masked)
    if c['dy_view']:                         # every other element of a buffer of twice the width
        wide = np.full(dy.shape + (2,), np.nan, np.float32)
        wide[..., 0] = dy
        T['dy_buf'] = Placed(wide, dev)
        T['dy'] = T['dy_buf'].view[..., 0]
        assert not T['dy'].is_contiguous()
    else:
        T['dy_buf'] = Placed(dy, dev)
        T['dy'] = T['dy_buf'].view
    return T


def _run_filter_case(c, dev, calls):
    B, N, Nin, F, G = c['B'], c['N'], c['Nin'], c['F'], c['G']
    route = fa.filter_route(c)
    T = _place_inputs(c, dev)
    w64, w32, mask, _ = fa.statements(c)
    full = 'hxb' if c['bias'] else 'hx'
    got, counted = _run(c, T, full, calls)
    again, counted2 = _run(c, T, full, calls)
    torch.cuda.synchronize()
    # ---- the route
    assert counted == counted2 == fa.expected_calls(c, full), (c['name'], counted, fa.expected_calls(c, full))
    # ---- the inputs and their margins
    for k in ('h', 'x', 'b', 'S', 'dy_buf'):
        assert T[k] is None or T[k].intact(), (c['name'], k)
    # ---- the same bytes twice
    for k in ('y', 'dh', 'dx', 'db'):
        assert _bytes(got[k]) == _bytes(again[k]), (c['name'], k)
    # ---- against float64
    assert got['y'].shape == (B, F, Nin) and got['dx'].shape == (B, G, Nin) and got['dh'].shape == w64['dh'].shape
    assert (got['db'] is None) == (c['bias'] is None)
    res = {k: None if v is None else v.cpu().numpy() for k, v in got.items()}
    for k in ('y', 'dh', 'dx', 'db'):
        if res[k] is not None:
            assert res[k].shape == w64[k].shape and res[k].dtype == np.float32, (c['name'], k)
            _hold('%s/%s' % (c['name'], k), route, res[k], w64[k], w32[k])
    # ---- exact zeros
    if c['relu']:
        live = mask[:, :, :Nin] > 0
        assert np.array_equal(res['y'] > 0, live) and _all_plus_zero(res['y'][~live]), c['name']
    if c['fold'] & 2:
        dead = fa.inputs(c)['x'] == 0
        assert dead.any() and _all_plus_zero(res['dx'][dead]), c['name']
    if c['bias'] == 'node' and Nin < N:
        assert _all_plus_zero(res['db'][:, Nin:]), c['name']
    # ---- partial requires_grad: the others get none, the one asked for is the all-grad run's to the bit
    if c['needs'] != 'hxb':
        part, counted = _run(c, T, c['needs'], calls)
        torch.cuda.synchronize()
        assert counted == fa.expected_calls(c), (c['name'], counted, fa.expected_calls(c))
        assert _bytes(part['y']) == _bytes(got['y'])
        for k, key in (('h', 'dh'), ('x', 'dx'), ('b', 'db')):
            if k in c['needs']:
                assert part[key] is not None and _bytes(part[key]) == _bytes(got[key]), (c['name'], key)
            else:
                assert part[key] is None, (c['name'], key)


def _run_powers_case(c, dev, calls):
    from gnn_pathplanning_amd import graphML as gml
    S = fa.inputs(c)['S']
    K, N = c['K'], c['N']
    Sh = S if c['f64'] else S.astype(np.float32)
    if c.get('s_view'):                      # a transposed view of the buffer that holds S^T
        placed = Placed(np.swapaxes(Sh, -1, -2), dev)
        Sd = placed.view.transpose(-1, -2)
        assert not Sd.is_contiguous()
    else:
        placed = Placed(Sh, dev)
        Sd = placed.view
    calls.take()
    P = gml.matrixPowersBatch(Sd, K)
    counted = calls.take()
    P2 = gml.matrixPowersBatch(Sd, K)
    torch.cuda.synchronize()
    assert counted == calls.take() == (0, 0, 0, fa.powers_gemms(c)), (c['name'], counted)
    assert placed.intact(), c['name']
    assert P.dtype == Sd.dtype and P.shape == S.shape[:-2] + (K,) + S.shape[-2:]
    got = P.cpu().numpy()
    assert got.tobytes() == P2.cpu().numpy().tobytes()
    power = lambda a, k: a[..., k, :, :]                                                           # noqa: E731
    assert np.array_equal(power(got, 0), np.broadcast_to(np.eye(N, dtype=got.dtype), Sh.shape))
    assert not np.signbit(power(got, 0)).any()
    if K > 1:
        assert power(got, 1).tobytes() == Sh.tobytes()
    if c['f64']:
        want = fa.powers_statement(S, K, np.float64)
        for k in range(2, K):
            err, bound = np.abs(power(got, k) - power(want, k)).max(), 8 * N * 2.0 ** -53 * np.abs(power(want, k)).max()
            print('RATIO %s %s/P%d max %.3g, bound %.3g' % (c['route'], c['name'], k, err, bound))
            assert err <= bound, (c['name'], k, err, bound)
    else:
        want, ref = fa.powers_statement(Sh, K, np.float64), fa.powers_statement(Sh, K, np.float32)
        for k in range(2, K):
            _hold('%s/P%d' % (c['name'], k), c['route'], power(got, k), power(want, k), power(ref, k))


@pytest.mark.parametrize('case', fa.CASES, ids=fa.case_id)
def test_filter_autograd_f64(dev, monkeypatch, case):
    calls = Calls(monkeypatch)
    if case['entry'] == 'matrixPowersBatch':
        _run_powers_case(case, dev, calls)
    else:
        _run_filter_case(case, dev, calls)
