"""GPU (-m gpu): the training calls of the team filter on neighbour lists on the MI355X (gnnpp_team_lists_transpose,
gnnpp_lsigf_team_lists_fwd_save, gnnpp_lsigf_team_lists_input_grad), and graphML.lsigf_team_train's autograd.  The
byte equalities include/gnnpp.h states, every result against a float64 statement (f64_yardstick), the error tables.
Cases and runner: tests/filter_team_train_cases.py."""
import numpy as np
import pytest
import torch

import filter_f64_cases as fc
import filter_team_cases as tc
import filter_team_train_cases as tt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def bk(dev):
    from gnn_pathplanning_amd import _native
    return fc.TorchBackend(_native.lib(), dev)


@pytest.mark.parametrize('case', tt.TRANSPOSE_CASES + tt.GPU_TRANSPOSE_CASES, ids=lambda c: c['name'])
def test_lists_transpose(bk, case):
    tt.run_transpose(bk, case)


def test_lists_transpose_errors(bk):
    tt.run_transpose_errors(bk)


@pytest.mark.parametrize('prec', tc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('case', tt.FILTER_CASES + tt.GPU_FILTER_CASES, ids=lambda c: c['name'])
def test_forward_keeps_tap_signals(bk, case, prec):
    tt.run_save(bk, case, prec)


@pytest.mark.parametrize('case', tt.FILTER_CASES + tt.GPU_FILTER_CASES, ids=lambda c: c['name'])
def test_input_grad_is_the_filter_on_the_transposed_lists(bk, case):
    tt.run_input_grad(bk, case)


def test_train_call_errors(bk):
    tt.run_train_errors(bk)


# ---- graphML.lsigf_team_train -----------------------------------------------------------------------------------------
def _statement(h, S, x, b, relu, dy, dt, mask=None):
    """y [B,F,N] and the gradients (dh, dx [B,G,N], db) of sum(y * dy) in numpy dtype dt.  relu: the cotangent is
    masked with `mask` (the call's own y > 0), so the statement is linear in dy."""
    F, E, K, G = h.shape
    y = fc.lsigf_statement(h, S, x, b, relu, dt)
    g = dy.astype(dt) * mask.astype(dt) if relu else dy.astype(dt)
    ht = np.ascontiguousarray(h.transpose(3, 1, 2, 0))
    dx = fc.lsigf_statement(ht, S, g.astype(dt), None, 0, dt, transposed=True)
    B, N = x.shape[0], x.shape[2]
    Z = fc.tap_signals(S, x, K, E, dt).reshape(E, K, B, N, G)
    dh = np.einsum('bfn,ekbng->fekg', g, Z)
    db = None if b is None else (g.sum((0, 2)).reshape(F, 1) if b.size == F else g.sum(0))
    return y, dh, dx, db


AUTOGRAD_CASES = [tt.FILTER_CASES[i] for i in (1, 2, 4, 5, 7, 10, 11)]


@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('case', AUTOGRAD_CASES, ids=lambda c: c['name'])
def test_lsigf_team_train_gradients_against_float64(dev, case, relu):
    """y, dh, dx and db of graphML.lsigf_team_train for a random cotangent.  relu=False is a linear statement; with
    relu=True the statement masks the cotangent with the call's own returned y > 0 (data of the call), and y itself is
    held to float64 separately."""
    from gnn_pathplanning_amd import graphML as gml
    c = dict(case, relu=int(relu))
    B, N, G, F, K, E = c['B'], c['N'], c['G'], c['F'], c['K'], c['E']
    batched = c.get('batched', True)
    h, S, x, b = tt._filter_inputs(c)
    dy = np.random.default_rng(c['seed'] + 3).standard_normal((B, F, N)).astype(np.float32)
    ht = torch.from_numpy(h).to(dev).requires_grad_(True)
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev).requires_grad_(True)
    bt = None if b is None else torch.from_numpy(b.reshape(F, -1)).to(dev).requires_grad_(True)
    lists = gml.team_lists_from_dense(torch.from_numpy(S).to(dev))
    before = dict(gml.team_train_calls)
    y = gml.lsigf_team_train(ht, lists, xt, bt, relu=relu, batched=batched)
    y.backward(torch.from_numpy(np.ascontiguousarray(dy.transpose(0, 2, 1))).to(dev))
    torch.cuda.synchronize()
    assert gml.team_train_calls['fwd_save'] == before['fwd_save'] + 1
    assert gml.team_train_calls['input_grad'] == before['input_grad'] + 1
    assert gml.team_train_calls['transpose'] == before['transpose'] + (K > 1)
    yn = y.detach().cpu().numpy().transpose(0, 2, 1)
    mask = (yn > 0).astype(np.float64)
    w64, w32 = _statement(h, S, x, b, relu, dy, np.float64, mask), _statement(h, S, x, b, relu, dy, np.float32, mask)
    got = (yn, ht.grad.cpu().numpy(), xt.grad.cpu().numpy().transpose(0, 2, 1),
           None if b is None else bt.grad.cpu().numpy())
    for name, a, a64, a32 in zip(('y', 'dh', 'dx', 'db'), got, w64, w32):
        if a is not None:
            fc.check('%s/relu=%d/%s' % (c['name'], relu, name), a, a64, a32)


def test_symmetric_promise_equals_the_explicit_transpose(dev):
    """On a symmetric S, symmetric=True gives the bytes of lists_t=team_lists_transpose(lists) and of lists_t=None."""
    from gnn_pathplanning_amd import graphML as gml
    c = tt.FILTER_CASES[12]
    assert c['s'] == 'sym'
    B, N, G, F, K, E = c['B'], c['N'], c['G'], c['F'], c['K'], c['E']
    h, S, x, _ = tt._filter_inputs(c)
    assert (S == np.swapaxes(S, -1, -2)).all()
    lists = gml.team_lists_from_dense(torch.from_numpy(S).to(dev))
    dy = torch.from_numpy(np.random.default_rng(5).standard_normal((B, N, F)).astype(np.float32)).to(dev)
    out = []
    for kw in (dict(symmetric=True), dict(lists_t=gml.team_lists_transpose(lists, B * E, N)), {}):
        ht = torch.from_numpy(h).to(dev).requires_grad_(True)
        xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev).requires_grad_(True)
        before = gml.team_train_calls['transpose']
        y = gml.lsigf_team_train(ht, lists, xt, None, relu=True, **kw)
        assert gml.team_train_calls['transpose'] == before + (not kw)
        y.backward(dy)
        out.append((y.detach(), ht.grad, xt.grad))
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert torch.equal(a, b)


def test_gradient_sinks_receive_the_parameter_gradients(dev):
    """A parameter with a registered gradient sink (_native.register_grad_sink) gets its gradient born in the sink."""
    from gnn_pathplanning_amd import _native, graphML as gml
    c = tt.FILTER_CASES[5]
    h, S, x, b = tt._filter_inputs(c)
    ht = torch.from_numpy(h).to(dev).requires_grad_(True)
    bt = torch.from_numpy(b.reshape(-1, 1)).to(dev).requires_grad_(True)
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev)
    bucket = torch.full((ht.numel() + bt.numel(),), float('nan'), device=dev)
    _native.register_grad_sink(ht, bucket, 0)
    _native.register_grad_sink(bt, bucket, ht.numel())
    try:
        lists = gml.team_lists_from_dense(torch.from_numpy(S).to(dev))
        gml.lsigf_team_train(ht, lists, xt, bt, relu=True).sum().backward()
        assert ht.grad.data_ptr() == bucket.data_ptr()
        assert bt.grad.data_ptr() == bucket.data_ptr() + 4 * ht.numel()
        assert torch.isfinite(bucket).all()
    finally:
        _native.unregister_grad_sinks(bucket)


def test_unserved_layers_raise(dev):
    from gnn_pathplanning_amd import _native, graphML as gml
    lists = gml.team_lists_from_dense(torch.zeros(1, 1, 20, 20, device=dev))
    x = torch.zeros(1, 20, 130, device=dev, requires_grad=True)
    with pytest.raises(_native.GnnppError):
        gml.lsigf_team_train(torch.zeros(8, 1, 2, 130, device=dev), lists, x, None)
    with pytest.raises(_native.GnnppError):
        gml.lsigf_team_train(torch.zeros(8, 1, 2, 16, device=dev), lists, x[:, :, :16], None, precision='split_f16')
    with pytest.raises(_native.GnnppError):
        gml.large_graph_training('sparse')
