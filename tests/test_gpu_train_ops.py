"""GPU (-m gpu): the five launches of csrc/train_ops.hip on the MI355X through the C ABI (gnnpp_gemm_kmajor,
gnnpp_gemm_kmajor_multi, gnnpp_linear_fwd, gnnpp_policy_loss, gnnpp_adam_step) at tile, split and launch edges: every
result against a float64 statement (f64_yardstick), the bytes around every output, two calls the same bytes, the error
tables; and training.FusedAdam over more than one table of 32 tensors.  Cases and runners: tests/train_ops_cases.py."""
import io

import numpy as np
import pytest
import torch

import filter_f64_cases as fc
import train_ops_cases as to

pytestmark = pytest.mark.gpu
by_name = lambda c: c['name']                                               # noqa: E731


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def bk(dev):
    from gnn_pathplanning_amd import _native
    return fc.TorchBackend(_native.lib(), dev)


def test_gemm_plan_is_the_library_s(bk):
    to.run_gemm_plan(bk, to.GEMM_CASES + to.GPU_GEMM_CASES + to.MULTI_CASES)


@pytest.mark.parametrize('case', to.GEMM_CASES + to.GPU_GEMM_CASES, ids=by_name)
def test_gemm_kmajor_against_float64(bk, case):
    to.run_gemm(bk, case)


def test_gemm_multi_is_each_product_alone(bk):
    to.run_gemm_multi(bk)


def test_gemm_refusals(bk):
    to.run_gemm_errors(bk)


@pytest.mark.parametrize('case', to.LINEAR_CASES, ids=by_name)
def test_linear_fwd_against_float64(bk, case):
    to.run_linear(bk, case)


def test_linear_fwd_relu_at_exactly_zero(bk):
    to.run_linear_relu_zero(bk)


def test_linear_fwd_refusals(bk):
    to.run_linear_errors(bk)


@pytest.mark.parametrize('case', to.LOSS_CASES, ids=by_name)
def test_policy_loss_against_float64(bk, case):
    to.run_loss(bk, case)


def test_policy_loss_refusals(bk):
    to.run_loss_errors(bk)


@pytest.mark.parametrize('case', to.ADAM_CASES, ids=by_name)
def test_adam_step_against_float64(bk, case):
    to.run_adam(bk, case)


def test_adam_step_refusals(bk):
    to.run_adam_errors(bk)


def test_fused_adam_with_more_tensors_than_one_table(dev):
    """training.FusedAdam on a bare module of 40 parameters of ragged sizes (1 .. 1500 elements): 39 receive gradients
    (one has grad None, one a non-contiguous .grad), so every step is a table of 32 (tick) and a table of 7.  Three steps
    against torch.optim.Adam in float64 on the same gradients, the optimizer state saved and loaded into a FRESH
    optimizer after the first step (the cached pointer tables are rebuilt on the loaded moments)."""
    from gnn_pathplanning_amd.training import FusedAdam
    g = np.random.default_rng(40)
    sizes = [1, 1500, 255, 256, 1023, 1024, 1025] + [int(n) for n in g.integers(1, 1501, 33)]
    NONE, STRIDED = 5, 9
    shapes = [(n,) for n in sizes]
    shapes[STRIDED] = (24, 31)
    p0 = [g.standard_normal(s).astype(np.float32) for s in shapes]
    grads = [[g.standard_normal(s).astype(np.float32) for s in shapes] for _ in range(3)]
    lr, wd, eps = 1e-2, 1e-3, 1e-8

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(p).clone()) for p in p0])

    def feed(net, s, dt, device):
        for i, (p, gr) in enumerate(zip(net.ps, grads[s])):
            if i == NONE:
                p.grad = None
            elif i == STRIDED and device.type == 'cuda':
                p.grad = torch.from_numpy(np.ascontiguousarray(gr.T)).to(device).t()      # the same values, column-major
                assert not p.grad.is_contiguous()
            else:
                p.grad = torch.from_numpy(gr).to(device=device, dtype=dt)

    net = Net().to(dev)
    opt = FusedAdam(net.parameters(), lr=lr, weight_decay=wd, eps=eps)
    traj = []
    for s in range(3):
        feed(net, s, torch.float32, dev)
        opt.step()
        traj.append([p.detach().cpu().numpy().copy() for p in net.ps])
        assert float(opt.state['gnnpp_group_0']['counter'][0]) == s + 1
        assert len(opt._gnnpp_tables[0]['tables']) == 2 and opt._gnnpp_tables[0]['tables'][1].count == 7
        tables = opt._gnnpp_tables[0]['tables']
        live = [p for i, p in enumerate(net.ps) if i != NONE]
        # the tables the step just used point at the moments the optimizer holds NOW
        assert [tables[0].m[j] for j in range(32)] == [opt.state[p]['exp_avg'].data_ptr() for p in live[:32]]
        assert [tables[1].v[j] for j in range(7)] == [opt.state[p]['exp_avg_sq'].data_ptr() for p in live[32:]]
        if s < 2:
            buf = io.BytesIO()
            torch.save(opt.state_dict(), buf)
            buf.seek(0)
            if s == 0:                       # into the SAME optimizer, which holds tables on the moments the load replaces
                old = [opt.state[p]['exp_avg'] for p in live]                 # (kept alive: their blocks are not reused)
                opt.load_state_dict(torch.load(buf, map_location='cpu'))
                assert all(opt.state[p]['exp_avg'].data_ptr() != o.data_ptr() for p, o in zip(live, old))
            else:                            # ... and into a fresh one
                opt = FusedAdam(net.parameters(), lr=lr, weight_decay=wd, eps=eps)
                opt.load_state_dict(torch.load(buf, map_location='cpu'))
            assert '_gnnpp_tables' not in opt.__dict__
    f32 = lambda v: float(np.float32(v))                                     # noqa: E731
    want = {}
    for dt in (torch.float64, torch.float32):
        ref = Net().to(dt)
        ro = torch.optim.Adam(ref.parameters(), lr=f32(lr), betas=(f32(0.9), f32(0.999)), eps=f32(eps),
                              weight_decay=f32(wd), foreach=False)
        want[dt] = []
        for s in range(3):
            feed(ref, s, dt, torch.device('cpu'))
            ro.step()
            want[dt].append([p.detach().numpy().copy() for p in ref.ps])
    for s in range(3):
        for i in range(len(shapes)):
            name = 'step %d, parameter %d %s' % (s + 1, i, shapes[i])
            if i == NONE:
                assert np.array_equal(traj[s][i], p0[i]), name
            else:
                to.check(name, traj[s][i], want[torch.float64][s][i], want[torch.float32][s][i])
