"""GPU (-m gpu): the team graph filter (graphs of up to 1024 nodes spread over workgroups, csrc/lsigf_team_kernel.hip)
on the MI355X.

The C calls against float64 with the fp32 numpy statement as the yardstick (runner tests/filter_team_cases.py over
tests/filter_f64_cases.py, unchanged): the matrix of tests/test_emu_filter_team.py at larger batches, plus N = 128, 129,
512, 1000 and 8 x 1024, and a GSO from BatchedRollout.gso on a 128 x 128 map.  Then the opt-in route
(`largeGraphFilter='lists'`) through DecentralPlannerNet: logits against the policy oracle at the project's parity
tolerance 1e-4, actions wherever the oracle's top-two margin exceeds 1e-5, agreement with the same net under 'dense' to
1e-4; a two-layer, two-edge-feature planner on a GSO larger than the team; GraphedPolicyStep (replay == eager, byte for
byte, also on a side stream); a BatchedRollout run; train mode (the dense route's gradients)."""
import numpy as np
import pytest
import torch

import filter_f64_cases as fc
import filter_team_cases as tc
from oracle import policy_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def bk(dev):
    from gnn_pathplanning_amd import _native
    lib = _native.lib()
    assert hasattr(lib, 'gnnpp_lsigf_team_fwd')
    return fc.TorchBackend(lib, dev)


def _cases():
    C = []
    i = 0
    for N in (113, 130, 200, 257):
        for K in (1, 2, 3, 4):
            for E in (1, 2):
                G, F = ((128, 128), (48, 40), (33, 128))[i % 3]
                bias = (None, 'feat', 'node')[(i // 3) % 3]
                C.append(dict(name='team/N%dK%dE%d/G%dF%d/%s' % (N, K, E, G, F, bias), seed=200 + i, B=(8, 3, 5)[i % 3],
                              N=N, G=G, F=F, K=K, E=E, bias=bias, relu=i % 2, f64=(i // 2) % 2,
                              batched=bool((i // 4) % 2 == 0), s=(None, 'sym', 'full_empty')[i % 3]))
                i += 1
    for j, N in enumerate((40, 128, 129, 512, 1000)):
        C.append(dict(name='team/N%dK3' % N, seed=300 + j, B=(8, 4)[j % 2], N=N, G=128, F=128, K=3, E=1, bias='feat',
                      relu=1, s='full_empty' if j % 2 else None))
    C.append(dict(name='team/B8N1024K3', seed=310, B=8, N=1024, G=128, F=128, K=3, E=1, bias='feat', relu=1))
    C.append(dict(name='team/B2N1024K4E2/G48F40/sharedS/f64S', seed=311, B=2, N=1024, G=48, F=40, K=4, E=2, bias='node',
                  batched=False, f64=1, s='full_empty'))
    return C


CASES = _cases()
HEAD = [
    dict(name='team/N130K3', seed=401, B=8, N=130, G=128, F=128, K=3, E=1, bias='feat'),
    dict(name='team/N200K2/G48F40/f64S/full_empty', seed=402, B=3, N=200, G=48, F=40, K=2, E=1, bias='feat', f64=1,
         s='full_empty'),
    dict(name='team/N113K1E2/G33F128/nobias', seed=403, B=5, N=113, G=33, F=128, K=1, E=2),
    dict(name='team/N40K4', seed=404, B=4, N=40, G=128, F=128, K=4, E=1, bias='feat'),
    dict(name='team/B8N1024K3', seed=405, B=8, N=1024, G=128, F=128, K=3, E=1, bias='feat'),
    dict(name='team/N1000K4E2', seed=406, B=2, N=1000, G=128, F=128, K=4, E=2, bias='feat', s='sym'),
]


@pytest.mark.parametrize('prec', tc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_team_lsigf_f64(bk, case, prec):
    # (the large cases at two scales: their float64 statements are the test's cost)
    for scale in (fc.SCALES if case['N'] < 1000 else (1e-3, 1.0)):
        tc.run_team(bk, case, prec, scale)


@pytest.mark.parametrize('prec', tc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('case', HEAD, ids=lambda c: c['name'])
def test_team_head_f64(bk, case, prec):
    for scale in (fc.SCALES if case['N'] < 1000 else (1e-3, 1.0)):
        tc.run_team_head(bk, case, prec, scale)


def test_team_errors_version_determinism(bk):
    tc.run_errors(bk)
    assert bk.lib.gnnpp_version() == 330
    for prec in tc.PRECS:
        tc.run_team(bk, CASES[10], prec, 1.0, twice=True)
        tc.run_team(bk, dict(name='team/B8N1024K3/twice', seed=312, B=8, N=1024, G=128, F=128, K=3, E=1, bias='feat'),
                    prec, 1.0, twice=True)


def _instances(seed, B, N, W):
    from rollout_team_cases import make_instances
    return make_instances(np.random.default_rng(seed), B, N, W, W, 0.05)


def test_team_rollout_gso_128_map(bk, dev):
    """S from BatchedRollout.gso of 1024-agent teams on a 128 x 128 map (a radius graph: a few dozen non-zeros per
    column), through gnnpp_lsigf_team_fwd and graphML.lsigf_team."""
    from gnn_pathplanning_amd import graphML as gml
    from gnn_pathplanning_amd.rollout import BatchedRollout
    B, N, G, F, K = 2, 1024, 128, 128, 3
    grids, starts, goals = _instances(31, B, N, 128)
    S = BatchedRollout(grids, starts, goals, 4, dev).gso()                     # [B,N,N]
    assert S.shape == (B, N, N)
    deg = (S != 0).sum(1)
    assert 0 < deg.float().mean().item() < 200
    h, _, x, b = fc.make_inputs(32, B, N, G, F, K, 1, bias='feat')
    S_np = S.cpu().numpy()[:, None]
    ht, xt = torch.from_numpy(h).to(dev), torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev)
    bt = torch.from_numpy(b).to(dev).reshape(F, 1)
    want = fc.lsigf_statement(h, S_np, x, b, 1, np.float64)
    ref = fc.lsigf_statement(h, S_np, x, b, 1, np.float32)
    for prec in ('fp32', 'fp32_mfma'):
        y = gml.lsigf_team(ht, S[:, None], xt, bt, relu=True, precision=prec)
        torch.cuda.synchronize(dev)
        fc.check('rollout_gso/%s' % prec, y.cpu().numpy().transpose(0, 2, 1), want, ref)


def _planner(dev, N, K, route, seed=23, **cfg):
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet

    class Cfg:
        num_agents, nGraphFilterTaps, device, largeGraphFilter = N, K, dev, route
    for k, v in cfg.items():
        setattr(Cfg, k, v)
    return DecentralPlannerNet(Cfg()).to(dev).eval()


def test_team_planner_lists_against_oracle_and_dense(dev):
    """Mirrors test_gpu_rollout_team.py::test_team_closed_loop_rollout_with_policy under largeGraphFilter='lists'."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    B, N, W = 4, 200, 50
    grids, starts, goals = _instances(15, B, N, W)
    sd = orc.init_state_dict(3, seed=23)
    net = _planner(dev, N, 3, 'lists')
    dense = _planner(dev, N, 3, 'dense')
    assert net.largeGraphFilter == 'lists' and dense.largeGraphFilter == 'dense'
    net.load_state_dict(sd)
    dense.load_state_dict(sd)
    env = BatchedRollout(grids, starts, goals, 8, dev, tie_mode='lowest')
    for t in range(4):
        obs = env.observe()
        S = env.gso()
        net.addGSO(S)
        dense.addGSO(S)
        logits = net.forward_logits(obs)                                  # [N,B,5]
        ld = dense.forward_logits(obs)
        with torch.no_grad():
            want = torch.stack(orc.policy_forward(sd, S.cpu(), obs.cpu()), 0)
        err, err_d = (logits.cpu() - want).abs().max().item(), (logits - ld).abs().max().item()
        print('step %d: |lists - oracle| = %.3g, |lists - dense| = %.3g' % (t, err, err_d))
        assert err <= 1e-4
        assert err_d <= 1e-4
        acts = net.decode_actions(logits).cpu().numpy()                   # [B,N]
        margin = torch.topk(want, 2, dim=-1).values
        clear = ((margin[..., 0] - margin[..., 1]) > 1e-5).numpy().T
        assert (acts[clear] == want.argmax(-1).numpy().T[clear]).all()
        env.move(logits=logits)
    # the list form of forward(): N views [B,5] of the same logits
    net.addGSO(S)
    out = net(obs)
    assert len(out) == N and torch.equal(torch.stack(out, 0), net.forward_logits(obs))


def test_team_rollout_run_ends_done(dev):
    from gnn_pathplanning_amd.rollout import BatchedRollout
    B, N, W = 4, 200, 50
    grids, starts, goals = _instances(15, B, N, W)
    net = _planner(dev, N, 3, 'lists')
    net.load_state_dict(orc.init_state_dict(3, seed=23))
    out = BatchedRollout(grids, starts, goals, 12, dev).run(net, check_every=4)
    assert out['done'].all() and out['steps'] <= 12


def test_team_two_layer_two_edge_features_larger_gso(dev):
    """L = 2, E = 2, widths 64 and 48, a GSO of 150 nodes for 130 agents: per-layer gnnpp_lsigf_team_fwd and
    gnnpp_filter_head_team_fwd through the module API, against the policy oracle -- and the 'dense' route on the same
    inputs, held to the same 1e-4.  With several layers AND a GSO larger than the team every layer zero-pads its input
    again (graphML.py:2464-2476, and the oracle): a route that carries the first layer's outputs on the extra nodes
    into the second layer is 0.067 off on these inputs."""
    B, N, Ns = 3, 130, 150
    torch.manual_seed(5)
    cfg = dict(nGraphFilterTaps=[2, 3], dimNodeSignals=[64, 48], numEdgeFeatures=2)
    net = _planner(dev, N, [2, 3], 'lists', **cfg)
    dense = _planner(dev, N, [2, 3], 'dense', **cfg)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    for k in sd:                                                        # non-trivial BatchNorm statistics
        if k.endswith('running_mean'):
            sd[k] = 0.1 * torch.randn_like(sd[k])
        elif k.endswith('running_var'):
            sd[k] = 0.5 + torch.rand_like(sd[k])
    net.load_state_dict(sd)
    dense.load_state_dict(sd)
    g = torch.Generator().manual_seed(6)
    obs = torch.rand(B, N, 3, 11, 11, generator=g)
    S = ((torch.rand(B, 2, Ns, Ns, generator=g) < 0.05) * torch.rand(B, 2, Ns, Ns, generator=g) / 3.0)
    net.addGSO(S.to(dev))
    dense.addGSO(S.to(dev))
    logits = net.forward_logits(obs.to(dev))
    ld = dense.forward_logits(obs.to(dev))
    assert logits.shape == (N, B, 5)
    with torch.no_grad():
        want = torch.stack(orc.policy_forward(sd, S, obs), 0)
    assert ld.shape == (N, B, 5)
    err, err_d = (logits.cpu() - want).abs().max().item(), (ld.cpu() - want).abs().max().item()
    print('|lists - oracle| = %.3g, |dense - oracle| = %.3g' % (err, err_d))
    assert err <= 1e-4
    assert err_d <= 1e-4


def test_team_unserved_combinations(dev):
    """G / F > 128 under 'lists' raises; split-f16 keeps the dense form (documented)."""
    from gnn_pathplanning_amd import _native, graphML as gml
    B, N = 2, 130
    g = torch.Generator().manual_seed(7)
    S = ((torch.rand(B, 1, N, N, generator=g) < 0.05) * torch.rand(B, 1, N, N, generator=g)).to(dev)
    with torch.no_grad():
        wide = gml.GraphFilterBatch(130, 16, 2, largeGraphFilter='lists').to(dev)
        wide.addGSO(S)
        with pytest.raises(_native.GnnppError):
            wide(torch.rand(B, 130, N, device=dev))
        ok = gml.GraphFilterBatch(24, 16, 3, largeGraphFilter='lists').to(dev)
        ref = gml.GraphFilterBatch(24, 16, 3).to(dev)
        ref.load_state_dict(ok.state_dict())
        ok.addGSO(S)
        ref.addGSO(S)
        x = torch.rand(B, 24, N, device=dev)
        assert (ok(x) - ref(x)).abs().max().item() <= 1e-5
        f16 = gml.GraphFilterBatch(24, 16, 3, precision='split_f16', largeGraphFilter='lists').to(dev)
        f16.load_state_dict(ok.state_dict())
        f16.addGSO(S)
        assert torch.equal(f16(x), ref(x))
    with pytest.raises(_native.GnnppError):
        gml.GraphFilterBatch(24, 16, 3, largeGraphFilter='sparse')


def test_team_graphed_policy_step_equals_eager(dev):
    from gnn_pathplanning_amd.rollout import BatchedRollout, GraphedPolicyStep
    B, N, W = 2, 200, 50
    grids, starts, goals = _instances(16, B, N, W)
    net = _planner(dev, N, 3, 'lists')
    net.load_state_dict(orc.init_state_dict(3, seed=23))
    env = BatchedRollout(grids, starts, goals, 8, dev, tie_mode='lowest')
    obs, S = env.observe(), env.gso()
    net.addGSO(S)
    eager = torch.stack(net(obs), 0).clone()
    step = GraphedPolicyStep(net, obs, S)
    # the workspace travels with the packs
    assert any(isinstance(b, torch.Tensor) and b.dtype is torch.uint8 for b in step._held)
    out = torch.stack(step(obs, S), 0)
    torch.cuda.synchronize(dev)
    assert out.cpu().numpy().tobytes() == eager.cpu().numpy().tobytes()
    env.move(logits=eager)
    obs2, S2 = env.observe(), env.gso()
    net.addGSO(S2)
    eager2 = torch.stack(net(obs2), 0).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out2 = torch.stack(step(obs2, S2), 0).clone()
    side.synchronize()
    assert out2.cpu().numpy().tobytes() == eager2.cpu().numpy().tobytes()


def test_team_train_mode_keeps_dense_gradients(dev):
    B, N = 2, 130
    nets = [_planner(dev, N, 2, route) for route in ('lists', 'dense')]
    nets[1].load_state_dict(nets[0].state_dict())
    g = torch.Generator().manual_seed(9)
    obs = torch.rand(B, N, 3, 11, 11, generator=g).to(dev)
    S = ((torch.rand(B, N, N, generator=g) < 0.05) * torch.rand(B, N, N, generator=g)).to(dev)
    grads = []
    for net in nets:
        net.train()
        net.addGSO(S)
        net.forward_logits(obs).square().sum().backward()
        grads.append({k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and 'GFL.0.weight' in grads[0]
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
