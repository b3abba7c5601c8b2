"""GPU (-m gpu): the training step of a planner with largeGraphTraining='lists' (teams of more than graphML.MAX_NODES
agents: every graph-filter layer on graphML.lsigf_team_train, no dense N x N product) against the float64 statement of
the same step.  Case construction, statement, comparison and the Adam check are those of tests/test_gpu_training_f64.py,
imported unchanged; only the planner construction is new.  Also: the route itself (the team training calls ran, no
gnnpp_gemm_kmajor product with an N x N operand), the default / 'dense' setting bit-identical whatever largeGraphFilter
says, and GraphedTrainStep."""
import pytest
import torch

from test_gpu_training_f64 import Cfg, check_adam, check_against_f64, make_case, statement

pytestmark = pytest.mark.gpu

ADAM = (1e-3, 1e-5, None)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


def planner(dev, sd, N, K, L=1, E=1, training='lists', large_filter=None):
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    cfg = Cfg(N, K, dev, L, E)
    if training is not None:
        cfg.largeGraphTraining = training
    if large_filter is not None:
        cfg.largeGraphFilter = large_filter
    net = DecentralPlannerNet(cfg).to(dev)
    net.load_state_dict(sd)
    return net.train()


class Route:
    """Counts the team training calls and records every gnnpp_gemm_kmajor(_multi) product's (batch, M, N, K)."""

    def __init__(self, monkeypatch):
        from gnn_pathplanning_amd import _native, graphML as gml
        self.gml, self.before, self.gemms = gml, dict(gml.team_train_calls), []
        one, multi = _native.gemm_kmajor, _native.gemm_kmajor_multi
        monkeypatch.setattr(_native, 'gemm_kmajor', lambda *a: (self.gemms.append(tuple(a[-4:])), one(*a))[1])
        monkeypatch.setattr(_native, 'gemm_kmajor_multi',
                            lambda specs: (self.gemms.extend(tuple(s[-4:]) for s in specs), multi(specs))[1])

    def calls(self):
        return {k: v - self.before[k] for k, v in self.gml.team_train_calls.items()}

    def graph_products(self, Ns):
        """Products that contract over the graph's nodes with the graph's nodes as rows: S z or S^T z."""
        return [g for g in self.gemms if g[1] == Ns and g[3] == Ns]


def step(dev, monkeypatch, sd, obs, S, tgt, N, K, L, E, via_step, training='lists'):
    """tests/test_gpu_training_f64.py's _step with this file's planner; also the route's record."""
    from gnn_pathplanning_amd import decentralplanner as dp
    from gnn_pathplanning_amd import training as tr
    net = planner(dev, sd, N, K, L, E, training)
    seen, res = {}, {}
    orig, orig_loss = dp._EncoderTrainFunction.apply, tr._policy_loss_and_grad
    with monkeypatch.context() as mp:
        mp.setattr(dp._EncoderTrainFunction, 'apply', lambda *a: seen.setdefault('feat', orig(*a)))
        mp.setattr(tr, '_policy_loss_and_grad', lambda lg, t: (seen.setdefault('logits', lg), orig_loss(lg, t))[1])
        route = Route(mp)
        if via_step:
            opt = tr.FusedAdam(net.parameters(), lr=ADAM[0], weight_decay=ADAM[1])
            loss = tr.train_step(net, opt, obs.to(dev), tgt.to(dev), S.to(dev))
            res['params'] = {k: p.detach().cpu().clone() for k, p in net.named_parameters()}
            res['logits'] = seen['logits'].detach().permute(1, 0, 2).cpu()
        else:
            net.addGSO(S.to(dev))
            out = net(obs.to(dev))
            loss = tr.policy_loss(out, tgt.to(dev))
            loss.backward()
            res['logits'] = torch.stack(list(out), 1).detach().cpu()
        torch.cuda.synchronize()
    res['feat'] = seen['feat'].detach().cpu()
    res['loss'] = loss.detach().cpu()
    res['grads'] = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}
    res['running'] = {k: b.detach().cpu().clone() for k, b in net.named_buffers() if 'running' in k}
    res['nbt'] = {k: int(b) for k, b in net.named_buffers() if 'num_batches' in k}
    return res, route


def one_case(dev, monkeypatch, B, N, K=3, L=1, E=1, Ns=None, seed=0, fp64_gso=False, via=(True, False)):
    sd, obs, S, tgt = make_case(B, N, K, L, E, Ns, seed, fp64_gso=fp64_gso)
    w64 = statement(sd, S, obs, tgt, N, torch.float64)
    w32 = statement(sd, S, obs, tgt, N, torch.float32)
    for via_step in via:
        got, route = step(dev, monkeypatch, sd, obs, S, tgt, N, K, L, E, via_step)
        # the route: one saving forward and one input gradient per layer, one transpose per addGSO, and no product
        # over the dense graph -- what fails on a planner that trains on the dense form
        assert route.calls() == dict(transpose=1, fwd_save=L, input_grad=L), route.calls()
        assert not route.graph_products(Ns or N), route.graph_products(Ns or N)
        assert set(got['grads']) == set(w64['grads'])
        bad = check_against_f64(got, w64, w32, B, N)
        if via_step:
            bad += check_adam(sd, got, ADAM)
        assert not bad, '\n'.join(str(b) for b in bad)


@pytest.mark.parametrize('B,N,K,L,E,Ns,fp64_gso', [(2, 113, 3, 1, 1, None, False), (2, 130, 3, 1, 1, None, False),
                                                   (2, 100, 3, 2, 1, 120, False), (2, 130, 2, 1, 2, None, False),
                                                   (2, 130, 3, 1, 1, None, True)],
                         ids=['2x113', '2x130', '2x100on120/L2', '2x130/E2K2', '2x130/fp64gso'])
def test_team_training_step_against_float64(dev, monkeypatch, B, N, K, L, E, Ns, fp64_gso):
    """Through train_step() and through plain policy_loss(...).backward(): 113 agents (the first size past MAX_NODES), 130
    (Np = 132), 100 agents on a GSO of 120 nodes with two layers (every layer re-pads), E = 2 with K = 2, an fp64 GSO."""
    one_case(dev, monkeypatch, B, N, K, L, E, Ns, seed=B + 10 * N + 100 * K, fp64_gso=fp64_gso)


def test_team_training_step_1024_agents_against_float64(dev, monkeypatch):
    one_case(dev, monkeypatch, 1, 1024, seed=1024, via=(True,))


def test_dense_route_still_takes_dense_products(dev, monkeypatch):
    """The contrast of the route check: the default planner makes K - 1 forward and K - 1 adjoint products over the dense
    graph and none of the team training calls."""
    B, N, K = 2, 130, 3
    sd, obs, S, tgt = make_case(B, N, K, seed=77)
    _, route = step(dev, monkeypatch, sd, obs, S, tgt, N, K, 1, 1, True, training=None)
    assert route.calls() == dict(transpose=0, fwd_save=0, input_grad=0)
    assert len(route.graph_products(N)) == 2 * (K - 1)


def test_default_and_dense_training_are_bit_identical(dev, monkeypatch):
    """largeGraphTraining unset or 'dense' leaves every gradient as it was, under both settings of largeGraphFilter."""
    B, N, K = 2, 130, 3
    sd, obs, S, tgt = make_case(B, N, K, seed=78)
    grads = []
    for training, large_filter in ((None, None), ('dense', None), (None, 'lists'), ('dense', 'lists')):
        net = planner(dev, sd, N, K, training=training, large_filter=large_filter)
        net.addGSO(S.to(dev))
        net.forward_logits(obs.to(dev)).square().sum().backward()
        grads.append({k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    assert 'GFL.0.weight' in grads[0]
    for other in grads[1:]:
        assert other.keys() == grads[0].keys()
        for k in grads[0]:
            assert torch.equal(grads[0][k], other[k]), k


def test_forward_train_lists_equals_the_gso_route(dev):
    """forward_train_lists(obs, lists) gives the bytes of addGSO(S) + forward under largeGraphTraining='lists', with the
    transpose built inside, handed in, or promised away on a symmetric S."""
    from gnn_pathplanning_amd import graphML as gml
    B, N, K = 2, 130, 3
    sd, obs, S, tgt = make_case(B, N, K, seed=79)
    assert torch.equal(S, S.transpose(1, 2))                          # (D^-1/2 A D^-1/2 of a symmetric A)
    S, obs = S.to(dev), obs.to(dev)
    lists = gml.team_lists_from_dense(S.unsqueeze(1))
    out = []
    for kw in (None, {}, dict(lists_t=gml.team_lists_transpose(lists, B, N)), dict(symmetric=True)):
        net = planner(dev, sd, N, K)
        if kw is None:
            net.addGSO(S)
            logits = torch.stack(list(net(obs)), 0)
        else:
            logits = torch.stack(list(net.forward_train_lists(obs, lists, **kw)), 0)
        logits.square().sum().backward()
        out.append([logits.detach()] + [p.grad for p in net.parameters()])
    for other in out[1:]:
        assert len(other) == len(out[0]) and all(torch.equal(a, b) for a, b in zip(out[0], other))


def test_unserved_planners_raise(dev):
    """Layers wider than 128 features, more than 1024 nodes, split-f16: GnnppError naming largeGraphTraining='dense'."""
    from gnn_pathplanning_amd import _native
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    B, N = 1, 120
    obs = torch.zeros(B, N, 3, 11, 11, device=dev)
    S = torch.eye(N, device=dev).unsqueeze(0)
    for extra in (dict(dimNodeSignals=[160]), dict(precision='split_f16')):
        cfg = Cfg(N, 2, dev)
        cfg.largeGraphTraining = 'lists'
        for k, v in extra.items():
            setattr(cfg, k, v)
        net = DecentralPlannerNet(cfg).to(dev).train()
        net.addGSO(S)
        with pytest.raises(_native.GnnppError, match="largeGraphTraining='dense'"):
            net(obs)
    cfg = Cfg(N, 2, dev)
    cfg.largeGraphTraining = 'sparse'
    with pytest.raises(_native.GnnppError):
        DecentralPlannerNet(cfg)


def test_graphed_train_step_replays_the_eager_steps(dev):
    """GraphedTrainStep at 2 x 130: after its three eager warm-up steps, two replayed steps leave the parameter bytes of
    two eager steps.  The list build and the transpose are launches of the captured graph: the replayed steps' GSOs
    differ from the captured one's."""
    from gnn_pathplanning_amd import training as tr
    B, N, K = 2, 130, 3
    sd = make_case(B, N, K, seed=80)[0]
    batches = []
    for seed in (80, 81, 82):
        _, obs, S, tgt = make_case(B, N, K, seed=seed)
        batches.append((obs.to(dev), tgt.to(dev), S.to(dev)))
    results = []
    for graphed in (False, True):
        net = planner(dev, sd, N, K)
        opt = tr.FusedAdam(net.parameters(), lr=1e-3, weight_decay=1e-5)
        if graphed:
            run = tr.GraphedTrainStep(net, opt, *batches[0])          # (3 eager warm-up steps, then the capture)
            for b in batches[1:]:
                run(*b)
        else:
            for b in [batches[0]] * 3 + batches[1:]:
                tr.train_step(net, opt, *b)
        torch.cuda.synchronize()
        results.append({k: p.detach().clone() for k, p in net.named_parameters()})
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k
