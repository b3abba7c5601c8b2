"""GPU (-m gpu): the training step with frozen parameters against the float64 statement of the same step, over the
(pattern, route) matrix of tests/train_freeze_cases.py (tests/test_train_freeze_cases.py shows on the CPU that the matrix
reaches every needs_input_grad signature and that every `direct` case sees a lost ReLU mask at > 1000 x the allowance).

Every case runs through training.train_step with FusedAdam(lr=1e-3, weight_decay=1e-5) and through
policy_loss(...).backward() without deferral, and is held
  * to the float64 statement by test_gpu_training_f64.check_against_f64 with its scales (freezing changes no value: the
    statement is the route's, computed once);
  * to the HIP run of the same route with NOTHING frozen, bit for bit, on every trainable gradient, the loss, the logits,
    the features and the running statistics: gemm_plan depends on a product's own shape alone and every reduction has a
    fixed order, so a product computes the same bits whichever launch carries it;
  * frozen tensors: `.grad is None`, bytes unchanged by the optimizer step (weight decay included), no exp_avg state;
  * the deferral queue: empty after every pass; under train_step the `direct` routes hand _native.defer_gemms one product
    per trainable tensor of the head and of EVERY filter layer (_forward_train sets fold bit 2 on each layer, so with
    L = 2 the first layer's taps and bias wait as well), the other routes none.
"""
import copy
import types

import pytest
import torch

import train_freeze_cases as fc
from f64_yardstick import gap
from test_gpu_training_f64 import check_adam, check_against_f64, make_case, statement

pytestmark = pytest.mark.gpu

ADAM = (1e-3, 1e-5, None)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


def run(dev, monkeypatch, r, pattern, via_step):
    """One HIP training step of route r with `pattern` frozen (None: nothing), through train_step or through
    policy_loss(...).backward(); everything the tests look at, on the CPU."""
    from gnn_pathplanning_amd import _native, decentralplanner as dp, training as tr
    sd, obs, S, tgt = fc.build(r)
    net = fc.planner(r, dev)
    if pattern is not None:
        fc.freeze(net, pattern)
    seen, queued, res = {}, [], {}
    orig, orig_loss, orig_defer = dp._EncoderTrainFunction.apply, tr._policy_loss_and_grad, _native.defer_gemms
    with monkeypatch.context() as mp:
        mp.setattr(dp._EncoderTrainFunction, 'apply', lambda *a: seen.setdefault('feat', orig(*a)))
        mp.setattr(tr, '_policy_loss_and_grad', lambda lg, t: (seen.setdefault('logits', lg), orig_loss(lg, t))[1])
        mp.setattr(_native, 'defer_gemms', lambda specs, prms: (queued.append(len(specs)), orig_defer(specs, prms))[1])
        if via_step:
            opt = tr.FusedAdam(net.parameters(), lr=ADAM[0], weight_decay=ADAM[1])
            loss = tr.train_step(net, opt, obs.to(dev), tgt.to(dev), S.to(dev))
            res['queue_after'] = len(_native._deferred_gemms)
            res['params'] = {k: p.detach().cpu().clone() for k, p in net.named_parameters()}
            res['logits'] = seen['logits'].detach().permute(1, 0, 2).cpu()
            res['moments'] = {k for k, p in net.named_parameters() if 'exp_avg' in opt.state.get(p, {})}
        else:
            net.addGSO(S.to(dev))
            out = net(obs.to(dev))
            loss = tr.policy_loss(out, tgt.to(dev))
            loss.backward()
            res['queue_after'] = len(_native._deferred_gemms)
            res['logits'] = torch.stack(list(out), 1).detach().cpu()
        torch.cuda.synchronize()
    res['queued'] = queued
    res['feat'] = seen['feat'].detach().cpu()
    res['loss'] = loss.detach().cpu()
    res['grads'] = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if p.grad is not None}
    res['running'] = {k: b.detach().cpu().clone() for k, b in net.named_buffers() if 'running' in k}
    res['nbt'] = {k: int(b) for k, b in net.named_buffers() if 'num_batches' in k}
    return res


_unfrozen = {}


def unfrozen(dev, monkeypatch, r, via_step):
    """The HIP run of the route with nothing frozen: once per (route, way of running), left unchanged."""
    if (r, via_step) not in _unfrozen:
        _unfrozen[(r, via_step)] = run(dev, monkeypatch, r, None, via_step)
    return _unfrozen[(r, via_step)]


@pytest.mark.parametrize('case', fc.MATRIX, ids=fc.case_id)
def test_frozen_training_step_against_float64(dev, monkeypatch, case):
    pattern, r = case
    c = fc.ROUTES[r]
    sd = fc.build(r)[0]
    w64, w32 = fc.statements(r)
    trainable = fc.trainable(case)
    for via_step in (True, False):
        got = run(dev, monkeypatch, r, pattern, via_step)
        ref = unfrozen(dev, monkeypatch, r, via_step)
        tag = 'train_step' if via_step else 'backward'
        # frozen tensors have no gradient, trainable ones all do
        assert list(got['grads']) == trainable, (tag, sorted(set(got['grads']) ^ set(trainable)))
        # the deferral queue
        assert got['queue_after'] == 0, tag
        assert sum(got['queued']) == (fc.deferred_products(case) if via_step else 0), (tag, got['queued'])
        # against float64
        bad = check_against_f64(got, w64, w32, c['B'], c['N'])
        if via_step:
            bad += check_adam(sd, got, ADAM)
        assert not bad, tag + '\n' + '\n'.join(str(b) for b in bad)
        # against the unfrozen HIP run: the same bits
        assert set(ref['grads']) == set(fc.param_names(r))
        for k in trainable:
            assert torch.equal(got['grads'][k], ref['grads'][k]), \
                (tag, k, (got['grads'][k].double() - ref['grads'][k].double()).abs().max().item())
        for k in ('loss', 'logits', 'feat'):
            assert torch.equal(got[k], ref[k]), (tag, k)
        for k, v in got['running'].items():
            assert torch.equal(v, ref['running'][k]), (tag, k)
        assert got['nbt'] == ref['nbt']
        # the optimizer: frozen bytes stay (weight decay moves no frozen tensor), no moments for them
        if via_step:
            assert got['moments'] == set(trainable)
            for k in fc.param_names(r):
                if k in trainable:
                    assert torch.equal(got['params'][k], ref['params'][k]), (k, 'the same gradient, the same update')
                    assert not torch.equal(got['params'][k], sd[k]), k
                else:
                    assert torch.equal(got['params'][k], sd[k]), k


def test_unfrozen_runs_defer_what_the_matrix_expects(dev, monkeypatch):
    """The contrast of the deferral counts: with everything trainable, 4 products on `direct`, 6 on `direct` with two
    layers, none elsewhere or outside train_step."""
    for r in fc.ROUTES:
        want = 2 + 2 * fc.ROUTES[r]['L'] if fc.route_name(r) == 'direct' else 0
        assert sum(unfrozen(dev, monkeypatch, r, True)['queued']) == want, r
        assert unfrozen(dev, monkeypatch, r, False)['queued'] == [], r


def test_gradient_sinks_hold_the_trainable_subset(dev):
    """FlatBucketDP built after freezing (world size 1): the bucket is the trainable tensors', every trainable gradient
    is born in it, no frozen tensor gets one."""
    from gnn_pathplanning_amd import training as tr
    r = 'direct'
    sd, obs, S, tgt = fc.build(r)
    net = fc.freeze(fc.planner(r, dev), 'transfer')
    dp = tr.FlatBucketDP(net)
    try:
        train = [p for p in net.parameters() if p.requires_grad]
        assert 0 < len(train) < len(list(net.parameters()))
        assert dp.bucket.numel() == sum(p.numel() for p in train) and len(dp.views) == len(train)
        opt = tr.FusedAdam(net.parameters(), lr=ADAM[0], weight_decay=ADAM[1])
        tr.train_step(net, opt, obs.to(dev), tgt.to(dev), S.to(dev), dp=dp)
        torch.cuda.synchronize()
        for p, v in zip(dp.params, dp.views):
            assert dp._in_bucket(p.grad, v)
        for k, p in net.named_parameters():
            assert (p.grad is None) == (not p.requires_grad), k
        # the bucket holds the gradients of the unfrozen statement
        w64, w32 = fc.statements(r)
        for (k, p), v in zip([(k, p) for k, p in net.named_parameters() if p.requires_grad], dp.views):
            ok, rep = gap(v.cpu(), w64['grads'][k], w32['grads'][k],
                          fc.grad_scale(k, w64['grads'], fc.ROUTES[r]['B'], fc.ROUTES[r]['N']))
            assert ok, (k, rep)
    finally:
        dp.close()


def test_graphed_transfer_step_replays_the_eager_steps(dev):
    """GraphedTrainStep on a planner frozen for transfer learning: after its three eager warm-up steps, two replays leave
    the parameter, running-statistics and num_batches_tracked bytes of two eager steps; frozen tensors keep theirs."""
    from gnn_pathplanning_amd import training as tr
    r = 'direct'
    c = fc.ROUTES[r]
    sd = fc.build(r)[0]
    batches = []
    for seed in (c['seed'], c['seed'] + 10, c['seed'] + 20):
        _, obs, S, tgt = make_case(c['B'], c['N'], c['K'], seed=seed, margin=False)
        batches.append((obs.to(dev), tgt.to(dev), S.to(dev)))
    results = []
    for graphed in (False, True):
        net = fc.freeze(fc.planner(r, dev), 'transfer')
        opt = tr.FusedAdam(net.parameters(), lr=ADAM[0], weight_decay=ADAM[1])
        if graphed:
            step = tr.GraphedTrainStep(net, opt, *batches[0])        # (3 eager warm-up steps, then the capture)
            for b in batches[1:]:
                step(*b)
        else:
            for b in [batches[0]] * 3 + batches[1:]:
                tr.train_step(net, opt, *b)
        torch.cuda.synchronize()
        results.append({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k
    frozen = fc._transfer()
    for k in fc.param_names(r):
        assert torch.equal(results[1][k], sd[k]) == (k in frozen), k
    for k in results[1]:
        if 'num_batches' in k:
            assert int(results[1][k]) == int(sd[k]) + 5 * c['N']


@pytest.mark.parametrize('r', list(fc.ROUTES))
def test_train_mode_forward_without_gradients(dev, r):
    """model.train() under torch.no_grad(), with every parameter frozen, and both: the logits and running statistics of the
    statement, the logits bit-identical to the grad-enabled forward's, nothing queued."""
    from gnn_pathplanning_amd import _native
    c = fc.ROUTES[r]
    sd, obs, S, tgt = fc.build(r)
    w64, w32 = fc.statements(r)
    outs = []
    for no_grad, frozen in ((False, False), (True, False), (False, True), (True, True)):
        net = fc.planner(r, dev)
        if frozen:
            for p in net.parameters():
                p.requires_grad_(False)
        net.addGSO(S.to(dev))
        with torch.set_grad_enabled(not no_grad):
            out = net(obs.to(dev))
        logits = torch.stack(list(out), 1)
        assert logits.requires_grad == (not no_grad and not frozen)
        torch.cuda.synchronize()
        assert not _native._deferred_gemms
        outs.append((logits.detach().cpu(), {k: b.detach().cpu().clone() for k, b in net.named_buffers()}))
    for logits, bufs in outs:
        ok, rep = gap(logits, w64['logits'], w32['logits'])
        assert ok, rep
        assert torch.equal(logits, outs[0][0])
        for k, b in bufs.items():
            assert torch.equal(b, outs[0][1][k]), k
            if 'running' in k:
                ok, rep = gap(b, w64['running'][k], w32['running'][k])
                assert ok, (k, rep)
            elif 'num_batches' in k:
                assert int(b) == w64['nbt'][k]


def test_checkpoint_loaded_for_transfer_learning(dev, monkeypatch, tmp_path):
    """formats.load_checkpoint(path, net, opt, train_TL=True) on a checkpoint of a fully trained step, then one train_step:
    the bytes of the `transfer` pattern started from that state (parameters, statistics, moments), the frozen tensors
    those of the checkpoint, the gradients and the Adam step held to float64 from that state."""
    from gnn_pathplanning_amd import formats, training as tr
    r = 'direct'
    c = fc.ROUTES[r]
    sd, obs, S, tgt = fc.build(r)
    batch = (obs.to(dev), tgt.to(dev), S.to(dev))
    net0 = fc.planner(r, dev)
    opt0 = tr.FusedAdam(net0.parameters(), lr=ADAM[0], weight_decay=ADAM[1])
    tr.train_step(net0, opt0, *batch)
    torch.cuda.synchronize()
    path = formats.save_checkpoint(str(tmp_path), net0, opt0, types.SimpleNamespace(state_dict=dict), 0, 1)
    sd1 = {k: v.detach().cpu().clone() for k, v in net0.state_dict().items()}
    # the checkpoint's moments, copied: Optimizer.load_state_dict adopts the tensors it is handed, so an optimizer loaded
    # from opt0.state_dict() would step opt0's own moments
    saved = {k: {m: opt0.state[p][m].cpu().clone() for m in ('exp_avg', 'exp_avg_sq')} for k, p in net0.named_parameters()}
    assert all(not torch.equal(sd1[k], sd[k]) for k in fc.param_names(r))

    def finish(net, opt):
        loss = tr.train_step(net, opt, *batch)
        torch.cuda.synchronize()
        return dict(loss=loss.cpu(), state={k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
                    grads={k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if p.grad is not None},
                    moments={k: opt.state[p]['exp_avg'].cpu().clone() for k, p in net.named_parameters()})
    net_a = fc.planner(r, dev)
    opt_a = tr.FusedAdam(net_a.parameters(), lr=ADAM[0], weight_decay=ADAM[1])
    assert formats.load_checkpoint(path, net_a, opt_a, train_TL=True) == (1, 1)
    a = finish(net_a, opt_a)
    net_b = fc.planner(r, dev, sd=sd1)
    opt_b = tr.FusedAdam(net_b.parameters(), lr=ADAM[0], weight_decay=ADAM[1])
    opt_b.load_state_dict(copy.deepcopy(opt0.state_dict()))
    fc.freeze(net_b, 'transfer')
    b = finish(net_b, opt_b)
    trainable = fc.trainable(('transfer', r))
    assert list(a['grads']) == list(b['grads']) == trainable
    assert torch.equal(a['loss'], b['loss'])
    for part in ('state', 'grads', 'moments'):
        for k in a[part]:
            assert torch.equal(a[part][k], b[part][k]), (part, k)
    for k in fc.param_names(r):
        assert torch.equal(a['state'][k], sd1[k]) == (k not in trainable), k
        if k not in trainable:                       # the loaded moments of a frozen tensor are not touched either
            assert torch.equal(a['moments'][k], saved[k]['exp_avg']), k
    # float64 from the checkpoint's state: the gradients, and Adam's second step on the loaded moments
    w64 = statement(sd1, S, obs, tgt, c['N'], torch.float64)
    w32 = statement(sd1, S, obs, tgt, c['N'], torch.float32)
    bad = []
    for k in trainable:
        ok, rep = gap(a['grads'][k], w64['grads'][k], w32['grads'][k], fc.grad_scale(k, w64['grads'], c['B'], c['N']))
        if not ok:
            bad.append((k, rep))
    state = types.SimpleNamespace(torch_state={k: dict(step=1, **saved[k]) for k in trainable})
    bad += check_adam(sd1, dict(grads=a['grads'], params=a['state']), (ADAM[0], ADAM[1], state))
    assert not bad, '\n'.join(str(x) for x in bad)
