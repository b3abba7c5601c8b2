"""GPU (-m gpu): training SEQUENCES -- eager steps, replays of a captured step, a partial batch, eval forwards, a rollout
step, checkpoint loads and `.data` edits mixed on one planner (tests/train_sequence_cases.py: scenarios, runner, oracles).

Every scenario is held, after every operation, to (a) its cache-free twin BIT FOR BIT and (b) the float64 statement of
that one operation from the device's own state, by f64_yardstick.gap; and wherever the last parameter update was one
step, the float64 statement at the parameters before it -- what a stale weight copy computes -- must sit
STALE_FACTOR x the allowance away, so that the comparison is known to notice one.

Every capture here runs GraphedTrainStep's default three warm-up steps; the scenarios that capture with warmup=0 are not
part of this file (see the commit that added it)."""
import pytest
import torch

import train_sequence_cases as tsc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', list(tsc.SCENARIOS))
def test_sequence_against_twin_and_float64(dev, name):
    c = tsc.SCENARIOS[name]
    _, _, batches = tsc.inputs(name)
    frozen = tsc.frozen_name if c['frozen'] else None
    fused = c['adam'] == 'fused'
    cached = tsc.run(name, dev, twin=False)
    twin = tsc.run(name, dev, twin=True)
    bad, ratios = [], {}
    last_update = None                                       # state before the last ONE-step parameter update
    for i, (r, t) in enumerate(zip(cached, twin)):
        op, arg, pre, got = r['op'], r['arg'], r['pre'], r['got']
        diff = tsc.first_bit_difference(r, t)                # oracle (a)
        if diff is not None:
            bad.append((i, op, 'differs from the cache-free twin in', diff))
        kind = 'train' if op in tsc.TRAINING_OPS else 'eval' if op == 'eval_forward' else None
        if op in tsc.TRAINING_OPS:                           # oracle (b)
            bad += [(i, op) + tuple(b) for b in tsc.check_training_op(pre, got, batches[arg], c['lr'], fused, frozen)]
        elif op == 'forward':
            bad += [(i, op) + tuple(b) for b in tsc.check_forward_op(pre, got, batches[arg])]
        elif op == 'eval_forward':
            bad += [(i, op) + tuple(b) for b in tsc.check_eval_op(pre, got['logits'], batches[arg])]
        if kind and last_update is not None:                 # would a one-step-stale copy have been noticed here?
            rr = tsc.stale_ratios(kind, pre['sd'], last_update, batches[arg], frozen)
            k = min(rr, key=rr.get)
            ratios[(i, op)] = (k, rr[k])
        if op in tsc.UPDATES:
            last_update = pre['sd']
        elif op == 'capture' and arg:
            last_update = None                               # several steps at once (the CPU trajectory has each of them)
    print(name, 'stale / allowed:', {k: '%s %.0fx' % v for k, v in ratios.items()})
    for b in bad:
        print(name, b)
    assert all(v[1] >= tsc.STALE_FACTOR for v in ratios.values()), ratios
    assert not bad, '\n'.join(str(b) for b in bad)


def test_eager_steps_pack_once_per_weight_version(dev):
    """The eager fast path stays: one pack per weight version (the cache's key moves with every optimizer step and is the
    key of the current weights afterwards), none when nothing changed."""
    from gnn_pathplanning_amd import _native
    from gnn_pathplanning_amd import training as tr
    name = '1_eager_eval_eager'
    sd, _, batches = tsc.inputs(name)
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    net = DecentralPlannerNet(tsc.Cfg(tsc.N, tsc.K, dev)).to(dev)
    net.load_state_dict(sd)
    net.train()
    opt = tr.FusedAdam(net.parameters(), lr=1e-3)
    obs, S, tgt = (t.to(dev) for t in batches[0])
    cache = net._train_pack_cache
    key_now = lambda: _native.PackCache.key_of([net.ConvLayers[i].weight for i in tsc.CONV] + [net.GFL[0].weight])  # noqa: E731
    net.addGSO(S)
    net(obs)
    buf = cache.buf
    assert cache.key == key_now()
    net(obs)
    assert cache.buf is buf and cache.key == key_now()       # nothing changed: no pack
    tr.train_step(net, opt, obs, tgt, S)                     # forward hits, the optimizer moves the weights
    assert cache.buf is buf and cache.key != key_now()
    net(obs)
    assert cache.buf is not buf and cache.key == key_now()   # one pack for the new version
    torch.cuda.synchronize()
