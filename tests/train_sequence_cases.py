"""Training SEQUENCES: eager steps, replays of a captured step, a smaller last batch, eval forwards, rollout steps and
checkpoint loads mixed on one planner -- the scenarios, the runner and the two oracles.  Shared by
tests/test_train_sequence_cases.py (CPU: the float64 trajectories and the sensitivity condition) and
tests/test_gpu_training_sequences.py (the MI355X).  A plain helper module, not a conftest.

Between two calls the kernels do not read the parameters but copies of them (the one-launch train pack, the per-weight
tap packs, each filter layer's packed taps, the BN-folded inference encoder, the head's pointer table), keyed on version
counters, object ids and a generation counter.  A copy that is one step old gives a plausible loss and plausible
gradients; only a sequence can see it.

Oracle (a): the same scenario on a second planner with every copy thrown away before every operation
(_native.invalidate_packs) and every replay run as an eager step -- equal BIT FOR BIT on everything downloaded after
every operation (fixed reduction orders; packs are permutations and casts; a replay issues the eager step's launches).
Oracle (b): before each operation the planner's parameters, running statistics and optimizer moments come off the
device; the float64 statement of that ONE operation from that state (test_gpu_training_f64.statement + one Adam step,
policy_f64_cases.policy_statement) is held to the device's result by f64_yardstick.gap with the fp32 statement as the
yardstick.  Restarting from the device's state at every operation keeps Adam's normalisation from amplifying roundoff
across steps, so the one-step factors hold.
Sensitivity: for every operation behind a parameter update the float64 statement is also taken at the parameters BEFORE
that update -- what a one-step-stale copy computes -- and must sit STALE_FACTOR x the allowance of oracle (b) away from
the current one (logits and every gradient; `stale_ratios`).
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as tF

from f64_yardstick import MAX_K, RMS_K, ULP, ULPS, gap
from oracle import policy_oracle as orc
from policy_f64_cases import policy_statement
from test_gpu_training_f64 import (BN, CONV, Cfg, check_adam, check_against_f64, grad_scale, make_case, statement,
                                   without_pool_near_ties)

N, K, B_FULL, B_PART = 4, 3, 8, 3
STALE_FACTOR = 100.0
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8

# operations: (name, argument)
#   ('eager', b) ('replay', b)    one optimisation step on batch b, eagerly / as a replay of the captured step
#   ('capture', w)                GraphedTrainStep(..., warmup=w) on batch 0
#   ('forward', b)                a train-mode forward and loss on batch b, no backward, no optimizer step
#   ('eval_forward', b)           forward_logits on batch b (the planner must be in eval mode)
#   ('rollout_step', None)        one BatchedRollout.step(model) of 2 episodes (eval mode)
#   ('load', 'b')                 load_state_dict of the second state dict + the matching optimizer state
#   ('data_edit', s)              p.data += a fixed perturbation (seed s) of every parameter, then invalidate_packed()
#   ('train', None) ('eval', None)
_EVAL = [('eval', None), ('eval_forward', 4), ('train', None)]
_S3 = [('capture', 3), ('replay', 1), ('replay', 2), ('eager', 'p'), ('replay', 3), ('replay', 4), ('eval', None),
       ('eval_forward', 1)]
SCENARIOS = {
    # name: dict(ops, adam 'fused' | 'torch', L, precision, frozen encoder, lr).  lr: Adam's first steps move every weight
    # by about lr; at 1e-2 the planner of the eight-step scenarios is dead (all-zero gradients) by the last step, at
    # 2e-3 every stale statement still sits > 1e4 allowances away (tests/test_train_sequence_cases.py prints them).
    # Every scenario trains with the project's FusedAdam: torch.optim.Adam(capturable=True) forms 1 - beta2^t in fp32 on
    # the device, which at t < 10 costs ~1e-5 of a step -- 20..60 x the fp32 CPU yardstick on the bias vectors (measured
    # on scenario 3: max error 1.9e-8 against 4.4e-10) -- while staying bit-equal to its twin; adam='torch' and the
    # ('forward', b) operation are kept for the warmup=0 scenarios this file does not hold yet.
    '1_eager_eval_eager': dict(ops=[('eager', 0), ('eager', 1), ('eager', 2)] + _EVAL + [('eager', 3), ('eager', 4)]),
    '3_replays_partial_eager_replays': dict(ops=_S3),
    '4_capture_then_eager_calls': dict(ops=[('capture', 3), ('eval', None), ('eval_forward', 1), ('train', None),
                                            ('eager', 2)]),
    '5_load_between_replays': dict(ops=[('capture', 3), ('replay', 1), ('replay', 2), ('load', 'b'), ('replay', 3),
                                        ('replay', 4)]),
    '6_rollout_between_replays': dict(ops=[('capture', 3), ('replay', 1), ('eval', None), ('rollout_step', None),
                                           ('train', None), ('replay', 2)]),
    '8_scenario3_frozen_encoder': dict(ops=_S3, frozen=True),
    '10_data_edits': dict(ops=[('eager', 0), ('data_edit', 5), ('eager', 1), ('eval', None), ('eval_forward', 2),
                               ('data_edit', 6), ('eval_forward', 3)]),
}
for _i, (_k, _v) in enumerate(SCENARIOS.items()):
    _v.setdefault('adam', 'fused')
    _v.setdefault('L', 1)
    _v.setdefault('precision', None)
    _v.setdefault('frozen', False)
    _v.setdefault('lr', 2e-3)
    _v.setdefault('seed', 9100 + 10 * _i)

TRAINING_OPS = ('eager', 'replay')
UPDATES = ('eager', 'replay', 'load', 'data_edit')          # operations that move the parameters


def frozen_name(k):
    return k.startswith('ConvLayers.')


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(name):
    """(state dict, second state dict, {batch id: (obs, GSO, targets)}) of a scenario: five batches of B_FULL samples
    (ids 0..4) and the partial batch 'p' of B_PART; binary observations without max-pool near-ties at the initial
    parameters, GSOs from synth_gso_geometric."""
    c = SCENARIOS[name]
    sd = make_case(B_FULL, N, K, c['L'], seed=c['seed'], margin=False)[0]
    sd_b = make_case(B_FULL, N, K, c['L'], seed=c['seed'] + 5, margin=False)[0]
    g = torch.Generator().manual_seed(c['seed'] + 1)
    draw = lambda *shape: (torch.rand(*shape, generator=g) < 0.25).float()          # noqa: E731
    batches = {}
    for i, b in enumerate([0, 1, 2, 3, 4, 'p']):
        B = B_PART if b == 'p' else B_FULL
        obs = without_pool_near_ties(sd, draw(B, N, 3, 11, 11), draw)
        S = torch.from_numpy(orc.synth_gso_geometric(B, N, max(8, 2 * N), seed=c['seed'] + 2 + i)).float()
        tgt = tF.one_hot(torch.randint(0, 5, (B, N), generator=g), 5).float()
        batches[b] = (obs, S, tgt)
    return sd, sd_b, batches


def edit_of(sd, seed):
    """The perturbation ('data_edit', seed) adds to every parameter: 1e-2 x N(0, 1), the size of an Adam step."""
    g = torch.Generator().manual_seed(seed)
    return {k: 1e-2 * torch.randn(v.shape, generator=g) for k, v in sd.items()
            if v.dtype.is_floating_point and 'running' not in k}


def loaded_moments(sd, seed=77, t=7):
    """The optimizer state ('load', 'b') installs: moments of the size a run leaves, at step t."""
    g = torch.Generator().manual_seed(seed)
    return {k: {'step': t, 'exp_avg': 1e-3 * torch.randn(v.shape, generator=g),
                'exp_avg_sq': 1e-6 * torch.rand(v.shape, generator=g)}
            for k, v in sd.items() if v.dtype.is_floating_point and 'running' not in k}


def rollout_episodes():
    """2 episodes of N agents on a 12 x 12 map."""
    rng = np.random.default_rng(31)
    grids, starts, goals = [], [], []
    for _ in range(2):
        g = (rng.random((12, 12)) < 0.1).astype(np.uint8)
        free = np.argwhere(g == 0)
        idx = rng.choice(len(free), size=2 * N, replace=False)
        grids.append(g)
        starts.append(free[idx[:N]])
        goals.append(free[idx[N:]])
    return np.stack(grids), np.stack(starts), np.stack(goals)


# ---- oracle (b): the float64 statement of one operation ------------------------------------------------------------------
def adam_statement(params, grads, moments, lr, dt, f32_hyper):
    """One torch.optim.Adam step in dtype dt on `grads` from `params` and `moments` (name -> step / exp_avg /
    exp_avg_sq), as test_gpu_training_f64.check_adam states it.  f32_hyper: the hyperparameters rounded to fp32 (what
    gnnpp_adam_step is handed); torch's own device Adam takes them as doubles."""
    r = (lambda v: float(np.float32(v))) if f32_hyper else float
    names = list(grads)
    ps = [params[k].to(dt).clone().requires_grad_(True) for k in names]
    opt = torch.optim.Adam(ps, lr=r(lr), betas=(r(BETAS[0]), r(BETAS[1])), eps=r(ADAM_EPS), weight_decay=0.0)
    for k, p in zip(names, ps):
        st = moments[k]
        opt.state[p] = {'step': torch.tensor(float(st['step']), dtype=torch.float32),
                        'exp_avg': st['exp_avg'].to(dt).clone(), 'exp_avg_sq': st['exp_avg_sq'].to(dt).clone()}
        p.grad = grads[k].to(dt)
    opt.step()
    return {k: p.detach() for k, p in zip(names, ps)}


def allowance_ratio(x, w64, w32, scale=None):
    """min over (rms, max) of |x - w64| / what oracle (b) allows that tensor."""
    _, rep = gap(x, w64, w32, scale)
    floor = ULPS * ULP * rep['scale']
    if floor == 0.0 and rep['max32'] == 0.0:                 # an all-zero tensor: nothing is allowed, nothing can be asked
        return float('inf') if rep['max'] > 0.0 else 0.0
    return min(rep['rms'] / (RMS_K * rep['rms32'] + floor), rep['max'] / (MAX_K * rep['max32'] + floor))


def zero_gradient(k):
    """A conv bias in front of train-mode BatchNorm: its gradient is exactly zero at any parameters."""
    return k.startswith('ConvLayers.') and int(k.split('.')[1]) in CONV and k.endswith('.bias')


def stale_ratios(kind, cur, prev, batch, frozen=None):
    """{tensor: allowance_ratio} of the float64 statement at the state `prev` (before the last parameter update)
    against the one at `cur`, for a training operation ('train': logits and every gradient that is not identically
    zero) or an eval forward ('eval': logits)."""
    obs, S, tgt = batch
    B = obs.shape[0]
    if kind == 'eval':
        S4 = S.unsqueeze(1)
        w64, w32, old = (policy_statement(s, S4, obs, dt)[1] for s, dt in ((cur, torch.float64), (cur, torch.float32),
                                                                           (prev, torch.float64)))
        return {'logits': allowance_ratio(old, w64, w32)}
    w64, w32, old = (statement(s, S, obs, tgt, N, dt, frozen=frozen)
                     for s, dt in ((cur, torch.float64), (cur, torch.float32), (prev, torch.float64)))
    out = {'logits': allowance_ratio(old['logits'], w64['logits'], w32['logits'])}
    for k, g in w64['grads'].items():
        if not zero_gradient(k):
            out[k] = allowance_ratio(old['grads'][k], g, w32['grads'][k], grad_scale(k, w64['grads'], B, N))
    return out


def _with_buffers(got):
    """The record of an operation in the form check_against_f64 reads: running statistics and counters by name."""
    return dict(got, running={k: v for k, v in got['sd'].items() if 'running' in k},
                nbt={k: int(v) for k, v in got['sd'].items() if 'num_batches' in k})


def check_training_op(pre, got, batch, lr, fused, frozen=None):
    """Oracle (b) for one optimisation step: [] or the list of (tensor, report) beyond the yardstick."""
    obs, S, tgt = batch
    B = obs.shape[0]
    sd = pre['sd']
    w64 = statement(sd, S, obs, tgt, N, torch.float64, frozen=frozen)
    w32 = statement(sd, S, obs, tgt, N, torch.float32, frozen=frozen)
    assert set(got['grads']) == set(w64['grads']), (sorted(got['grads']), sorted(w64['grads']))
    bad = check_against_f64(_with_buffers(got), w64, w32, B, N)
    if fused:
        state = types.SimpleNamespace(torch_state=pre['moments'])
        bad += check_adam(sd, dict(got, params=got['sd']), (lr, 0.0, state))
    else:
        p64, p32 = (adam_statement(sd, got['grads'], pre['moments'], lr, dt, False)
                    for dt in (torch.float64, torch.float32))
        for k in got['grads']:
            ok, rep = gap(got['sd'][k], p64[k], p32[k])
            if not ok:
                bad.append(('adam ' + k, rep))
    for k, v in sd.items():                                  # a parameter without a gradient does not move
        if v.dtype.is_floating_point and 'running' not in k and k not in got['grads'] and not torch.equal(v, got['sd'][k]):
            bad.append(('frozen parameter moved', k))
    return bad


def check_forward_op(pre, got, batch, frozen=None):
    """Oracle (b) for a train-mode forward and loss without a backward pass."""
    obs, S, tgt = batch
    w64, w32 = (statement(pre['sd'], S, obs, tgt, N, dt, frozen=lambda k: True) for dt in (torch.float64, torch.float32))
    return check_against_f64(_with_buffers(dict(got, grads={})), w64, w32, obs.shape[0], N)


def check_eval_op(pre, logits, batch):
    """Oracle (b) for an eval-mode forward: logits [N,B,5] against policy_statement at the current state."""
    obs, S, _ = batch
    w64, w32 = (policy_statement(pre['sd'], S.unsqueeze(1), obs, dt)[1] for dt in (torch.float64, torch.float32))
    ok, rep = gap(logits, w64, w32)
    return [] if ok else [('eval logits', rep)]


# ---- the float64 trajectory (CPU): what the scenario's states are, without a device -------------------------------------
def f64_trajectory(name):
    """[(operation index, kind, state before the operation, state before the last update, batch)] for every training
    or eval operation of the scenario that follows a parameter update, with the states from float64 statements and
    float64 Adam steps -- the inputs of the sensitivity condition, on the CPU."""
    c = SCENARIOS[name]
    sd, sd_b, batches = inputs(name)
    frozen = frozen_name if c['frozen'] else None
    cur = {k: v.clone() for k, v in sd.items()}
    mom = None
    prev, out = None, []

    def step(b):
        nonlocal cur, mom, prev
        obs, S, tgt = batches[b]
        w = statement(cur, S, obs, tgt, N, torch.float64, frozen=frozen)
        if mom is None:
            mom = {k: {'step': 0, 'exp_avg': torch.zeros_like(cur[k]), 'exp_avg_sq': torch.zeros_like(cur[k])}
                   for k in w['grads']}
        new = adam_statement(cur, w['grads'], mom, c['lr'], torch.float64, False)
        for k, g in w['grads'].items():
            m = mom[k]
            m['exp_avg'] = 0.9 * m['exp_avg'].double() + 0.1 * g
            m['exp_avg_sq'] = 0.999 * m['exp_avg_sq'].double() + 0.001 * g * g
            m['step'] += 1
        prev = cur
        cur = dict(cur, **{k: v.float() for k, v in new.items()}, **{k: v.float() for k, v in w['running'].items()})

    for i, (op, arg) in enumerate(c['ops']):
        if op in TRAINING_OPS or op == 'eval_forward':
            if prev is not None:
                out.append((i, 'eval' if op == 'eval_forward' else 'train', cur, prev, batches[arg]))
        if op in TRAINING_OPS:
            step(arg)
        elif op == 'capture':
            for _ in range(arg):
                step(0)
        elif op == 'load':
            prev, cur = cur, {k: v.clone() for k, v in sd_b.items()}
            mom = {k: dict(v) for k, v in loaded_moments(sd_b).items() if not (frozen and frozen(k))}
        elif op == 'data_edit':
            prev, cur = cur, dict(cur, **{k: cur[k] + d for k, d in edit_of(sd, arg).items()})
    return out


# ---- the runner (device) --------------------------------------------------------------------------------------------------
class _Taps:
    """Keeps the encoder features and the logits of the last train-mode forward reachable (for a captured step: the
    graph's own tensors, which every replay rewrites -- held here so that the capture cannot reuse their memory)."""

    def __init__(self):
        self.feat = self.logits = None

    def __enter__(self):
        from gnn_pathplanning_amd import decentralplanner as dp
        from gnn_pathplanning_amd import training
        self._mods = (dp, training)
        self._orig = (dp._EncoderTrainFunction.apply, training._policy_loss_and_grad)
        assert 'apply' not in dp._EncoderTrainFunction.__dict__
        enc, loss = self._orig

        def enc_tap(*a):
            self.feat = enc(*a)
            return self.feat

        def loss_tap(lg, t):
            self.logits = lg
            return loss(lg, t)
        dp._EncoderTrainFunction.apply = enc_tap
        training._policy_loss_and_grad = loss_tap
        return self

    def __exit__(self, *exc):
        dp, training = self._mods
        del dp._EncoderTrainFunction.apply                   # (the inherited classmethod again)
        training._policy_loss_and_grad = self._orig[1]
        return False


def _moments(net, opt, fused):
    out = {}
    ctr = opt.state.get('gnnpp_group_0', {}).get('counter') if fused else None
    for k, p in net.named_parameters():
        if not p.requires_grad:
            continue
        st = opt.state.get(p) or {}
        step = (float(ctr[0]) if ctr is not None else 0.0) if fused else float(st['step']) if 'step' in st else 0.0
        out[k] = {'step': step,
                  'exp_avg': st['exp_avg'].detach().cpu().clone() if 'exp_avg' in st else torch.zeros(p.shape),
                  'exp_avg_sq': st['exp_avg_sq'].detach().cpu().clone() if 'exp_avg_sq' in st else torch.zeros(p.shape)}
    return out


def _state(net, opt, fused):
    torch.cuda.synchronize()
    return dict(sd={k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, moments=_moments(net, opt, fused))


def run(name, dev, twin):
    """The scenario on the device; returns one record per operation: {'pre': state before it, 'got': what it produced
    (always 'sd': parameters, running statistics and counters afterwards)}.  twin: every cached copy is thrown away
    before every operation, a replay is the same step run eagerly, a capture is its warm-up steps alone."""
    from gnn_pathplanning_amd import _native
    from gnn_pathplanning_amd import training as tr
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from gnn_pathplanning_amd.rollout import BatchedRollout
    c = SCENARIOS[name]
    sd, sd_b, batches = inputs(name)
    fused = c['adam'] == 'fused'
    cfg = Cfg(N, K, dev, c['L'])
    if c['precision']:
        cfg.precision = c['precision']
    net = DecentralPlannerNet(cfg).to(dev)
    if c['precision']:
        for l in range(c['L']):
            net.GFL[2 * l].precision = c['precision']
    net.load_state_dict(sd)
    net.train()
    if c['frozen']:
        net.ConvLayers.requires_grad_(False)
    ps = [p for p in net.parameters() if p.requires_grad]
    opt = tr.FusedAdam(ps, lr=c['lr']) if fused else torch.optim.Adam(ps, lr=c['lr'], capturable=True)
    dbatch = {b: tuple(t.to(dev) for t in v) for b, v in batches.items()}
    step = graph_taps = graph_grads = env = None
    records = []

    def trained(taps, loss, grads):
        torch.cuda.synchronize()
        return dict(loss=loss.detach().cpu().clone(), logits=taps.logits.detach().permute(1, 0, 2).cpu().clone(),
                    feat=taps.feat.detach().cpu().clone(), grads={k: g.detach().cpu().clone() for k, g in grads.items()})

    for op, arg in c['ops']:
        if twin:
            _native.invalidate_packs()
        pre = _state(net, opt, fused)
        got = {}
        if op == 'eager' or (op == 'replay' and twin):
            obs, S, tgt = dbatch[arg]
            with _Taps() as taps:
                loss = tr.train_step(net, opt, obs, tgt, S)
            got = trained(taps, loss, {k: p.grad for k, p in net.named_parameters() if p.grad is not None})
        elif op == 'replay':
            obs, S, tgt = dbatch[arg]
            loss = step(obs, tgt, S)
            got = trained(graph_taps, loss, graph_grads)
        elif op == 'capture':
            obs, S, tgt = dbatch[0]
            if twin:
                for _ in range(arg):
                    tr.train_step(net, opt, obs, tgt, S)
            else:
                with _Taps() as graph_taps:
                    step = tr.GraphedTrainStep(net, opt, obs, tgt, S, warmup=arg)
                # the captured step's own gradient tensors: `p.grad` is replaced by the next eager step
                graph_grads = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
        elif op == 'forward':
            obs, S, tgt = dbatch[arg]
            with _Taps() as taps:
                net.addGSO(S)
                out = net(obs)
                loss = tr.policy_loss_fused(out, tgt)
            torch.cuda.synchronize()
            got = dict(loss=loss.detach().cpu().clone(), logits=out.stacked.detach().permute(1, 0, 2).cpu().clone(),
                       feat=taps.feat.detach().cpu().clone())
            del out, loss
        elif op == 'eval_forward':
            obs, S, _ = dbatch[arg]
            net.addGSO(S)
            with torch.no_grad():
                got = dict(logits=net.forward_logits(obs).detach().cpu().clone())
        elif op == 'rollout_step':
            if env is None:
                env = BatchedRollout(*rollout_episodes(), 20, dev, tie_mode='lowest')
            env.step(net)
            torch.cuda.synchronize()
            lg = env._logits
            got = dict(logits=lg.detach().cpu().clone(), actions=net.decode_actions(lg).cpu().clone(),
                       pos=env.pos.detach().cpu().clone())
        elif op == 'load':
            net.load_state_dict(sd_b)
            osd = opt.state_dict()
            names = [k for k, p in net.named_parameters() if p.requires_grad]
            mom = loaded_moments(sd_b)
            for i, k in enumerate(names):
                e = {'exp_avg': mom[k]['exp_avg'].to(dev), 'exp_avg_sq': mom[k]['exp_avg_sq'].to(dev)}
                if not fused:
                    e['step'] = torch.tensor(float(mom[k]['step']), device=dev)
                osd['state'][i] = e
            if fused:
                ctr = torch.zeros(8)
                ctr[0] = float(mom[names[0]]['step'])
                osd['state']['gnnpp_group_0'] = {'counter': ctr.to(dev)}
            if step is not None:
                step.load_optimizer_state(osd)               # (into the tensors the graph reads)
            else:
                opt.load_state_dict(osd)
        elif op == 'data_edit':
            for k, p in net.named_parameters():
                p.data.add_(edit_of(sd, arg)[k].to(dev))
            net.invalidate_packed()
        elif op == 'train':
            net.train()
        elif op == 'eval':
            net.eval()
        else:
            raise ValueError(op)
        got['sd'] = _state(net, opt, fused)['sd']
        got['moments'] = _moments(net, opt, fused)
        records.append(dict(op=op, arg=arg, pre=pre, got=got))
    return records


def flatten(rec):
    """{name: tensor} of everything a record's operation produced."""
    out = {}
    for k, v in rec['got'].items():
        if isinstance(v, dict):
            for k2, v2 in v.items():
                if isinstance(v2, dict):
                    out.update({'%s.%s.%s' % (k, k2, k3): torch.as_tensor(v3) for k3, v3 in v2.items()})
                else:
                    out['%s.%s' % (k, k2)] = torch.as_tensor(v2)
        else:
            out[k] = v
    return out


def first_bit_difference(a, b):
    """None, or the name of the first tensor of two records that differs in any bit."""
    fa, fb = flatten(a), flatten(b)
    if list(fa) != list(fb):
        return 'tensor sets: %s' % sorted(set(fa) ^ set(fb))
    for k in fa:
        x, y = fa[k].contiguous().numpy(), fb[k].contiguous().numpy()
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            return k
    return None
