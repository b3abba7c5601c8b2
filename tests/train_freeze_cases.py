"""The training step with FROZEN parameters (formats.freeze_for_transfer_learning and every other requires_grad pattern a
fine-tuning run may set): the freeze patterns, the routes DecentralPlannerNet._forward_train takes, the case matrix, and
the float64 statement of a frozen step.  Shared by tests/test_train_freeze_cases.py (CPU: coverage of the
needs_input_grad signatures, the statement, the sensitivity guard) and tests/test_gpu_training_frozen_f64.py (the
MI355X).  A plain helper module, not a conftest.

What the matrix is for: the backward pass is a chain of contracts between neighbouring autograd Functions (who masks a
ReLU's gradient, whose parameter-gradient products wait for whose launch), each decided by the route alone, while every
Function builds its list of products from ctx.needs_input_grad.  A pattern is a predicate frozen(name) on parameter
names; a case is a (pattern, route) pair.

The issue's ten patterns leave six needs_input_grad signatures unreached (an input that needs no gradient next to a
single trainable parameter); `SIGNATURE_PATTERNS` adds the six patterns that reach them.
"""
import functools

import torch
import torch.nn.functional as tF

from test_gpu_training_f64 import BN, CONV, Cfg, grad_scale, make_case, statement
from f64_yardstick import MAX_K, RMS_K, ULP, ULPS, gap

MAX_NODES = 112                       # restated from graphML (tests/test_planner_routes.py holds it to the package's value)

_BIASES = ('compressMLP.0.bias', 'actionsMLP.0.bias')
_WEIGHTS = ('compressMLP.0.weight', 'actionsMLP.0.weight')


def _is_bias(k):
    return k in _BIASES or (k.startswith('GFL.') and k.endswith('.bias'))


def _is_taps(k):
    return k in _WEIGHTS or (k.startswith('GFL.') and k.endswith('.weight'))


def _bn_affine(k):
    return k.startswith('ConvLayers.') and int(k.split('.')[1]) in BN


def _transfer_frozen():
    """The names formats.freeze_for_transfer_learning itself freezes, read off a planner it was applied to (the name set
    is the same for every L: GFL.* and actionsMLP.* stay trainable)."""
    from gnn_pathplanning_amd import formats
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    net = DecentralPlannerNet(Cfg(2, [2, 2], 'cpu', L=2))
    formats.freeze_for_transfer_learning(net)
    frozen = frozenset(k for k, p in net.named_parameters() if not p.requires_grad)
    assert frozen and any(p.requires_grad for p in net.parameters())
    return frozen


@functools.lru_cache(maxsize=None)
def _transfer():
    return _transfer_frozen()


def _in_transfer(k):
    return k in _transfer()


# name -> frozen(parameter name)
ISSUE_PATTERNS = {
    'transfer': _in_transfer,
    'head_only': lambda k: not k.startswith('actionsMLP.'),
    'head_frozen': lambda k: k.startswith('actionsMLP.'),
    'filter_frozen': lambda k: k.startswith('GFL.'),
    'compress_frozen': lambda k: k.startswith('compressMLP.'),
    'encoder_frozen': lambda k: k.startswith('ConvLayers.'),
    'biases_frozen': _is_bias,
    'taps_frozen': _is_taps,
    'bn_affine_frozen': _bn_affine,
    'first_filter_frozen': lambda k: k.startswith('GFL.0.'),             # L = 2 only
}
SIGNATURE_PATTERNS = {
    # one trainable parameter next to an input that needs no gradient: the signatures (F,T,F) / (F,F,T) of the two Linear
    # Functions and (T,F,F) / (F,F,T) of the filter Function
    'transfer_biases_frozen': lambda k: _in_transfer(k) or _is_bias(k),
    'transfer_taps_frozen': lambda k: _in_transfer(k) or _is_taps(k),
    'head_weight_only': lambda k: k != 'actionsMLP.0.weight',
    'head_bias_only': lambda k: k != 'actionsMLP.0.bias',
    'encoder_biases_frozen': lambda k: k.startswith('ConvLayers.') or _is_bias(k),
    'encoder_taps_frozen': lambda k: k.startswith('ConvLayers.') or _is_taps(k),
}
PATTERNS = dict(ISSUE_PATTERNS, **SIGNATURE_PATTERNS)

# name -> the smallest shape the existing training tests use for that route of _forward_train
ROUTES = {
    'direct': dict(B=8, N=4, K=3, L=1, E=1, Ns=None, widths=None, seed=8403),
    'direct_L2': dict(B=4, N=6, K=[2, 3], L=2, E=2, Ns=None, widths=[64, 48], seed=4602),
    'padded_L2': dict(B=4, N=5, K=3, L=2, E=1, Ns=8, widths=None, seed=4503),
    'dense': dict(B=2, N=113, K=3, L=1, E=1, Ns=None, widths=None, seed=21133, training='dense'),
    'lists': dict(B=2, N=113, K=3, L=1, E=1, Ns=None, widths=None, seed=21134, training='lists', precision='fp32'),
    'lists_mfma_E2': dict(B=2, N=113, K=2, L=1, E=2, Ns=None, widths=None, seed=21135, training='lists',
                          precision='fp32_mfma'),
}
DIRECT = ('direct', 'direct_L2')
SMALL = ('direct', 'direct_L2', 'padded_L2')
# on every route but the first: the four the issue names and the three that complete the filter Function's signatures
ELSEWHERE = ('transfer', 'filter_frozen', 'head_frozen', 'biases_frozen', 'taps_frozen', 'transfer_biases_frozen',
             'transfer_taps_frozen')


def _matrix():
    m = [(p, 'direct') for p in PATTERNS if p != 'first_filter_frozen']
    for r in ROUTES:
        if r != 'direct':
            m += [(p, r) for p in ELSEWHERE]
            if ROUTES[r]['L'] == 2:
                m.append(('first_filter_frozen', r))
    return tuple(m)


MATRIX = _matrix()


def case_id(case):
    return '%s-%s' % case


def route_name(r):
    """The branch of _forward_train the route's shape takes, restated."""
    c = ROUTES[r]
    Ns = c['Ns'] or c['N']
    if Ns > MAX_NODES:
        return 'lists' if c.get('training') == 'lists' else 'dense'
    return 'direct' if Ns == c['N'] else 'padded'


def param_names(r):
    L = ROUTES[r]['L']
    names = []
    for ci, bi in zip(CONV, BN):
        names += ['ConvLayers.%d.weight' % ci, 'ConvLayers.%d.bias' % ci, 'ConvLayers.%d.weight' % bi,
                  'ConvLayers.%d.bias' % bi]
    names += ['compressMLP.0.weight', 'compressMLP.0.bias']
    for l in range(L):
        names += ['GFL.%d.weight' % (2 * l), 'GFL.%d.bias' % (2 * l)]
    return names + ['actionsMLP.0.weight', 'actionsMLP.0.bias']


def trainable(case):
    p, r = case
    return [k for k in param_names(r) if not PATTERNS[p](k)]


def signatures(case):
    """needs_input_grad of every autograd Function of the step, from the predicate and the chain rule alone: an
    activation needs a gradient when any parameter below it is trainable (the observations never do).
      'encoder'  (conv w, conv b, bn w, bn b) x 5            'compress', 'head'  (x, W, b)
      'GFL.<2l>' (h, x, b) -- the S / flag inputs of the filter Functions never need one."""
    p, r = case
    t = lambda k: not PATTERNS[p](k)                                     # noqa: E731
    names = param_names(r)
    sig = {'encoder': tuple(t(k) for k in names[:20])}
    below = any(sig['encoder'])
    sig['compress'] = (below, t('compressMLP.0.weight'), t('compressMLP.0.bias'))
    below = any(sig['compress'])
    for l in range(ROUTES[r]['L']):
        sig['GFL.%d' % (2 * l)] = (t('GFL.%d.weight' % (2 * l)), below, t('GFL.%d.bias' % (2 * l)))
        below = any(sig['GFL.%d' % (2 * l)])
    sig['head'] = (below, t('actionsMLP.0.weight'), t('actionsMLP.0.bias'))
    return sig


def deferred_products(case):
    """Products _native.defer_gemms is handed under train_step: on the `direct` route the head (defer = 1) and EVERY
    filter layer (fold bit 2 is set on each of them, not on the last alone) queue the products of their trainable
    parameters for the compress layer's launch; no other route defers."""
    if route_name(case[1]) != 'direct':
        return 0
    return sum(1 for k in trainable(case) if k.startswith(('GFL.', 'actionsMLP.')))


# ---- inputs and statements ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build(r):
    """(state_dict, observations, GSO, targets) of a route: test_gpu_training_f64.make_case in the plain regime
    (margin=False: the ReLU masks are non-trivial)."""
    c = ROUTES[r]
    return make_case(c['B'], c['N'], c['K'], c['L'], c['E'], c['Ns'], c['seed'], margin=False, widths=c['widths'])


@functools.lru_cache(maxsize=None)
def statements(r):
    """(float64, fp32) statements of the route's step with NOTHING frozen.  Freezing changes no value (the CPU tests hold
    the frozen statement's gradients to these bit for bit), so every pattern of the route is held to this pair."""
    sd, obs, S, tgt = build(r)
    N = ROUTES[r]['N']
    return statement(sd, S, obs, tgt, N, torch.float64), statement(sd, S, obs, tgt, N, torch.float32)


def frozen_statement(case, dtype=torch.float64, relu=None):
    p, r = case
    sd, obs, S, tgt = build(r)
    return statement(sd, S, obs, tgt, ROUTES[r]['N'], dtype, frozen=PATTERNS[p], relu=relu)


def planner(r, dev, sd=None):
    """The route's planner in train mode (nothing frozen yet)."""
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    c = ROUTES[r]
    cfg = Cfg(c['N'], c['K'], dev, c['L'], c['E'], c['widths'])
    if c.get('training'):
        cfg.largeGraphTraining = c['training']
    if c.get('precision'):
        cfg.precision = c['precision']
    net = DecentralPlannerNet(cfg).to(dev)
    if c.get('precision'):                       # the arithmetic of each layer's forward contraction is the layer's own
        for l in range(c['L']):
            net.GFL[2 * l].precision = c['precision']
    net.load_state_dict(build(r)[0] if sd is None else sd)
    return net.train()


def freeze(net, pattern):
    """requires_grad of every parameter by the pattern; `transfer` by the package's own function."""
    if pattern == 'transfer':
        from gnn_pathplanning_amd import formats
        formats.freeze_for_transfer_learning(net)
    else:
        for k, p in net.named_parameters():
            p.requires_grad_(not PATTERNS[pattern](k))
    return net


# ---- the mask regime and the lost-mask guard ----------------------------------------------------------------------------
def mask_names(r):
    return ['compress'] + ['GFL.%d' % (2 * l) for l in range(ROUTES[r]['L'])]


@functools.lru_cache(maxsize=None)
def non_positive_shares(r):
    """Share of non-positive pre-activations at the compress output and at each filter output, in float64."""
    seen = {}

    def relu(name, pre):
        seen.setdefault(name, []).append(pre.detach())
        return tF.relu(pre)
    sd, obs, S, tgt = build(r)
    statement(sd, S, obs, tgt, ROUTES[r]['N'], torch.float64, frozen=lambda k: True, relu=relu)
    return {k: float(torch.cat([t.flatten() for t in v]).le(0).double().mean()) for k, v in seen.items()}


def relu_without_backward_mask(which):
    """relu(name, pre) that lets the whole gradient through at layer `which` (forward values unchanged): the statement of
    a backward pass that lost that layer's ReLU mask -- a fold promised by one Function and not kept by its neighbour."""
    def relu(name, pre):
        y = tF.relu(pre)
        return pre + (y - pre).detach() if name == which else y
    return relu


def below_mask(r, which):
    """Parameters whose gradient passes through the ReLU of layer `which` ('compress' | 'GFL.<2l>')."""
    names = param_names(r)
    if which == 'compress':
        return names[:22]
    return names[:22 + 2 * (int(which.split('.')[1]) // 2 + 1)]


def lost_mask_excess(case, which):
    """{trainable tensor below the mask: min over (rms, max) of difference / allowance} for the float64 statement with
    the mask of `which` dropped against the true one; the allowance is f64_yardstick's for the route's fp32 statement."""
    p, r = case
    c = ROUTES[r]
    w64, w32 = statements(r)
    wrong = frozen_statement(case, relu=relu_without_backward_mask(which))['grads']
    out = {}
    for k in below_mask(r, which):
        if k not in wrong:
            continue
        _, rep = gap(wrong[k], w64['grads'][k], w32['grads'][k], grad_scale(k, w64['grads'], c['B'], c['N']))
        floor = ULPS * ULP * rep['scale']
        out[k] = min(rep['rms'] / (RMS_K * rep['rms32'] + floor), rep['max'] / (MAX_K * rep['max32'] + floor))
    return out
