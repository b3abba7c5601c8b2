"""Planners with several graph-filter layers on a GSO with more nodes than the team: the routes DecentralPlannerNet
takes, restated, and the case matrix that reaches each of them.  Shared by tests/test_planner_routes.py (CPU: route
coverage and the sensitivity guard) and tests/test_gpu_planner_routes_f64.py (the MI355X).  A plain helper module, not a
conftest.

What the matrix is for: the reference's GraphFilterBatch.forward zero-pads its input to the GSO's node count, filters,
and cuts the output back to the team's nodes (utils/graphUtils/graphML.py:2464-2476) -- EVERY layer does, so with
L >= 2 layers the extra nodes carry zeros into every layer, not only the first.  A route that pads once hands layer l's
bias + ReLU output on the extra nodes to layer l + 1.  The float64 statement (policy_f64_cases.filter_stack) re-pads per
layer; `policy_statement_padded_once` is the statement of the defect, used only to show that every case would expose it
(the guard of tests/test_planner_routes.py).

A case is a dict: N agents, Ns GSO nodes, taps per layer, widths (output features per layer), E edge features, B
samples, f64 (an fp64 GSO), obs (the kind of pc.make_obs).
"""
import functools
import math

import torch
import torch.nn.functional as tF

import policy_f64_cases as pc

# restated from gnn_pathplanning_amd/graphML.py (tests/test_planner_routes.py holds them to the package's values)
MAX_NODES = 112                       # rows one workgroup holds in LDS
TEAM_MAX_NODES = 1024                 # nodes the neighbour-list (team) kernels serve
FEATURES = 128                        # the encoder's output width: the first filter layer's input

EVAL_ROUTES = ('policy_fwd', 'small_general', 'small_general+gemm_head', 'dense', 'lists', 'lists_one_call')
TRAIN_ROUTES = ('train_direct', 'train_padded', 'train_dense')
PRECISIONS = ('fp32', 'fp32_mfma', 'split_f16')


def route(training, N, Ns, L, E, widths, precision='fp32', largeGraphFilter='dense'):
    """The route DecentralPlannerNet._forward_eval / _forward_train takes (decentralplanner.py), by name:
      policy_fwd               one gnnpp_policy_fwd call: one layer of 128 features, Ns == N <= MAX_NODES
      small_general            encoder, gnnpp_lsigf_fwd per inner layer, gnnpp_filter_head_fwd (Ns <= MAX_NODES)
      small_general+gemm_head  the same with a last layer wider than 128: gnnpp_lsigf_fwd for it, the head as a GEMM
      dense                    Ns > MAX_NODES: encoder, graphML._lsigf_large per layer ('dense', and split_f16 always)
      lists / lists_one_call   Ns > MAX_NODES under largeGraphFilter='lists': the team kernels per layer / the one
                               gnnpp_policy_team_fwd call (one layer of 128 features, Ns == N)
      train_direct             train mode, Ns == N <= MAX_NODES: the LDS-resident kernels with the fused ReLU folds
      train_padded             train mode, N < Ns <= MAX_NODES: the LDS-resident kernels on the zero-padded signal
      train_dense              train mode, Ns > MAX_NODES: graphML._LSIGFFunction's dense form
    E does not change the route (E > 1 only keeps gnnpp_policy_fwd off its fused kernel)."""
    assert Ns >= N and L == len(widths) and E >= 1 and precision in PRECISIONS
    assert largeGraphFilter in ('dense', 'lists')
    one_call = L == 1 and Ns == N and widths[-1] == FEATURES
    if training:
        if Ns > MAX_NODES:
            return 'train_dense'
        return 'train_direct' if Ns == N else 'train_padded'
    if Ns > MAX_NODES:
        if largeGraphFilter == 'lists' and precision != 'split_f16':
            return 'lists_one_call' if one_call else 'lists'
        return 'dense'
    if one_call:
        return 'policy_fwd'
    return 'small_general+gemm_head' if widths[-1] > FEATURES else 'small_general'


def _case(N, Ns, taps, widths, E=1, B=3, f64=False, obs='real'):
    return dict(N=N, Ns=Ns, taps=tuple(taps), widths=tuple(widths), E=E, B=B, f64=f64, obs=obs)


CASES = (
    # several layers on a GSO larger than the team: every route that has to pad again per layer
    _case(6, 9, [3, 3], [128, 128]),
    _case(6, 9, [3, 3], [128, 128], f64=True, obs='binary'),
    _case(50, 64, [2, 3, 2], [64, 48, 128], E=2, B=2),
    _case(20, 28, [2, 2], [128, 160]),
    _case(100, 120, [3, 2], [128, 128], B=2),            # the team fits one workgroup, the GSO does not
    _case(100, 120, [3, 2], [128, 128], B=2, f64=True, obs='binary'),
    _case(130, 150, [2, 3], [64, 48], E=2, B=2),
    # controls: nothing to pad again
    _case(6, 6, [3, 3], [128, 128]),
    _case(6, 9, [3], [128]),
    # the one-call routes (N = 20: beyond the fused kernel's 16 agents, so the feature workspace is written)
    _case(20, 20, [3], [128]),
    _case(130, 130, [3], [128], B=2),
)


def case_id(c):
    return 'N%d_Ns%d_K%s_F%s_E%d%s' % (c['N'], c['Ns'], 'x'.join(map(str, c['taps'])),
                                       'x'.join(map(str, c['widths'])), c['E'], '_S64' if c['f64'] else '')


def case_seed(c):
    return 7000 + CASES.index(c)


def needs_repadding(c):
    return c['Ns'] > c['N'] and len(c['taps']) >= 2


def case_routes(c, training):
    """The routes the case reaches over the precisions and the largeGraphFilter values it runs under."""
    args = (c['N'], c['Ns'], len(c['taps']), c['E'], c['widths'])
    if training:
        return {route(True, *args)}
    lgfs = ('dense', 'lists') if c['Ns'] > MAX_NODES else ('dense',)
    return {route(False, *args, precision=p, largeGraphFilter=g) for p in PRECISIONS for g in lgfs}


@functools.lru_cache(maxsize=None)
def _build(ci, seed):
    c = CASES[ci]
    B, N, Ns, E = c['B'], c['N'], c['Ns'], c['E']
    obs1 = pc.make_obs(seed, B * N, c['obs'])
    sd = dict(pc.make_net(seed, obs1, K=c['taps'][0], E=E))
    g = torch.Generator().manual_seed(seed + 13)
    F = (FEATURES,) + c['widths']
    for l, K in enumerate(c['taps']):
        # the reference's rule (graphML.py:2442-2447): weight and bias uniform in +- 1 / sqrt(G K); the bias is NOT
        # zero, so relu(bias) is what a route that pads once carries on the extra nodes
        stdv = 1.0 / math.sqrt(F[l] * K)
        sd['GFL.%d.weight' % (2 * l)] = (torch.rand(F[l + 1], E, K, F[l], generator=g) * 2 - 1) * stdv
        sd['GFL.%d.bias' % (2 * l)] = (torch.rand(F[l + 1], 1, generator=g) * 2 - 1) * stdv
        assert (sd['GFL.%d.bias' % (2 * l)] > 0).any()
    sd['actionsMLP.0.weight'] = torch.randn(5, F[-1], generator=g) * math.sqrt(2.0 / (F[-1] + 5))
    S = pc.make_gso(seed, B, E, N, Ns=Ns, f64=c['f64'])
    if Ns > N:                                             # the extra nodes are connected to real ones
        assert (S[:, :, N:, :N].abs().sum((2, 3)) > 0).all()
    return sd, obs1.reshape(B, N, 3, 11, 11), S


def build_case(c, seed=None):
    """(state_dict, observations [B,N,3,11,11], GSO [B,E,Ns,Ns]) of a case: the calibrated network of pc.make_net
    with the case's filter layers and head, drawn from the seed."""
    return _build(CASES.index(c), case_seed(c) if seed is None else seed)


def planner_config(c, dev, precision='fp32', largeGraphFilter=None):
    class Config:
        num_agents, device = c['N'], dev
        nGraphFilterTaps, dimNodeSignals, numEdgeFeatures = list(c['taps']), list(c['widths']), c['E']
        range_policy = 'flag'
    Config.precision = precision
    if largeGraphFilter is not None:
        Config.largeGraphFilter = largeGraphFilter
    return Config()


def add_gso(net, S, dev):
    """addGSO with the shape the planner takes: [B,Ns,Ns] for one edge feature, [B,E,Ns,Ns] otherwise."""
    net.addGSO((S.squeeze(1) if S.shape[1] == 1 else S).to(dev))


@functools.lru_cache(maxsize=None)
def _statements(ci, seed):
    sd, obs, S = _build(ci, seed)
    with torch.no_grad():
        return (pc.policy_statement(sd, S, obs, torch.float64)[1].numpy(),
                pc.policy_statement(sd, S, obs, torch.float32)[1].numpy())


def statements(c, seed=None):
    """(float64 logits, fp32 logits) [N,B,5] of pc.policy_statement on the case."""
    return _statements(CASES.index(c), case_seed(c) if seed is None else seed)


def filter_stack_padded_once(h, S4, p, N):
    """pc.filter_stack WITHOUT the per-layer zero padding: the signal is padded to the GSO's nodes once, every layer
    runs on all Ns nodes, the outputs are cut back to N after the last.  The statement of the defect, not of the
    planner."""
    B, Ns = h.shape[0], S4.shape[-1]
    h = torch.cat([h, h.new_zeros(B, h.shape[1], Ns - N)], 2) if Ns > N else h
    l = 0
    while 'GFL.%d.weight' % (2 * l) in p:
        w, b = p['GFL.%d.weight' % (2 * l)], p.get('GFL.%d.bias' % (2 * l))
        y = 0
        for e in range(w.shape[1]):
            z = h
            for k in range(w.shape[2]):
                if k:
                    z = z @ S4[:, e]
                y = y + torch.einsum('fg,bgn->bfn', w[:, e, k], z)
        if b is not None:
            y = y + b
        h = tF.relu(y)
        l += 1
    return h[:, :, :N]


def policy_statement_padded_once(sd, S, obs, dt):
    """Logits [N,B,5] of pc.policy_statement with filter_stack_padded_once in place of filter_stack."""
    B, N = obs.shape[:2]
    feat = pc.encoder_statement(sd, obs.reshape(B * N, 3, 11, 11), dt)
    p = {k: v.to(dt) for k, v in sd.items() if k.startswith('GFL.')}
    h = filter_stack_padded_once(feat.reshape(B, N, 128).permute(0, 2, 1), S.float().to(dt), p, N)
    return torch.einsum('af,bfn->nba', sd['actionsMLP.0.weight'].to(dt), h) + sd['actionsMLP.0.bias'].to(dt)
