"""CPU: the planner route matrix of tests/planner_route_cases.py reaches every route, and every case that has a GSO
larger than the team and several filter layers is SENSITIVE to the per-layer zero padding -- so that the GPU tests
built on the matrix (tests/test_gpu_planner_routes_f64.py) cannot pass on a planner that pads only once."""
import numpy as np
import pytest
import torch

import planner_route_cases as prc
import policy_f64_cases as pc
from f64_yardstick import gap

# the float64 difference a single padding makes must exceed the largest error the yardstick allows by this factor:
# a condition on the inputs, not a tolerance (a case that falls short gets other inputs, not another factor)
SENSITIVITY = 1000.0

REQUIRED = (   # (N, Ns, taps, widths, E) -> (eval routes, train route)
    ((6, 9, (3, 3), (128, 128), 1), {'small_general'}, 'train_padded'),
    ((50, 64, (2, 3, 2), (64, 48, 128), 2), {'small_general'}, 'train_padded'),
    ((20, 28, (2, 2), (128, 160), 1), {'small_general+gemm_head'}, 'train_padded'),
    ((100, 120, (3, 2), (128, 128), 1), {'dense', 'lists'}, 'train_dense'),
    ((130, 150, (2, 3), (64, 48), 2), {'dense', 'lists'}, 'train_dense'),
    ((6, 6, (3, 3), (128, 128), 1), {'small_general'}, 'train_direct'),
    ((6, 9, (3,), (128,), 1), {'small_general'}, 'train_padded'),
)


def _key(c):
    return (c['N'], c['Ns'], c['taps'], c['widths'], c['E'])


def test_restated_limits_are_the_packages():
    import gnn_pathplanning_amd.graphML as gml
    assert (prc.MAX_NODES, prc.TEAM_MAX_NODES) == (gml.MAX_NODES, gml.TEAM_MAX_NODES)


def test_case_list_reaches_every_route():
    reached = set()
    for c in prc.CASES:
        reached |= prc.case_routes(c, False) | prc.case_routes(c, True)
    assert reached == set(prc.EVAL_ROUTES) | set(prc.TRAIN_ROUTES)


@pytest.mark.parametrize('key,eval_routes,train_route', REQUIRED, ids=lambda v: None)
def test_required_rows_and_their_routes(key, eval_routes, train_route):
    rows = [c for c in prc.CASES if _key(c) == key]
    assert rows, key
    for c in rows:
        assert prc.case_routes(c, False) == eval_routes
        assert prc.case_routes(c, True) == {train_route}


def test_fp64_gso_variants_present():
    for key in (REQUIRED[0][0], REQUIRED[3][0]):
        assert {c['f64'] for c in prc.CASES if _key(c) == key} == {False, True}


def test_route_edges():
    r = prc.route
    assert r(False, 112, 112, 1, 1, (128,)) == 'policy_fwd'
    assert r(False, 113, 113, 1, 1, (128,)) == 'dense'
    assert r(False, 113, 113, 1, 1, (128,), largeGraphFilter='lists') == 'lists_one_call'
    assert r(False, 113, 113, 1, 1, (128,), 'split_f16', 'lists') == 'dense'
    assert r(False, 113, 113, 1, 1, (64,), largeGraphFilter='lists') == 'lists'
    assert r(False, 100, 113, 1, 1, (128,), largeGraphFilter='lists') == 'lists'
    assert r(False, 10, 10, 1, 2, (64,)) == 'small_general'
    assert r(False, 10, 10, 1, 1, (129,)) == 'small_general+gemm_head'
    assert r(True, 112, 112, 2, 1, (128, 128)) == 'train_direct'
    assert r(True, 111, 112, 1, 1, (128,)) == 'train_padded'
    assert r(True, 113, 113, 1, 1, (128,)) == 'train_dense'


def test_package_route_function_is_the_restated_one():
    """The package's one route decision (decentralplanner.planner_route) against the restatement of this suite, over
    every combination of the grid; largeGraphTraining='lists' turns training on more than MAX_NODES nodes into
    'train_lists' and changes nothing else."""
    import itertools
    from gnn_pathplanning_amd.decentralplanner import planner_route
    grid = itertools.product((False, True),
                             ((6, 6), (6, 9), (112, 112), (111, 112), (113, 113), (100, 113), (1024, 1024)),
                             ((1, (128,)), (1, (64,)), (1, (129,)), (2, (128, 128)), (2, (128, 160))),
                             (1, 2), prc.PRECISIONS, ('dense', 'lists'))
    n = 0
    for training, (N, Ns), (L, widths), E, prec, lgf in grid:
        want = prc.route(training, N, Ns, L, E, widths, prec, lgf)
        assert planner_route(training, N, Ns, L, E, widths, prec, lgf, 'dense') == want, (training, N, Ns, L, E, prec, lgf)
        assert planner_route(training, N, Ns, L, E, widths, prec, lgf) == want           # 'dense' is the default
        lists = planner_route(training, N, Ns, L, E, widths, prec, lgf, 'lists')
        assert lists == ('train_lists' if training and Ns > prc.MAX_NODES else want), (training, N, Ns, L, E, prec, lgf)
        n += 1
    assert n == 2 * 7 * 5 * 2 * 3 * 2


@pytest.mark.parametrize('case', prc.CASES, ids=prc.case_id)
def test_case_inputs(case):
    """Shapes, dtypes, non-zero biases on every layer and logits of the scale the yardstick's floor assumes."""
    sd, obs, S = prc.build_case(case)
    B, N, Ns, E = case['B'], case['N'], case['Ns'], case['E']
    assert obs.shape == (B, N, 3, 11, 11) and S.shape == (B, E, Ns, Ns)
    assert S.dtype == (torch.float64 if case['f64'] else torch.float32)
    F = (128,) + case['widths']
    for l, K in enumerate(case['taps']):
        assert sd['GFL.%d.weight' % (2 * l)].shape == (F[l + 1], E, K, F[l])
        b = sd['GFL.%d.bias' % (2 * l)]
        assert b.shape == (F[l + 1], 1) and (b > 0).any() and (b != 0).all()
    assert sd['actionsMLP.0.weight'].shape == (5, F[-1])
    l64, _ = prc.statements(case)
    assert l64.shape == (N, B, 5) and 1e-3 < np.abs(l64).max() < 10.0


@pytest.mark.parametrize('case', [c for c in prc.CASES if prc.needs_repadding(c)], ids=prc.case_id)
def test_padding_once_is_far_outside_the_yardstick(case):
    """max |logits padded once - logits padded per layer| in float64 >= SENSITIVITY x the largest error the yardstick
    (f64_yardstick.gap through pc.allowed_error) allows on the case, the allowance taken from the float64 and fp32
    CPU statements alone."""
    sd, obs, S = prc.build_case(case)
    l64, l32 = prc.statements(case)
    with torch.no_grad():
        wrong = prc.policy_statement_padded_once(sd, S, obs, torch.float64).numpy()
    _, rep = gap(l32, l64, l32)
    allowed = pc.allowed_error(rep)
    delta = float(np.abs(wrong - l64).max())
    print('%s: |padded once - per layer| = %.3g, allowed %.3g (x %.0f), logit scale %.3g'
          % (prc.case_id(case), delta, allowed, delta / allowed, rep['scale']))
    assert delta >= SENSITIVITY * allowed, (delta, allowed)


@pytest.mark.parametrize('case', [c for c in prc.CASES if not prc.needs_repadding(c)], ids=prc.case_id)
def test_controls_have_nothing_to_pad_again(case):
    """One layer, or a GSO of the team's size: both statements are the same computation."""
    sd, obs, S = prc.build_case(case)
    l64, _ = prc.statements(case)
    with torch.no_grad():
        once = prc.policy_statement_padded_once(sd, S, obs, torch.float64).numpy()
    assert np.array_equal(once, l64)
