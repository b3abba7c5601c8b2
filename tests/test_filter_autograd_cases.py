"""CPU: the cases of tests/filter_autograd_cases.py can tell a wrong graph filter from a right one before any GPU sees
them, so that tests/test_gpu_filter_autograd_f64.py cannot pass on an implementation with one of the listed mistakes.

(a) the float64 statement (autograd over the tap recursion) agrees with an independently written formulation (einsums
    over numpy.linalg.matrix_power, every gradient by its formula) within 64 x 2^-53 x the tensor's scale: float64
    roundoff of contractions of at most 512 x 130 terms summed in another order;
(b) for every case, each wrong variant that applies to it differs from the float64 statement, in every tensor named for
    the variant, by more than SENSITIVITY x what the yardstick allows there (MAX_K x the fp32 statement's largest
    error + the floor): a condition on the inputs, not a tolerance;
(c) no two cases are the same call, every route is named by at least two cases, and the case list holds what the device
    test is meant to cover."""
import numpy as np
import pytest

import filter_autograd_cases as fa
from f64_yardstick import gap

SENSITIVITY = 1000.0                       # the project's own factor (tests/test_planner_routes.py)
F64_BOUND = 64 * 2.0 ** -53
FILTER = [c for c in fa.CASES if c['entry'] != 'matrixPowersBatch']
POWERS = [c for c in fa.CASES if c['entry'] == 'matrixPowersBatch']
TENSORS = ('y', 'dh', 'dx', 'db')


def _scale(a):
    return float(np.abs(a).max())


@pytest.mark.parametrize('case', FILTER, ids=fa.case_id)
def test_statement_is_the_explicit_formulation(case):
    w64, _, _, _ = fa.statements(case)
    ex = fa.explicit(case)
    for t in TENSORS:
        if w64[t] is None:
            assert ex[t] is None and case['bias'] is None
            continue
        assert w64[t].shape == ex[t].shape, t
        err = float(np.abs(w64[t] - ex[t]).max())
        assert err <= F64_BOUND * _scale(ex[t]), (t, err, _scale(ex[t]))


@pytest.mark.parametrize('case', POWERS, ids=fa.case_id)
def test_powers_statement_is_matrix_power(case):
    S = fa.inputs(case)['S']
    for Sx in (S, S.astype(np.float32)):
        got, want = fa.powers_statement(Sx, case['K'], np.float64), fa.explicit_powers(Sx, case['K'])
        assert got.shape == want.shape == S.shape[:-2] + (max(case['K'], 1),) + S.shape[-2:]
        assert float(np.abs(got - want).max()) <= F64_BOUND * _scale(want)


def _allowed(case, t):
    w64, w32, _, _ = fa.statements(case)
    _, rep = gap(w32[t], w64[t], w32[t])
    return fa.allowed_error(rep)


@pytest.mark.parametrize('case', FILTER, ids=fa.case_id)
def test_wrong_variants_are_far_outside_the_yardstick(case):
    w64, _, _, _ = fa.statements(case)
    applied = 0
    for wrong in fa.WRONG:
        if not fa.applies(case, wrong):
            continue
        applied += 1
        bad = fa.explicit(case, wrong)
        for t in fa.WRONG_SHOWS[wrong]:
            delta, allowed = float(np.abs(bad[t] - w64[t]).max()), _allowed(case, t)
            print('%s: %s in %s: %.3g, allowed %.3g (x %.0f)' % (case['name'], wrong, t, delta, allowed, delta / allowed))
            assert delta >= SENSITIVITY * allowed, (wrong, t, delta, allowed)
    assert applied >= 1


@pytest.mark.parametrize('case', [c for c in POWERS if fa.applies(c, 'short_chain')], ids=fa.case_id)
def test_short_power_chain_is_far_outside_the_yardstick(case):
    S, K = fa.inputs(case)['S'], case['K']
    if case['f64']:                       # held to numpy float64 within 8 N 2^-53 max |P_k|
        want = fa.explicit_powers(S, K)
        allowed = 8 * case['N'] * 2.0 ** -53 * _scale(want[..., K - 1, :, :])
    else:
        S32 = S.astype(np.float32)
        want = fa.powers_statement(S32, K, np.float64)
        p32 = fa.powers_statement(S32, K, np.float32)
        _, rep = gap(p32[..., K - 1, :, :], want[..., K - 1, :, :], p32[..., K - 1, :, :])
        allowed = fa.allowed_error(rep)
    bad = fa.explicit_powers(S if case['f64'] else S.astype(np.float32), K, 'short_chain')
    delta = float(np.abs(bad - want).max())
    assert delta >= SENSITIVITY * allowed, (delta, allowed)


@pytest.mark.parametrize('case', [c for c in FILTER if c['relu']], ids=fa.case_id)
def test_relu_masks_do_not_hang_on_roundoff(case):
    """No pre-activation within 8 allowances of 0: an implementation inside the yardstick has the statement's mask."""
    w64, w32, mask, _ = fa.statements(case)
    _, rep = gap(w32['pre'], w64['pre'], w32['pre'])
    assert float(np.abs(w64['pre']).min()) > 8 * fa.allowed_error(rep)
    assert np.array_equal(w32['pre'] > 0, mask > 0)
    assert 0.2 < mask.mean() < 0.8


def test_inputs_are_what_the_cases_say():
    for c in fa.CASES:
        inp = fa.inputs(c)
        S = inp['S']
        assert S.dtype == np.float64 and S.shape[-1] == S.shape[-2] == c['N']
        flat = S.reshape(-1, c['N'], c['N'])
        for M in flat:
            assert (M != M.astype(np.float32)).any()                          # not an fp32 number when given as fp64
            assert M.min() >= 0 and M.sum(1).max() <= 1 + 1e-12 and M.sum(1).min() >= 0.7 - 1e-12
            assert (M != 0).sum(1).max() <= 3
            if c['N'] > 2:
                assert np.abs(M - M.T).max() > 0.25 * np.abs(M).max()        # S and S^T differ by O(1)
        if c['entry'] == 'matrixPowersBatch':
            assert S.ndim == c['dim']
            continue
        B, G, F, K, E, N, Nin = (c[k] for k in ('B', 'G', 'F', 'K', 'E', 'N', 'Nin'))
        assert inp['h'].shape == (F, E, K, G) and inp['x'].shape == (B, G, Nin) and inp['dy'].shape == (B, F, Nin)
        assert S.shape == ((B, E, N, N) if c['batched'] else (E, N, N))
        assert (inp['b'] is None) == (c['bias'] is None)
        if c['bias']:
            assert inp['b'].shape == (F, N if c['bias'] == 'node' else 1) and (inp['b'] != 0).all()
        if c['fold'] & 2:
            assert 0.3 < (inp['x'] == 0).mean() < 0.7 and (inp['x'] >= 0).all()


def test_no_collapsed_pairs_and_every_route_twice():
    keys = [fa.call_key(c) for c in fa.CASES]
    assert len(set(keys)) == len(keys)
    names = [c['name'] for c in fa.CASES]
    assert len(set(names)) == len(names)
    for r in fa.ROUTES:
        assert sum(c['route'] == r for c in fa.CASES) >= 2, r
    assert {c['route'] for c in fa.CASES} == set(fa.ROUTES)
    for c in fa.CASES:
        assert c['B'] <= 4 and c['N'] <= 130
        if c['entry'] != 'matrixPowersBatch':
            assert max(c['G'], c['F']) <= 128 or 512 in (c['G'], c['F']) or c['F'] == 160
            assert not c['fold'] & 4 and (not c['fold'] or c['entry'] == 'apply')


def test_case_list_holds_the_required_rows():
    def has(**kw):
        return any(all(c.get(k) == v for k, v in kw.items()) for c in fa.CASES)
    for N in (113, 130):
        assert has(route='dense', N=N, G=24, F=40)
    dense = [c for c in fa.CASES if c['route'] == 'dense' and c['N'] > 112]
    assert {c['K'] for c in dense} >= {1, 3, 4} and {c['E'] for c in dense} == {1, 2}
    assert {c['batched'] for c in dense} == {True, False} and any(c['f64'] for c in dense)
    assert {c['N'] - c['Nin'] for c in dense} >= {0, 1} and any(c['Nin'] == 1 for c in dense)
    assert {c['bias'] for c in dense} == {None, 'feat', 'node'}
    assert {c['relu'] for c in dense if c['entry'] == 'forward_node_major'} == {True, False}
    assert has(route='dense', N=50, G=512, F=16) and has(route='dense', N=112, G=128, F=128)
    assert has(route='lds', N=112, G=16, F=16)
    assert has(route='mixed-dx', N=50, G=16, F=512, Nin=50) and has(route='mixed-dx', N=50, G=16, F=512, Nin=37)
    assert {c['fold'] for c in fa.CASES if c['entry'] == 'apply' and c['route'] == 'mixed-dx'} == {0, 1, 2, 3}
    assert has(route='lds', N=20, Nin=13, E=2) and has(route='lds', Nin=13, bias='node')
    assert has(route='lds', batched=False) and has(route='lds', N=1, K=3) and has(route='lds', N=16)
    assert has(route='lds', N=17) and has(route='lds', F=160) and has(route='lds', K=1) and has(route='lds', B=1)
    mp = [c for c in fa.CASES if c['entry'] == 'matrixPowersBatch']
    assert {c['K'] for c in mp} == {1, 2, 3, 4} and {c['E'] for c in mp} == {1, 2} and {c['dim'] for c in mp} == {3, 4}
    assert {c['N'] for c in mp if not c['f64']} >= {5, 17, 100, 113} and any(c['f64'] for c in mp)
    assert {c['K'] > 2 for c in mp if c.get('s_view')} == {True, False}
    assert has(entry='GraphFilterBatchGSO', N=10, E=2, K=3) and has(entry='GraphFilterBatchGSO', N=120, E=2, K=3)
    for route in fa.FILTER_ROUTES:
        rows = [c for c in fa.CASES if c['route'] == route]
        assert {c['needs'] for c in rows} >= {'h', 'x', 'b', 'hxb'}, route
        assert any(c['dy_view'] for c in rows) and any(c['retain'] for c in rows), route
        assert {c['dscale'] for c in rows} >= {1e-6, 1.0, 1e3}, route
    for route in ('lds', 'mixed-dx'):
        assert {c['prec'] for c in fa.CASES if c['route'] == route} >= {0, 1, 2}, route


def test_named_routes_agree_with_the_library_room_check():
    """gnnpp_lsigf_fits (a host function of the library) accepts the forward launch of every `lds` / `mixed-dx` case
    and the input-gradient launch (widths swapped) of every `lds` case, and refuses the one the route says is refused."""
    from gnn_pathplanning_amd import _native
    _native.build()
    lib = _native.lib()
    for c in FILTER:
        E, K = (c['E'] * c['K'], 2) if c['entry'] in fa.PRE_POWERED else (c['E'], c['K'])
        fwd = c['N'] <= 112 and lib.gnnpp_lsigf_fits(c['N'], c['G'], c['F'], K, E) == 1
        bwd = c['N'] <= 112 and lib.gnnpp_lsigf_fits(c['N'], c['F'], c['G'], K, E) == 1
        want = 'dense' if not fwd else 'lds' if bwd else 'mixed-dx'
        assert fa.filter_route(c) == want, (c['name'], fwd, bwd)
