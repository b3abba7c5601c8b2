"""CPU: the summary kernel (csrc/rollout_summary_kernels.hip), compiled unmodified for the host emulation, over the shared
table of shapes (tests/rollout_summary_cases.py) against the float64 numpy restatement: integers and the histogram exactly,
the doubles within the measured bound; the degenerate rules written out by hand; two calls give the same bytes; nothing is
written behind the record.  One mutant of the restatement shows that the table can tell a wrong rule."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rollout_summary_cases as rc                                                  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.load()


@pytest.mark.parametrize('C,N,G', rc.SHAPES)
def test_emu_summary_table(emu, C, N, G):
    worst = 0.0
    for with_valid, degenerate in rc.VARIANTS:
        x = rc.inputs(C, N, G, with_valid, degenerate)
        want = rc.restate(x)
        got = rc.run_host(emu, x)
        worst = max(worst, rc.check(got, want, (C, N, G, with_valid, degenerate)))
        if degenerate == 'all':                              # no case enters the rates: NaN means, NaN deviations, M2 = 0
            assert (got[0][:, rc.I_DEGENERATE] == got[0][:, rc.I_N]).all()
            assert np.isnan(got[1][:, rc.F_AVG_DMP:rc.F_STD_DFT + 1]).all() and not got[1][:, rc.F_M2_DMP:].any()
        if G == 3:
            assert got[0][0, rc.I_BAD_GROUP] == (1 if x['valid'] is None or x['valid'][C // 2] else 0)
            assert not got[0][1:, rc.I_BAD_GROUP].any() and got[0][1, rc.I_N] == 0 and not got[2][1].any()
            assert np.isnan(got[1][1, rc.F_RATE_REACH]) and tuple(got[0][1, rc.I_MIN:rc.I_MAX + 1]) == (-1, -1)
    print('largest relative difference from numpy float64 at C=%d N=%d G=%d: %.3g' % (C, N, G, worst))


@pytest.mark.parametrize('C,N,G', rc.HIST_SHAPES)
def test_emu_summary_histogram_paths(emu, C, N, G):
    for with_valid in (True, False):
        x = rc.inputs(C, N, G, with_valid, 'one')
        rc.check(rc.run_host(emu, x), rc.restate(x), (C, N, G, with_valid))


def test_emu_summary_hand_values(emu):
    """Five cases of two agents, written out by hand.  Case 0: both reach, at the expert's costs (optimal).  Case 1: one
    reaches, the other was shielded (a failure by shielding), makespan 12 against 8 and flowtime 20 against 16.  Case 2:
    degenerate (target flowtime 0), both reach.  Case 3: invalid.  Case 4: none reaches, nobody shielded, costs 10 / 5 and
    30 / 20."""
    i32 = np.int32
    x = {'C': 5, 'N': 2, 'G': 1, 'valid': np.array([1, 1, 1, 0, 2], i32), 'group': None,
         'reached': np.array([[1, 1], [1, 0], [1, 1], [0, 0], [0, 0]], i32),
         'stats': np.array([[4, 7], [12, 20], [0, 0], [99, 99], [10, 30]], i32),
         'targets': np.array([[4, 7], [8, 16], [3, 0], [1, 1], [5, 20]], i32), 'target_stride': 2,
         'shielded': np.array([[3, 0], [0, 2], [0, 0], [5, 5], [0, 0]], i32), 'audit_ok': np.array([1, 0, 1, 1, 1], i32)}
    i64, f64, hist = rc.run_host(emu, x)
    assert i64[0].tolist() == [4, 2, 2, 5, 1, 0, 4 + 12 + 10, 4 + 8 + 5, 7 + 20 + 30, 7 + 16 + 20, 0, 2, 1, 3, 2, 0]
    assert hist[0].tolist() == [1, 1, 2]
    d_mp, d_ft = np.array([0.0, 0.5, 1.0]), np.array([0.0, 0.25, 0.5])
    assert f64[0, rc.F_RATE_REACH] == 0.5 and f64[0, rc.F_MEAN_REACHED] == 1.25
    assert f64[0, rc.F_AVG_DMP] == 0.5 and f64[0, rc.F_AVG_DFT] == 0.25
    assert f64[0, rc.F_M2_DMP] == 0.5 and f64[0, rc.F_M2_DFT] == 0.125
    assert f64[0, rc.F_STD_DMP] == np.std(d_mp, ddof=1) == 0.5 and f64[0, rc.F_STD_DFT] == np.std(d_ft, ddof=1) == 0.25
    assert rc.check((i64, f64, hist), rc.restate(x), 'hand') == 0.0
    # one case left for the rates: its mean, and numpy's NaN for the deviation
    x['valid'] = np.array([0, 1, 1, 0, 0], i32)
    i64, f64, _ = rc.run_host(emu, x)
    assert i64[0, rc.I_N] == 2 and i64[0, rc.I_DEGENERATE] == 1
    assert f64[0, rc.F_AVG_DMP] == 0.5 and np.isnan(f64[0, rc.F_STD_DMP]) and f64[0, rc.F_M2_DMP] == 0.0
    # no valid case at all
    x['valid'] = np.zeros(5, i32)
    i64, f64, hist = rc.run_host(emu, x)
    assert i64[0].tolist() == [0] * 10 + [-1, -1, 0, 0, 0, 0] and not hist.any()
    assert np.isnan(f64[0, :rc.F_M2_DMP]).all() and not f64[0, rc.F_M2_DMP:].any()


def test_emu_summary_two_calls_give_the_same_bytes(emu):
    x = rc.inputs(600, 3, 3, True, 'one')
    a, b = rc.run_host(emu, x), rc.run_host(emu, x, poison=0xa5)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


def test_emu_summary_mutant_degenerate_cases_in_the_divisor(emu):
    """One-off mutant of the restatement: the rates' divisor is n instead of n - n_degenerate.  Every entry of the table
    with a degenerate case among the valid ones must tell."""
    x = rc.inputs(257, 3, 1, False, 'one')
    got, want = rc.run_host(emu, x), rc.restate(x)
    m = int(want[0][0, rc.I_N] - want[0][0, rc.I_DEGENERATE])
    assert want[0][0, rc.I_DEGENERATE] == 1
    wrong = want[1].copy()
    wrong[0, rc.F_AVG_DMP] *= m / (m + 1.0)
    assert rc.rel_diff(got[1], want[1]) <= rc.TOL < 1e-3 < rc.rel_diff(got[1], wrong)
