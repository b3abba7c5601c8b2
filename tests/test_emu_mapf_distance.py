"""CPU: gnnpp_mapf_distances and gnnpp_mapf_orders (csrc/mapf_distance_kernels.hip), compiled unmodified for the host
emulation, against a queue-based breadth-first search and an np.lexsort restatement of the ranking rules
(tests/mapf_distance_cases.py): exact equality of every output element.  Then the chain distances -> orders -> solve at
the C level on the case that shows the feature (the index order fails, longest first solves it), on a seeded set against
the yardstick of the solver, the documented error codes, and the host-side step limit.  tests/test_gpu_mapf_distance.py
runs the same cases on the device."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mapf_cases as mc  # noqa: E402
import mapf_distance_cases as dc  # noqa: E402
from gnn_pathplanning_amd._native import ERR_ARG, ERR_UNSUPPORTED  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')
POISON = dc.POISON


@pytest.fixture(scope='module')
def lib():
    import emu_lib
    return emu_lib.load()


def _ptr(a):
    return None if a is None else a.ctypes.data


def call_distances(lib, grid, starts, goals, expect=0, null=None, dims=None):
    """One call on host arrays with poisoned outputs.  null: the name of an output passed as NULL; dims: (C, N, H, W)
    the call is TOLD (the arrays are never smaller than what a call that passes its checks reads)."""
    grid = np.ascontiguousarray(grid, dtype=np.uint8)
    start, goal = np.ascontiguousarray(starts, dtype=np.int32), np.ascontiguousarray(goals, dtype=np.int32)
    C, N = start.shape[:2]
    H, W = grid.shape[-2:]
    out = {'dist': np.full((C, N), POISON, np.int32), 'lower_makespan': np.full(C, POISON, np.int32),
           'lower_flowtime': np.full(C, POISON, np.int32)}
    tC, tN, tH, tW = dims or (C, N, H, W)
    rc = lib.gnnpp_mapf_distances(_ptr(grid), int(grid.ndim == 3), _ptr(start), _ptr(goal), tC, tN, tH, tW,
                                  *[None if k == null else _ptr(out[k]) for k in ('dist', 'lower_makespan', 'lower_flowtime')],
                                  None)
    assert rc == expect, rc
    return out


def call_orders(lib, dist, rules, seed=0, expect=0, N=None, null_order=False):
    """dist [C,N] or None; rules: names of dc.RULES or raw codes."""
    d = None if dist is None else np.ascontiguousarray(dist, dtype=np.int32)
    C, n = (1, N) if d is None else d.shape
    N = n if N is None else N
    R = len(rules)
    codes = (ctypes.c_int * max(R, 1))(*[dc.RULES.get(r, r) for r in rules])
    order = np.full((C, max(R, 1), min(N, 1024)), POISON, np.int32)
    rc = lib.gnnpp_mapf_orders(_ptr(d), C, N, R, codes, seed, None if null_order else _ptr(order), None)
    assert rc == expect, rc
    return order


def run_case(lib, name, shared=False):
    case = dc.CASES[name]()
    out = call_distances(lib, case['grid'][0] if shared else case['grid'], case['starts'], case['goals'])
    dc.assert_equal_to_yardstick(case, out['dist'], out['lower_makespan'], out['lower_flowtime'])
    return out


# ---- distances -----------------------------------------------------------------------------------------------------
def test_one_and_two_cells(lib):
    assert run_case(lib, 'one_cell_start_is_goal')['dist'].tolist() == [[0]]
    assert run_case(lib, 'two_cells')['dist'].tolist() == [[1, 1, 0]]


@pytest.mark.parametrize('W', [63, 64, 65, 128, 129])
def test_rows_across_the_word_boundaries(lib, W):
    """The carries of the horizontal shifts in both directions (a one-row strip), and the vertical step next to a
    boundary (a wall with gaps at columns 63 / 64 and 127 / 128); 5 x 65 is an item of 10 threads."""
    run_case(lib, 'strip_W%d' % W)
    run_case(lib, 'doors_at_the_word_boundaries_W%d' % W)


def test_one_wave_items_finish_at_different_steps(lib):
    out = run_case(lib, 'one_wave_items_finish_at_different_steps')
    assert out['dist'][0, :7].tolist() == [126, 64, 0, -1, -2, -2, 0]


def test_several_items_per_workgroup_end_one_bit_past_a_word(lib):
    """7 x 65: four items of 14 threads in a workgroup and a partial second batch, the only door in the bit of word 1."""
    assert run_case(lib, 'several_items_per_workgroup_end_one_bit_past_a_word')['dist'][0, 6] == 130


def test_largest_map(lib):
    assert run_case(lib, 'largest_map_nearly_open')['dist'][0, :2].tolist() == [510, 510]


def test_walled_off_goal_ends_when_the_layer_stops_growing(lib):
    """On 256 x 256 the loop's bound is 65536 steps of 1024 lane-accurate threads: this test finishes only because the
    search ends at the first layer that gains no bit."""
    assert run_case(lib, 'small_map_goal_walled_off')['dist'].tolist() == [[-1, 2, -1, 4]]
    assert run_case(lib, 'largest_map_goal_walled_off')['dist'].tolist() == [[-1, 300]]


@pytest.mark.parametrize('n', [9, 15])
def test_serpentine_beyond_the_solver_horizon(lib, n):
    out = run_case(lib, 'serpentine_%d' % n)
    assert n < 15 or out['dist'][0, 0] > mc.default_horizon(n, n)


def test_invalid_ends_flag_only_themselves(lib):
    out = run_case(lib, 'invalid_ends_flag_only_themselves')
    assert out['dist'][1].tolist() == [-2, -2, -2, 4] and out['lower_makespan'].tolist() == [10, -1, 10]


def test_shared_grid_next_to_batched_grid(lib):
    shared = run_case(lib, 'shared_grid_next_to_batched_grid', shared=True)
    batched = run_case(lib, 'shared_grid_next_to_batched_grid')
    for k in shared:
        assert shared[k].tobytes() == batched[k].tobytes(), k


def test_more_items_than_the_persistent_grid(lib):
    run_case(lib, 'more_items_than_the_persistent_grid')


# ---- orders --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', dc.ORDER_SIZES)
def test_orders_equal_the_lexsort_twin(lib, N):
    """Three cases of synthetic keys (heavy ties, -1 / -2 among distances, distinct keys up to the largest int32): all
    four rules in one call, then each rule alone."""
    keys = dc.synthetic_keys(N)
    got = call_orders(lib, keys, dc.ALL_RULES, seed=5)
    dc.assert_permutations(got, N)
    assert np.array_equal(got, dc.rank_orders(keys, dc.ALL_RULES, seed=5))
    for rule in dc.ALL_RULES:
        alone = call_orders(lib, keys, [rule], seed=5)
        assert np.array_equal(alone, dc.rank_orders(keys, [rule], seed=5)), rule


def test_orders_rules_in_any_number_and_without_keys(lib):
    """35 restarts: two launches of the order kernel (32 rules each at most); the hash depends on the restart's index.
    Index and hashed orders need no keys."""
    keys = dc.synthetic_keys(7)
    rules = (dc.ALL_RULES * 9)[:35]
    assert np.array_equal(call_orders(lib, keys, rules, seed=9), dc.rank_orders(keys, rules, seed=9))
    got = call_orders(lib, None, ['index', 'hashed', 'hashed'], seed=3, N=6)
    assert np.array_equal(got, dc.rank_orders(np.zeros((1, 6)), ['index', 'hashed', 'hashed'], seed=3))
    assert got[0, 1].tolist() != got[0, 2].tolist()
    assert got[0, 1].tolist() != call_orders(lib, None, ['index', 'hashed'], seed=4, N=6)[0, 1].tolist()


def test_negative_keys_rank_first_under_both_distance_rules(lib):
    got = call_orders(lib, np.array([[3, -1, 7, -2, 3, 0]]), ['longest_first', 'shortest_first'])
    assert got[0].tolist() == [[1, 3, 2, 0, 4, 5], [1, 3, 5, 0, 4, 2]]


# ---- the chain distances -> orders -> solve ------------------------------------------------------------------------
def solve_with_rules(lib, grid, starts, goals, T, rules, seed=0, team=False):
    """What mapf.solve(priorities=<string>) enqueues, at the C level: (solver outputs, distances' outputs, orders)."""
    from test_emu_mapf_team import call
    d = call_distances(lib, grid, starts, goals)
    order = call_orders(lib, d['dist'], rules, seed) if rules is not None else None
    return call(lib, grid, starts, goals, T, order, team=team), d, order


@pytest.mark.parametrize('team', [False, True])
def test_longest_first_solves_what_the_index_order_does_not(lib, team):
    grid, starts, goals, T = dc.corridor_2x4()
    out, d, _ = solve_with_rules(lib, grid, starts[None], goals[None], T, None, team=team)
    assert (out['status'][0], out['failing'][0], out['arrival'][0].tolist()) == (mc.NO_PATH, 1, [1, -1])
    assert d['dist'].tolist() == [[1, 3]] and d['lower_makespan'].tolist() == [3] and d['lower_flowtime'].tolist() == [4]
    out, _, order = solve_with_rules(lib, grid, starts[None], goals[None], T, ['longest_first'], team=team)
    assert order.tolist() == [[[1, 0]]]
    assert (out['status'][0], out['failing'][0], out['arrival'][0].tolist()) == (0, -1, [3, 3])
    mc.assert_outputs_equal(out, [mc.solve_case(grid, starts, goals, T, [[1, 0]])])


def test_mixed_orders_equal_explicit_orders_and_respect_the_bounds(lib):
    """6 cases of 10 agents on 20 x 20, 'mixed' with four restarts: every output equals the solver's yardstick run on the
    twin's orders, and every solved case respects the lower bounds."""
    cases = dc.explicit_order_sets()[0]
    grids, starts, goals = (np.stack([c[k] for c in cases]) for k in range(3))
    T = mc.default_horizon(20, 20)
    out, d, order = solve_with_rules(lib, grids, starts, goals, T, dc.mixed_rules(4), seed=3)
    want_d = dc.want_distances(grids, starts, goals)
    assert np.array_equal(d['dist'], want_d[0])
    twin = dc.rank_orders(want_d[0], dc.mixed_rules(4), seed=3)
    assert np.array_equal(order, twin)
    mc.assert_outputs_equal(out, [mc.solve_case(*cases[c], T, list(twin[c])) for c in range(len(cases))])
    solved = out['status'] == 0
    assert solved.any()
    assert (out['arrival'][solved] >= d['dist'][solved]).all()
    assert (out['makespan'][solved] >= d['lower_makespan'][solved]).all()
    assert (out['flowtime'][solved] >= d['lower_flowtime'][solved]).all()


# ---- errors --------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(lib):
    grid = np.zeros((4, 4), np.uint8)
    s, g = np.array([[[0, 0], [1, 1]]]), np.array([[[3, 3], [2, 2]]])
    assert call_distances(lib, grid, s, g)['dist'].tolist() == [[6, 2]]
    many = np.zeros((1, 1025, 2), np.int32)
    for kw, code in ((dict(starts=many, goals=many), ERR_ARG), (dict(dims=(1, 2, 257, 4)), ERR_UNSUPPORTED),
                     (dict(dims=(1, 2, 4, 257)), ERR_UNSUPPORTED), (dict(null='dist'), ERR_ARG),
                     (dict(null='lower_makespan'), ERR_ARG), (dict(null='lower_flowtime'), ERR_ARG),
                     (dict(dims=(0, 2, 4, 4)), ERR_ARG), (dict(dims=(1, 0, 4, 4)), ERR_ARG),
                     (dict(dims=(1, 2, 0, 4)), ERR_ARG),
                     # N is refused before the map size is looked at
                     (dict(starts=many, goals=many, dims=(1, 1025, 257, 4)), ERR_ARG)):
        args = dict(grid=grid, starts=s, goals=g)
        args.update(kw)
        out = call_distances(lib, args.pop('grid'), args.pop('starts'), args.pop('goals'), expect=code, **args)
        for k in out:
            assert (out[k] == POISON).all(), (kw, k)            # nothing enqueued
    keys = np.array([[1, 2, 3]])
    for kw, rules in ((dict(N=1025), ['index']), (dict(null_order=True), ['index']), (dict(), [4]), (dict(), [-1]),
                      (dict(), [])):
        assert (call_orders(lib, keys if 'N' not in kw else None, rules, expect=ERR_ARG, **kw) == POISON).all()
    assert (call_orders(lib, None, ['index', 'longest_first'], expect=ERR_ARG, N=3) == POISON).all()   # a rule needs keys
    assert lib.gnnpp_mapf_orders(_ptr(keys.astype(np.int32)), 1, 3, 1, None, 0, _ptr(np.zeros(3, np.int32)), None) == ERR_ARG


# ---- the step limit (host arithmetic on the bounds) ----------------------------------------------------------------
def test_maxstep_from_distances():
    """rate * lower_makespan by hand: 1.5 * (4, 7, 0, 1) = 6, 10.5, 0, 1.5 -> 6, 11, 1 (at least one step), 2."""
    import torch
    from gnn_pathplanning_amd import _native, mapf
    got = mapf.maxstep_from_distances(torch.tensor([4, 7, 0, 1], dtype=torch.int32), 1.5)
    assert got.dtype == torch.int32 and got.tolist() == [6, 11, 1, 2]
    assert mapf.maxstep_from_distances(np.array([3, 510]), 2).tolist() == [6, 1020]
    with pytest.raises(_native.GnnppError, match='cannot reach'):
        mapf.maxstep_from_distances(torch.tensor([4, -1, 2]), 2.0)
