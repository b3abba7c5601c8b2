"""CPU: gnnpp_mapf_solve (csrc/mapf_kernels.hip), compiled unmodified for the host emulation, against the sequential
numpy restatement of the contract (tests/mapf_cases.py): equality of every output element, on small random cases and
on hand-built edge cases."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mapf_cases as mc  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')

ERR_ARG, ERR_UNSUPPORTED = -1, -2
POISON = -7


class Mapf(ctypes.Structure):
    """struct gnnpp_mapf (include/gnnpp.h)."""
    _fields_ = [('grid', ctypes.c_void_p), ('grid_batched', ctypes.c_int), ('start', ctypes.c_void_p),
                ('goal', ctypes.c_void_p), ('order', ctypes.c_void_p), ('C', ctypes.c_int), ('N', ctypes.c_int),
                ('H', ctypes.c_int), ('W', ctypes.c_int), ('R', ctypes.c_int), ('T_max', ctypes.c_int),
                ('schedule', ctypes.c_void_p), ('arrival', ctypes.c_void_p), ('makespan', ctypes.c_void_p),
                ('flowtime', ctypes.c_void_p), ('status', ctypes.c_void_p), ('failing', ctypes.c_void_p),
                ('restart', ctypes.c_void_p), ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t)]


@pytest.fixture(scope='module')
def lib():
    import emu_lib
    L = emu_lib.load()
    L.gnnpp_mapf_solve.argtypes = [ctypes.POINTER(Mapf), ctypes.c_void_p]
    L.gnnpp_mapf_solve.restype = ctypes.c_int
    L.gnnpp_mapf_workspace_bytes.argtypes = [ctypes.c_int] * 4
    L.gnnpp_mapf_workspace_bytes.restype = ctypes.c_size_t
    return L


def call(lib, grids, starts, goals, T, orders=None, expect=0, ws_bytes=None):
    """One gnnpp_mapf_solve call on host arrays; outputs start out poisoned, so an element the call does not write
    cannot pass for one it wrote."""
    grid = np.ascontiguousarray(grids, dtype=np.uint8)
    start = np.ascontiguousarray(starts, dtype=np.int32)
    goal = np.ascontiguousarray(goals, dtype=np.int32)
    C, N = start.shape[:2]
    order = None if orders is None else np.ascontiguousarray(orders, dtype=np.int32)
    R = 1 if order is None else order.shape[1]
    H, W = grid.shape[-2:]
    need = lib.gnnpp_mapf_workspace_bytes(C, R, min(H, 64), T)
    ws = np.zeros(max(need, 8) // 8 + 1, np.uint64)
    out = {'schedule': np.full((C, T + 1, N, 2), POISON, np.int32), 'arrival': np.full((C, N), POISON, np.int32)}
    for k in ('makespan', 'flowtime', 'status', 'failing', 'restart'):
        out[k] = np.full(C, POISON, np.int32)
    m = Mapf()
    m.grid, m.grid_batched, m.start, m.goal = grid.ctypes.data, int(grid.ndim == 3), start.ctypes.data, goal.ctypes.data
    m.order = order.ctypes.data if order is not None else None
    m.C, m.N, m.H, m.W, m.R, m.T_max = C, N, H, W, R, T
    for k in out:
        setattr(m, k, out[k].ctypes.data)
    m.workspace, m.workspace_bytes = ws.ctypes.data, need if ws_bytes is None else ws_bytes
    assert lib.gnnpp_mapf_solve(ctypes.byref(m), None) == expect
    return out


def assert_matches(out, c, want):
    for k in ('status', 'restart', 'makespan', 'flowtime', 'failing'):
        assert int(out[k][c]) == want[k], (k, int(out[k][c]), want[k])
    assert np.array_equal(out['arrival'][c], want['arrival'])
    assert np.array_equal(out['schedule'][c], want['schedule'])


def run_and_compare(lib, cases, T, orders=None, batched=True):
    """cases: [(grid, starts, goals)] of one map size; every output of every case equal to the yardstick's."""
    grids = np.stack([g for g, _, _ in cases]) if batched else cases[0][0]
    out = call(lib, grids, np.stack([s for _, s, _ in cases]), np.stack([g for _, _, g in cases]), T, orders)
    wants = []
    for c, (g, s, gl) in enumerate(cases):
        want = mc.solve_case(g, s, gl, T, None if orders is None else list(orders[c]))
        assert_matches(out, c, want)
        wants.append(want)
    return out, wants


def test_random_cases_equal_the_restatement(lib):
    rng = np.random.default_rng(5)
    cases = mc.random_cases(rng, 6, 6, 10, density=0.15)
    out, wants = run_and_compare(lib, cases, mc.default_horizon(10, 10))
    assert any(w['status'] == 0 for w in wants)


def test_crowded_cases_with_failures(lib):
    """Dense maps and many agents: some cases end with NO_PATH, the agents after the failing one left unplanned."""
    rng = np.random.default_rng(8)
    cases = mc.random_cases(rng, 6, 10, 7, density=0.25)
    out, wants = run_and_compare(lib, cases, 20)
    assert {w['status'] for w in wants} == {0, mc.NO_PATH}


def test_agent_on_its_goal_steps_aside_and_comes_back(lib):
    grid = np.array([[1, 1, 0, 1, 1],
                     [0, 0, 0, 0, 0],
                     [1, 1, 1, 1, 1]], np.uint8)
    starts, goals = np.array([[1, 0], [1, 2]]), np.array([[1, 4], [1, 2]])
    out = call(lib, grid, starts[None], goals[None], 12)
    want = mc.solve_case(grid, starts, goals, 12)
    assert_matches(out, 0, want)
    assert want['arrival'].tolist() == [4, 3]
    assert want['schedule'][1:4, 1].tolist() == [[0, 2], [0, 2], [1, 2]]


def test_target_conflict(lib):
    grid = np.zeros((3, 7), np.uint8)
    starts, goals = np.array([[1, 0], [0, 3]]), np.array([[1, 6], [1, 3]])
    out = call(lib, grid, starts[None], goals[None], 20)
    want = mc.solve_case(grid, starts, goals, 20)
    assert_matches(out, 0, want)
    assert want['arrival'].tolist() == [6, 4]                   # not 1: agent 0 crosses the goal at t = 3


def test_swap_is_not_a_shortcut(lib):
    grid = np.zeros((2, 2), np.uint8)
    starts, goals = np.array([[0, 0], [0, 1]]), np.array([[0, 1], [0, 0]])
    out = call(lib, grid, starts[None], goals[None], 8)
    want = mc.solve_case(grid, starts, goals, 8)
    assert_matches(out, 0, want)
    assert want['arrival'].tolist() == [1, 3]                   # the swap would have taken 1 step


def test_walled_in_agent_stops_the_plan(lib):
    grid = np.zeros((6, 6), np.uint8)
    grid[3:6, 3] = 1
    grid[3, 3:6] = 1                                            # (4,4), (4,5), (5,4), (5,5) walled in
    starts = np.array([[0, 0], [5, 5], [0, 5], [2, 0]])
    goals = np.array([[1, 1], [0, 3], [2, 5], [1, 0]])
    out = call(lib, grid, starts[None], goals[None], 30)
    want = mc.solve_case(grid, starts, goals, 30)
    assert_matches(out, 0, want)
    assert want['status'] == mc.NO_PATH and want['failing'] == 1
    assert want['arrival'][2:].tolist() == [-1, -1] and (want['schedule'][:, 1:] == -1).all()
    assert out['makespan'][0] == -1 and out['flowtime'][0] == -1


def test_bad_cases_flag_only_themselves(lib):
    grid = np.zeros((5, 5), np.uint8)
    grid[2, 2] = 1
    ok_s, ok_g = np.array([[0, 0], [4, 4], [0, 4]]), np.array([[4, 0], [0, 0], [4, 4]])
    variants = []
    for k, v in (('s', [-1, 0]), ('s', [0, 5]), ('g', [5, 1]), ('g', [1, -1]), ('s', [2, 2]), ('g', [2, 2]),
                 ('s', [4, 4]), ('g', [0, 0])):
        s, g = ok_s.copy(), ok_g.copy()
        (s if k == 's' else g)[0] = v                           # off the map, on the obstacle, a duplicate
        variants.append((s, g))
    starts = np.stack([ok_s] + [s for s, _ in variants] + [ok_s, ok_s, ok_s])
    goals = np.stack([ok_g] + [g for _, g in variants] + [ok_g, ok_g, ok_g])
    C = len(starts)
    orders = np.tile(np.array([[0, 1, 2], [2, 1, 0]]), (C, 1, 1))
    orders[-3, 1] = [0, 0, 2]                                   # not a permutation
    orders[-2, 0] = [0, 1, 3]                                   # out of range
    out = call(lib, grid, starts, goals, 16, orders)
    for c in range(C):
        want = mc.solve_case(grid, starts[c], goals[c], 16, list(orders[c]))
        assert_matches(out, c, want)
        assert (want['status'] == mc.BAD_CASE) == (c not in (0, C - 1)), c
    assert out['status'][0] == 0 and out['status'][-1] == 0


@pytest.mark.parametrize('H,W', [(64, 64), (5, 64), (64, 5)])
def test_widest_and_tallest_maps(lib, H, W):
    """Bit 63 of a row and lane 63 of the wave."""
    grid = np.zeros((H, W), np.uint8)
    grid[H // 2, 1:W - 1] = 1
    starts = np.array([[0, 0], [H - 1, 0], [0, W - 1]])
    goals = np.array([[H - 1, W - 1], [0, W - 1], [H - 1, 0]])
    T = 2 * (H + W)
    out = call(lib, grid, starts[None], goals[None], T)
    want = mc.solve_case(grid, starts, goals, T)
    assert want['status'] == 0
    assert_matches(out, 0, want)


def test_non_square_random_maps(lib):
    rng = np.random.default_rng(13)
    run_and_compare(lib, mc.random_cases(rng, 3, 5, 7, 13, density=0.1), 40)
    run_and_compare(lib, mc.random_cases(rng, 3, 5, 13, 7, density=0.1), 40)


def test_restarts_pick_the_best_and_ties_the_lowest(lib):
    rng = np.random.default_rng(21)
    cases = mc.random_cases(rng, 4, 8, 8, density=0.2)
    N = 8
    orders = np.stack([np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(3)]) for _ in cases])
    orders[1, 2] = orders[1, 0]                                 # restart 2 repeats restart 0: a tie
    orders[2, 1:] = orders[2, 0]                                # every restart the same order
    out, wants = run_and_compare(lib, cases, 32, orders)
    assert wants[2]['restart'] == 0 and out['restart'][1] != 2
    # the index order fails (agent 0 parks in the corridor agent 1 must cross), the reversed order solves the case;
    # restart 2 repeats restart 1: the tie keeps restart 1
    grid = np.array([[0, 0, 0],
                     [1, 0, 1]], np.uint8)
    starts, goals = np.array([[1, 1], [0, 0]]), np.array([[0, 1], [0, 2]])
    orders = np.array([[[0, 1], [1, 0], [1, 0]]])
    out = call(lib, grid, starts[None], goals[None], 10, orders)
    want = mc.solve_case(grid, starts, goals, 10, list(orders[0]))
    assert_matches(out, 0, want)
    assert mc.plan_order(grid, starts, goals, [0, 1], 10)[0] == mc.NO_PATH
    assert want['restart'] == 1 and want['status'] == 0 and want['arrival'].tolist() == [2, 2]


def test_batched_grid_next_to_shared_grid(lib):
    rng = np.random.default_rng(34)
    grid, _, _ = mc.random_cases(rng, 1, 5, 9)[0]
    cases = []
    for _ in range(3):
        free = np.argwhere(grid == 0)
        idx = rng.choice(len(free), 10, replace=False)
        cases.append((grid, free[idx[:5]], free[idx[5:]]))
    shared, _ = run_and_compare(lib, cases, 36, batched=False)
    batched, _ = run_and_compare(lib, cases, 36, batched=True)
    for k in shared:
        assert np.array_equal(shared[k], batched[k]), k


def test_argument_errors(lib):
    grid = np.zeros((4, 4), np.uint8)
    s, g = np.array([[[0, 0], [1, 1]]]), np.array([[[3, 3], [2, 2]]])
    call(lib, grid, s, g, 8)
    for kw in (dict(T=-1), dict(T=1025), dict(orders=None, ws_bytes=0)):
        out = call(lib, grid, s, g, kw.pop('T', 8), expect=ERR_ARG, **kw)
        assert (out['status'] == POISON).all()                 # nothing enqueued
    big = np.zeros((65, 4), np.uint8)
    out = call(lib, big, s, g, 8, expect=ERR_UNSUPPORTED)
    assert (out['status'] == POISON).all() and (out['schedule'] == POISON).all()
    many = np.zeros((1, 129, 2), np.int32)
    call(lib, np.zeros((64, 64), np.uint8), many, many, 4, expect=ERR_ARG)
    assert lib.gnnpp_mapf_solve(None, None) == ERR_ARG
    assert lib.gnnpp_mapf_solve(ctypes.byref(Mapf()), None) == ERR_ARG
    assert lib.gnnpp_mapf_workspace_bytes(1, 1, 65, 8) == 0 and lib.gnnpp_mapf_workspace_bytes(1, 1, 4, 8) > 0
