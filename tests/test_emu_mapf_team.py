"""CPU: gnnpp_mapf_team_solve (csrc/mapf_team_kernels.hip), compiled unmodified for the host emulation, against the
sequential numpy restatement of the contract (tests/mapf_cases.py): equality of every output element.  The shapes are
small (a lane-accurate workgroup is slow) but cross every boundary of the layout: teams beyond 128 agents, rows of two
and three words (W = 65, 128, 129), more than one wave of rows (H = 65 .. 70), and the one-wave call's own sizes, where
the two entry points must write the same bytes."""
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
KEYS = ('status', 'restart', 'makespan', 'flowtime', 'failing', 'arrival', 'schedule')


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
    for f in (L.gnnpp_mapf_solve, L.gnnpp_mapf_team_solve):
        f.argtypes = [ctypes.POINTER(Mapf), ctypes.c_void_p]
        f.restype = ctypes.c_int
    L.gnnpp_mapf_workspace_bytes.argtypes = [ctypes.c_int] * 4
    L.gnnpp_mapf_workspace_bytes.restype = ctypes.c_size_t
    L.gnnpp_mapf_team_workspace_bytes.argtypes = [ctypes.c_int] * 5
    L.gnnpp_mapf_team_workspace_bytes.restype = ctypes.c_size_t
    return L


def one_slot_bytes(lib, C, R, H, W, T):
    """The summary and exactly one slot: the smallest workspace the call accepts."""
    slot = (T + 1) * 6 * H * ((W + 63) // 64) * 8
    full = lib.gnnpp_mapf_team_workspace_bytes(C, R, H, W, T)
    return full - (min(C * R, 256) - 1) * slot


def call(lib, grids, starts, goals, T, orders=None, expect=0, ws_bytes=None, team=True, poison_ws=False):
    """One call on host arrays; outputs start out poisoned, so an element the call does not write cannot pass for one
    it wrote.  ws_bytes: what the call is told (the buffer is never smaller than that)."""
    grid = np.ascontiguousarray(grids, dtype=np.uint8)
    start = np.ascontiguousarray(starts, dtype=np.int32)
    goal = np.ascontiguousarray(goals, dtype=np.int32)
    C, N = start.shape[:2]
    order = None if orders is None else np.ascontiguousarray(orders, dtype=np.int32)
    R = 1 if order is None else order.shape[1]
    H, W = grid.shape[-2:]
    if team:
        need = lib.gnnpp_mapf_team_workspace_bytes(C, R, min(H, 256), min(W, 256), max(0, min(T, 2048)))
    else:
        need = lib.gnnpp_mapf_workspace_bytes(C, R, H, T)
    told = need if ws_bytes is None else ws_bytes
    ws = np.full(max(need, told, 8) // 8 + 1, 0x5a5a5a5a5a5a5a5a if poison_ws else 0, np.uint64)
    out = {'schedule': np.full((C, T + 1 if T >= 0 else 1, N, 2), POISON, np.int32),
           'arrival': np.full((C, N), POISON, np.int32)}
    for k in ('makespan', 'flowtime', 'status', 'failing', 'restart'):
        out[k] = np.full(C, POISON, np.int32)
    m = Mapf()
    m.grid, m.grid_batched, m.start, m.goal = grid.ctypes.data, int(grid.ndim == 3), start.ctypes.data, goal.ctypes.data
    m.order = order.ctypes.data if order is not None else None
    m.C, m.N, m.H, m.W, m.R, m.T_max = C, N, H, W, R, T
    for k in out:
        setattr(m, k, out[k].ctypes.data)
    m.workspace, m.workspace_bytes = ws.ctypes.data, told
    fn = lib.gnnpp_mapf_team_solve if team else lib.gnnpp_mapf_solve
    assert fn(ctypes.byref(m), None) == expect
    return out


def assert_matches(out, c, want):
    for k in ('status', 'restart', 'makespan', 'flowtime', 'failing'):
        assert int(out[k][c]) == want[k], (k, int(out[k][c]), want[k])
    assert np.array_equal(out['arrival'][c], want['arrival'])
    assert np.array_equal(out['schedule'][c], want['schedule'])


def run_and_compare(lib, cases, T, orders=None, batched=True, **kw):
    """cases: [(grid, starts, goals)] of one map size; every output of every case equal to the yardstick's."""
    grids = np.stack([g for g, _, _ in cases]) if batched else cases[0][0]
    out = call(lib, grids, np.stack([s for _, s, _ in cases]), np.stack([g for _, _, g in cases]), T, orders, **kw)
    wants = []
    for c, (g, s, gl) in enumerate(cases):
        want = mc.solve_case(g, s, gl, T, None if orders is None else list(orders[c]))
        assert_matches(out, c, want)
        wants.append(want)
    return out, wants


def assert_same_bytes(a, b):
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_more_than_128_agents_on_one_word_rows(lib):
    """129 agents on 20 x 20: an open map where all of them are planned, and one with obstacles where a late agent
    finds no path (more than 128 agents have been looked at by then or not: both are the yardstick's answer)."""
    cases = mc.random_cases(np.random.default_rng(40), 1, 129, 20, density=0.0) + \
        mc.random_cases(np.random.default_rng(41), 1, 129, 20, density=0.1)
    out, wants = run_and_compare(lib, cases, mc.default_horizon(20, 20), poison_ws=True)
    assert wants[0]['status'] == 0 and (wants[0]['arrival'] >= 0).all()
    assert wants[1]['status'] == mc.NO_PATH and wants[1]['failing'] > 64


@pytest.mark.parametrize('W', [65, 128, 129])
def test_random_cases_on_rows_of_several_words(lib, W):
    rng = np.random.default_rng(100 + W)
    cases = mc.random_cases(rng, 2, 12, 5, W, density=0.1)
    out, wants = run_and_compare(lib, cases, 2 * (5 + W), poison_ws=True)
    assert any(w['status'] == 0 for w in wants)
    if W >= 128:                                                # (W = 65: one column beyond the boundary; the corridor
        crossed = False                                         # test below forces the crossing there)
        for w, (_, s, g) in zip(wants, cases):
            n = int((w['arrival'] >= 0).sum())                  # the planned agents: some go right, some left
            crossed |= bool(((s[:n, 1] // 64) < (g[:n, 1] // 64)).any() and ((s[:n, 1] // 64) > (g[:n, 1] // 64)).any())
        assert crossed


@pytest.mark.parametrize('W', [65, 128, 129])
def test_corridor_forces_the_crossing_both_ways(lib, W):
    """Five rows; the middle one is a wall with two doors, one on each side of the last word boundary b (columns
    b - 1 and b).  Agent 0 goes from the top left to the bottom right corner, agent 1 from the top right to the bottom
    left: both must pass the boundary column, in opposite directions, whichever door they take.  For W = 65 and 129
    column b is the last word's only valid bit."""
    b = 64 if W < 129 else 128
    grid = np.zeros((5, W), np.uint8)
    grid[2, :] = 1
    grid[2, b - 1:b + 1] = 0
    starts = np.array([[0, 0], [0, W - 1], [1, 10], [4, 5]])
    goals = np.array([[4, W - 1], [4, 0], [0, W - 2], [0, 3]])
    T = 4 * W
    out = call(lib, grid, starts[None], goals[None], T, poison_ws=True)
    want = mc.solve_case(grid, starts, goals, T)
    assert want['status'] == 0
    assert_matches(out, 0, want)
    for n, step in ((0, 1), (1, -1)):
        cols = want['schedule'][:want['arrival'][n] + 1, n, 1]
        k = int(np.nonzero(cols == (b if step > 0 else b - 1))[0][0])
        assert cols[k - 1] == cols[k] - step                    # entered the boundary column from the other word


def test_swap_refused_across_the_word_boundary(lib):
    """Agents in columns 63 and 64 want each other's cell.  The swap over the boundary is no move: on a 2 x 2 block of
    free cells astride the boundary the second agent goes round (the 2 x 2 case of the one-wave tests, shifted)."""
    grid = np.ones((2, 66), np.uint8)
    grid[0:2, 63:65] = 0
    starts, goals = np.array([[0, 63], [0, 64]]), np.array([[0, 64], [0, 63]])
    out = call(lib, grid, starts[None], goals[None], 12)
    want = mc.solve_case(grid, starts, goals, 12)
    assert_matches(out, 0, want)
    assert want['status'] == 0 and want['arrival'].tolist() == [1, 3]      # the swap would have taken 1 step
    # with those two cells alone there is no way round: NO_PATH for agent 1, not a swap
    grid2 = np.ones((1, 66), np.uint8)
    grid2[0, 63:65] = 0
    out = call(lib, grid2, starts[None], goals[None], 12)
    want = mc.solve_case(grid2, starts, goals, 12)
    assert_matches(out, 0, want)
    assert want['status'] == mc.NO_PATH and want['failing'] == 1


@pytest.mark.parametrize('H,W', [(65, 6), (70, 9), (66, 65)])
def test_more_than_one_wave_of_rows(lib, H, W):
    """The vertical exchange across waves: a wall with one door between rows 63 and 64."""
    grid = np.zeros((H, W), np.uint8)
    grid[63, :] = 1
    grid[63, W // 2] = 0
    starts = np.array([[0, 0], [H - 1, 0], [0, W - 1], [H - 1, W - 1]])
    goals = np.array([[H - 1, W - 1], [0, W - 1], [H - 1, 0], [1, 1]])
    T = 2 * (H + W)
    out = call(lib, grid, starts[None], goals[None], T, poison_ws=True)
    want = mc.solve_case(grid, starts, goals, T)
    assert want['status'] == 0
    assert_matches(out, 0, want)


def test_random_cases_on_tall_maps(lib):
    rng = np.random.default_rng(67)
    run_and_compare(lib, mc.random_cases(rng, 2, 10, 67, 7, density=0.1), 2 * (67 + 7))


def test_several_waves_of_rows_of_several_words(lib):
    """70 x 130: 210 threads in four waves, rows of three words, 140 agents."""
    cases = mc.random_cases(np.random.default_rng(70130), 1, 140, 70, 130, density=0.1)
    out, wants = run_and_compare(lib, cases, 200, poison_ws=True)
    assert (wants[0]['arrival'] >= 0).sum() > 128


def test_given_orders_with_a_failing_restart(lib):
    rng = np.random.default_rng(21)
    cases = mc.random_cases(rng, 3, 8, 6, 70, density=0.15)
    N = 8
    orders = np.stack([np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(2)]) for _ in cases])
    orders[1, 2] = orders[1, 0]                                 # a tie: the lower index wins
    run_and_compare(lib, cases, 160, orders)
    # the index order fails (agent 0 parks in the corridor agent 1 must cross), the reversed order solves the case
    grid = np.ones((2, 67), np.uint8)
    grid[0, 63:66] = 0
    grid[1, 64] = 0
    starts, goals = np.array([[1, 64], [0, 63]]), np.array([[0, 64], [0, 65]])
    orders = np.array([[[0, 1], [1, 0], [1, 0]]])
    out = call(lib, grid, starts[None], goals[None], 10, orders)
    want = mc.solve_case(grid, starts, goals, 10, list(orders[0]))
    assert_matches(out, 0, want)
    assert mc.plan_order(grid, starts, goals, [0, 1], 10)[0] == mc.NO_PATH
    assert want['restart'] == 1 and want['status'] == 0 and want['arrival'].tolist() == [2, 2]


def test_crowded_cases_solved_and_failing(lib):
    rng = np.random.default_rng(8)
    cases = mc.random_cases(rng, 6, 10, 5, 66, density=0.2)
    out, wants = run_and_compare(lib, cases, 60)
    assert {w['status'] for w in wants} == {0, mc.NO_PATH}


def test_bad_cases_flag_only_themselves(lib):
    grid = np.zeros((5, 70), np.uint8)
    grid[2, 66] = 1
    ok_s, ok_g = np.array([[0, 0], [4, 69], [0, 68]]), np.array([[4, 0], [0, 0], [4, 69]])
    variants = []
    for k, v in (('s', [-1, 0]), ('s', [0, 70]), ('g', [5, 1]), ('g', [1, -1]), ('s', [2, 66]), ('g', [2, 66]),
                 ('s', [4, 69]), ('g', [0, 0]), ('s', [0, 100]), ('g', [3, 127])):
        s, g = ok_s.copy(), ok_g.copy()
        (s if k == 's' else g)[0] = v                           # off the map, on the obstacle, a duplicate
        variants.append((s, g))
    starts = np.stack([ok_s] + [s for s, _ in variants] + [ok_s, ok_s, ok_s])
    goals = np.stack([ok_g] + [g for _, g in variants] + [ok_g, ok_g, ok_g])
    C = len(starts)
    orders = np.tile(np.array([[0, 1, 2], [2, 1, 0]]), (C, 1, 1))
    orders[-3, 1] = [0, 0, 2]                                   # not a permutation
    orders[-2, 0] = [0, 1, 3]                                   # out of range
    out = call(lib, grid, starts, goals, 160, orders)
    for c in range(C):
        want = mc.solve_case(grid, starts[c], goals[c], 160, list(orders[c]))
        assert_matches(out, c, want)
        assert (want['status'] == mc.BAD_CASE) == (c not in (0, C - 1)), c
    assert out['status'][0] == 0 and out['status'][-1] == 0


def test_batched_grid_next_to_shared_grid(lib):
    rng = np.random.default_rng(34)
    grid, _, _ = mc.random_cases(rng, 1, 5, 4, 66)[0]
    cases = []
    for _ in range(3):
        free = np.argwhere(grid == 0)
        idx = rng.choice(len(free), 10, replace=False)
        cases.append((grid, free[idx[:5]], free[idx[5:]]))
    shared, _ = run_and_compare(lib, cases, 140, batched=False)
    batched, _ = run_and_compare(lib, cases, 140, batched=True)
    assert_same_bytes(shared, batched)


def _both(lib, grids, starts, goals, T, orders=None):
    a = call(lib, grids, starts, goals, T, orders, team=False)
    b = call(lib, grids, starts, goals, T, orders, team=True, poison_ws=True)
    assert_same_bytes(a, b)
    return a


def test_same_bytes_as_the_one_wave_call(lib):
    """Every case both entry points accept: all outputs byte-equal (random, crowded with failures, restarts with a bad
    order, the widest one-word map)."""
    rng = np.random.default_rng(5)
    cases = mc.random_cases(rng, 4, 6, 10, density=0.15)
    _both(lib, np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases]), 40)
    rng = np.random.default_rng(8)
    cases = mc.random_cases(rng, 6, 10, 7, density=0.25)
    out = _both(lib, np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases]), 20)
    assert set(out['status'].tolist()) == {0, mc.NO_PATH}
    rng = np.random.default_rng(21)
    cases = mc.random_cases(rng, 3, 8, 8, density=0.2)
    orders = np.stack([np.stack([np.arange(8)] + [rng.permutation(8) for _ in range(2)]) for _ in cases])
    orders[2, 1] = [0, 0, 1, 2, 3, 4, 5, 6]
    out = _both(lib, np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases]), 32,
                orders)
    assert out['status'][2] == mc.BAD_CASE
    grid = np.zeros((64, 64), np.uint8)
    grid[32, 1:63] = 1
    starts = np.array([[[0, 0], [63, 0], [0, 63]]])
    goals = np.array([[[63, 63], [0, 63], [63, 0]]])
    out = _both(lib, grid, starts, goals, 256)
    assert out['status'][0] == 0
    cases = mc.random_cases(np.random.default_rng(77), 1, 128, 16, density=0.05)
    _both(lib, cases[0][0], cases[0][1][None], cases[0][2][None], 64)


def test_outputs_do_not_depend_on_the_slot_count(lib):
    rng = np.random.default_rng(55)
    cases = mc.random_cases(rng, 5, 6, 4, 66, density=0.15)
    N = 6
    orders = np.stack([np.stack([np.arange(N), rng.permutation(N)]) for _ in cases])
    grids, starts, goals = (np.stack([c[k] for c in cases]) for k in range(3))
    full = call(lib, grids, starts, goals, 60, orders, poison_ws=True)
    one = one_slot_bytes(lib, 5, 2, 4, 66, 60)
    assert one < lib.gnnpp_mapf_team_workspace_bytes(5, 2, 4, 66, 60)
    single = call(lib, grids, starts, goals, 60, orders, ws_bytes=one, poison_ws=True)
    three = call(lib, grids, starts, goals, 60, orders, ws_bytes=one + 2 * (61 * 6 * 4 * 2 * 8) + 100, poison_ws=True)
    assert_same_bytes(full, single)
    assert_same_bytes(full, three)
    for c, (g, s, gl) in enumerate(cases):
        assert_matches(single, c, mc.solve_case(g, s, gl, 60, list(orders[c])))


def test_zero_horizon_and_single_agent(lib):
    grid = np.zeros((2, 65), np.uint8)
    s, g = np.array([[[0, 64]]]), np.array([[[0, 64]]])
    out = call(lib, grid, s, g, 0)
    assert_matches(out, 0, mc.solve_case(grid, s[0], g[0], 0))
    assert out['status'][0] == 0 and out['arrival'][0, 0] == 0
    g2 = np.array([[[1, 64]]])
    out = call(lib, grid, s, g2, 0)
    assert_matches(out, 0, mc.solve_case(grid, s[0], g2[0], 0))
    assert out['status'][0] == mc.NO_PATH


def test_argument_errors(lib):
    grid = np.zeros((4, 4), np.uint8)
    s, g = np.array([[[0, 0], [1, 1]]]), np.array([[[3, 3], [2, 2]]])
    assert call(lib, grid, s, g, 8)['status'][0] == 0
    one = one_slot_bytes(lib, 1, 1, 4, 4, 8)
    for kw in (dict(T=-1), dict(T=2049), dict(ws_bytes=0), dict(ws_bytes=one - 1)):
        out = call(lib, grid, s, g, kw.pop('T', 8), expect=ERR_ARG, **kw)
        for k in KEYS:
            assert (out[k] == POISON).all(), k                  # nothing enqueued
    for shape in ((257, 4), (4, 257)):
        out = call(lib, np.zeros(shape, np.uint8), s, g, 8, expect=ERR_UNSUPPORTED)
        for k in KEYS:
            assert (out[k] == POISON).all(), k
    many = np.zeros((1, 1025, 2), np.int32)
    out = call(lib, np.zeros((64, 64), np.uint8), many, many, 4, expect=ERR_ARG)
    assert (out['status'] == POISON).all() and (out['schedule'] == POISON).all()
    # N and T_max are refused before the map size is looked at
    call(lib, np.zeros((257, 4), np.uint8), many, many, 4, expect=ERR_ARG)
    call(lib, np.zeros((257, 4), np.uint8), s, g, 2049, expect=ERR_ARG)
    # orders without R, NULLs
    assert lib.gnnpp_mapf_team_solve(None, None) == ERR_ARG
    assert lib.gnnpp_mapf_team_solve(ctypes.byref(Mapf()), None) == ERR_ARG
    W = lib.gnnpp_mapf_team_workspace_bytes
    assert W(1, 1, 4, 4, 8) > 0 and W(1, 1, 256, 256, 2048) > 0
    for bad in ((0, 1, 4, 4, 8), (1, 0, 4, 4, 8), (1, 1, 257, 4, 8), (1, 1, 4, 257, 8), (1, 1, 0, 4, 8), (1, 1, 4, 0, 8),
                (1, 1, 4, 4, -1), (1, 1, 4, 4, 2049), (1 << 20, 1 << 12, 4, 4, 8)):
        assert W(*bad) == 0, bad
    # the full size is for min(C R, 256) slots
    slot = 9 * 6 * 4 * 8
    assert W(300, 1, 4, 4, 8) - W(256, 1, 4, 4, 8) == (300 * 16 + 255) // 256 * 256 - 256 * 16
    assert W(2, 1, 4, 4, 8) - W(1, 1, 4, 4, 8) == slot
