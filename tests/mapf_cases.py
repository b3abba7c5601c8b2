"""Yardstick of the device MAPF solver (csrc/mapf_kernels.hip, gnn_pathplanning_amd/mapf.py): a SEQUENTIAL numpy
restatement of the prioritized-planning contract of include/gnnpp.h (gnnpp_mapf), and two independent checks of it:

  bfs_arrival      a plain (cell, t) breadth-first search with a queue, given the earlier agents' actual paths: the
                   smallest arrival an agent can have (or None), to confirm each a_i is the minimum and each failure
                   genuine;
  check_plans      a validator for moves, obstacles, vertex, swap and parking conflicts, and replay_through_simulator:
                   the schedule played through the reference simulator (oracle.rollout_oracle.move_step), which must
                   flag no collision and reproduce every position.

The second half holds the solver's cases themselves (ONE_WAVE, TEAM, BOTH): each hand-built or seeded call is built
once here, with the facts the yardstick's answer must show, and is run under the host emulation
(tests/test_emu_mapf.py, tests/test_emu_mapf_team.py) and on the device (tests/test_gpu_mapf_cases.py).
"""
from collections import deque

import numpy as np

from oracle import rollout_oracle as ro

MOVES = ((-1, 0), (0, -1), (1, 0), (0, 1))            # up, left, down, right (the reference's DELTA without stop)
NO_PATH, BAD_CASE = 1, 2


def default_horizon(H, W):
    return 4 * (H + W)


def valid_case(grid, starts, goals, order):
    H, W = grid.shape
    N = len(starts)
    for p in list(starts) + list(goals):
        if not (0 <= p[0] < H and 0 <= p[1] < W) or grid[p[0], p[1]] != 0:
            return False
    if len({tuple(map(int, p)) for p in starts}) != N or len({tuple(map(int, p)) for p in goals}) != N:
        return False
    return sorted(int(i) for i in order) == list(range(N))


def plan_order(grid, starts, goals, order, T):
    """One restart.  (status, arrival [N] (-1 unplanned), {agent: path [a+1,2]}, failing agent or -1)."""
    grid = np.asarray(grid)
    starts, goals = np.asarray(starts, dtype=np.int64), np.asarray(goals, dtype=np.int64)
    H, W = grid.shape
    N = len(starts)
    free = grid == 0
    occ = np.zeros((T + 1, H, W), bool)
    mv = np.zeros((T + 1, 4, H, W), bool)              # mv[t, e]: the occupant of the cell at t moves by MOVES[e]
    arrival = np.full(N, -1, dtype=np.int64)
    paths = {}
    for i in order:
        (sx, sy), (gx, gy) = starts[i], goals[i]
        hits = np.nonzero(occ[:, gx, gy])[0]
        tmin = int(hits[-1]) + 1 if len(hits) else 0
        layers = [np.zeros((H, W), bool)]
        layers[0][sx, sy] = True
        a = 0 if tmin <= 0 and (sx, sy) == (gx, gy) else -1
        t = 0
        while a < 0 and tmin <= T and t < T:
            R, Rn = layers[t], layers[t].copy()
            Rn[:-1] |= R[1:] & ~mv[t, 2, :-1]           # up from the row below (a swap when the occupant moves down)
            Rn[:, :-1] |= R[:, 1:] & ~mv[t, 3, :, :-1]  # left from the column to the right
            Rn[1:] |= R[:-1] & ~mv[t, 0, 1:]            # down from the row above
            Rn[:, 1:] |= R[:, :-1] & ~mv[t, 1, :, 1:]   # right from the column to the left
            Rn &= free & ~occ[t + 1]
            layers.append(Rn)
            t += 1
            if t >= tmin and Rn[gx, gy]:
                a = t
            if not Rn.any():
                break
        if a < 0:
            return NO_PATH, arrival, paths, int(i)
        path = [(gx, gy)]
        cx, cy = gx, gy
        for t in range(a, 0, -1):
            L = layers[t - 1]
            if L[cx, cy]:
                pass
            elif cx + 1 < H and L[cx + 1, cy] and not mv[t - 1, 2, cx, cy]:
                cx += 1
            elif cy + 1 < W and L[cx, cy + 1] and not mv[t - 1, 3, cx, cy]:
                cy += 1
            elif cx > 0 and L[cx - 1, cy] and not mv[t - 1, 0, cx, cy]:
                cx -= 1
            elif cy > 0 and L[cx, cy - 1] and not mv[t - 1, 1, cx, cy]:
                cy -= 1
            else:
                raise AssertionError('walk back found no predecessor')
            path.append((cx, cy))
        path = np.array(path[::-1], dtype=np.int64)
        for t in range(T + 1):
            x, y = path[t] if t <= a else (gx, gy)
            occ[t, x, y] = True
            if t < a and tuple(path[t + 1]) != (x, y):
                mv[t, MOVES.index((int(path[t + 1][0] - x), int(path[t + 1][1] - y))), x, y] = True
        arrival[i] = a
        paths[int(i)] = path
    return 0, arrival, paths, -1


def solve_case(grid, starts, goals, T, orders=None):
    """The call's outputs for one case: dict(status, restart, makespan, flowtime, failing, arrival [N],
    schedule [T+1,N,2]).  orders: list of R planning orders (default: the index order)."""
    N = len(starts)
    orders = [np.arange(N)] if orders is None else [np.asarray(o) for o in orders]
    bad = {'status': BAD_CASE, 'restart': -1, 'makespan': -1, 'flowtime': -1, 'failing': -1,
           'arrival': np.full(N, -1, dtype=np.int64), 'schedule': np.full((T + 1, N, 2), -1, dtype=np.int64)}
    if not all(valid_case(np.asarray(grid), starts, goals, o) for o in orders):
        return bad
    best, best_key = None, None
    for r, o in enumerate(orders):
        st, arr, paths, fail = plan_order(grid, starts, goals, o, T)
        key = (0, int(arr.sum()), int(arr.max())) if st == 0 else (1, -1, -1)
        if best is None or key < best_key:
            best, best_key = (r, st, arr, paths, fail), key
    r, st, arr, paths, fail = best
    sched = np.full((T + 1, N, 2), -1, dtype=np.int64)
    for n, p in paths.items():
        sched[:len(p), n] = p
        sched[len(p):, n] = p[-1]
    return {'status': st, 'restart': r, 'makespan': best_key[2], 'flowtime': best_key[1],
            'failing': fail, 'arrival': arr, 'schedule': sched}


# ---- independent checks ------------------------------------------------------------------------------------
def bfs_arrival(grid, start, goal, earlier, T):
    """Smallest a <= T such that the agent can be on its goal at a and stay there until T, moving from `start` at 0
    against the earlier agents' position arrays `earlier` ([T+1,2] each): no cell of theirs at t >= 1, no swap.
    None when there is none.  A plain queue over (cell, t)."""
    H, W = grid.shape
    at = [dict() for _ in range(T + 1)]                 # t -> {cell: position array of the agent there}
    for p in earlier:
        for t in range(T + 1):
            at[t][(int(p[t][0]), int(p[t][1]))] = p
    goal = (int(goal[0]), int(goal[1]))
    last = max([t for t in range(T + 1) if goal in at[t]], default=-1)
    q = deque([((int(start[0]), int(start[1])), 0)])
    seen = {q[0]}
    while q:
        cell, t = q.popleft()
        if cell == goal and t > last:
            return t
        if t == T:
            continue
        for d in MOVES + ((0, 0),):
            nxt = (cell[0] + d[0], cell[1] + d[1])
            if not (0 <= nxt[0] < H and 0 <= nxt[1] < W) or grid[nxt] != 0 or nxt in at[t + 1]:
                continue
            other = at[t].get(nxt)
            if d != (0, 0) and other is not None and tuple(other[t + 1]) == cell:
                continue                                # a swap with an earlier agent
            if (nxt, t + 1) not in seen:
                seen.add((nxt, t + 1))
                q.append((nxt, t + 1))
    return None


def check_plans(grid, starts, goals, schedule, arrival):
    """Validator of a solved schedule [T,N,2]: starts, goals, parking, the five moves, obstacles, vertex and swap
    conflicts.  Raises AssertionError."""
    grid = np.asarray(grid)
    H, W = grid.shape
    sched = np.asarray(schedule)
    T, N = sched.shape[:2]
    assert np.array_equal(sched[0], starts)
    for n in range(N):
        assert (sched[arrival[n]:, n] == goals[n]).all(), 'agent %d does not park on its goal' % n
    for t in range(T):
        cells = {tuple(p) for p in sched[t]}
        assert len(cells) == N, 'vertex conflict at t = %d' % t
        for n in range(N):
            x, y = sched[t, n]
            assert 0 <= x < H and 0 <= y < W and grid[x, y] == 0
            if t + 1 < T:
                d = tuple(int(v) for v in sched[t + 1, n] - sched[t, n])
                assert d in MOVES + ((0, 0),), 'agent %d jumps at t = %d' % (n, t)
                for m in range(N):
                    assert m == n or not (tuple(sched[t, m]) == tuple(sched[t + 1, n]) and
                                          tuple(sched[t + 1, m]) == tuple(sched[t, n]) and d != (0, 0)), \
                        'swap of agents %d and %d at t = %d' % (n, m, t)


def actions_of(schedule):
    """[T-1,N] action ids (index into oracle.rollout_oracle.DELTA) of consecutive states."""
    d = np.diff(np.asarray(schedule), axis=0)
    out = np.full(d.shape[:2], 4, dtype=np.int64)
    for k, (dx, dy) in enumerate(MOVES):
        out[(d[..., 0] == dx) & (d[..., 1] == dy)] = k
    return out


def replay_through_simulator(grid, goals, schedule):
    """Every step of the schedule through the reference simulator's move(): no collision flag, the same positions."""
    sched = np.asarray(schedule)
    ep = ro.EpisodeState(grid, goals, sched[0], maxstep=10 ** 6)
    for t, act in enumerate(actions_of(sched)):
        _, move_col, pred_col = ro.move_step(ep, act, t + 1, lambda agents: agents[0])
        assert not move_col and not pred_col, 'collision flagged at step %d' % (t + 1)
        assert np.array_equal(ep.cur, sched[t + 1]), 'positions differ after step %d' % (t + 1)


def random_cases(rng, count, N, H, W=None, density=0.1):
    """[(grid, starts, goals)] on tests/expert_cases.random_map: distinct free starts and goals."""
    import expert_cases as ec
    return [ec.random_map(rng, N, H, W or H, density) for _ in range(count)]


# ---- the solver's cases: defined once, run under the host emulation and on the device ----------------------
# A case is one solver call: dict(name, grid [H,W] (shared by the call's cases) or [C,H,W], starts / goals [C,N,2],
# T, orders None | [C,R,N], facts, structured, poison_ws).  facts(wants) asserts what the yardstick must answer for the
# case to be the edge case its name says; structured cases are hand-built, and what the solver returns for a solved one
# also goes through check_plans and replay_through_simulator; poison_ws: the call gets a workspace full of 0x5a bytes.
POISON = -7                                             # what every output element holds before a call
ONE_WAVE, TEAM, BOTH = {}, {}, {}                       # name -> builder (gnnpp_mapf_solve, _team_solve, both)


def make_case(name, grid, starts, goals, T, orders=None, facts=None, structured=False, poison_ws=False):
    starts, goals = np.asarray(starts), np.asarray(goals)
    if starts.ndim == 2:
        starts, goals = starts[None], goals[None]
    return {'name': name, 'grid': np.asarray(grid, np.uint8), 'starts': starts, 'goals': goals, 'T': int(T),
            'orders': None if orders is None else np.asarray(orders), 'facts': facts, 'structured': structured,
            'poison_ws': poison_ws}


def case_of_list(name, cases, T, **kw):
    """One call of [(grid, starts, goals)] of one map size, a map per case."""
    return make_case(name, np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]),
                     np.stack([c[2] for c in cases]), T, **kw)


def case_inputs(case, c):
    grid = case['grid']
    return grid if grid.ndim == 2 else grid[c], case['starts'][c], case['goals'][c]


_WANTS = {}


def wants_of(case):
    """The yardstick's outputs of every case of the call (computed once per case name), its facts asserted."""
    if case['name'] not in _WANTS:
        orders = case['orders']
        wants = [solve_case(*case_inputs(case, c), case['T'], None if orders is None else list(orders[c]))
                 for c in range(len(case['starts']))]
        if case['facts'] is not None:
            case['facts'](wants)
        _WANTS[case['name']] = wants
    return _WANTS[case['name']]


def assert_outputs_equal(out, wants):
    """out: host arrays schedule [C,T+1,N,2], arrival [C,N], makespan / flowtime / status / failing / restart [C]."""
    for c, want in enumerate(wants):
        for k in ('status', 'restart', 'makespan', 'flowtime', 'failing'):
            assert int(out[k][c]) == want[k], (c, k, int(out[k][c]), want[k])
        assert np.array_equal(out['arrival'][c], want['arrival']), c
        assert np.array_equal(out['schedule'][c], want['schedule']), c


def check_solved_plans(case, out):
    """Every solved case of the call: the returned schedule through the validator and the reference simulator."""
    for c in range(len(case['starts'])):
        if int(out['status'][c]) == 0:
            grid, starts, goals = case_inputs(case, c)
            sched = np.asarray(out['schedule'][c][:int(out['makespan'][c]) + 1], dtype=np.int64)
            check_plans(grid, starts, goals, sched, np.asarray(out['arrival'][c]))
            replay_through_simulator(grid, goals, sched)


def _case(registry, name=None):
    def register(fn):
        registry[name or fn.__name__] = fn
        return fn
    return register


def _every(registry, stem, params, label):
    """One registry entry per parameter tuple of a builder fn(name, *params)."""
    def register(fn):
        for p in params:
            name = '%s_%s' % (stem, label % p)
            registry[name] = (lambda name=name, p=p: fn(name, *p))
        return fn
    return register


def _status_set(expected):
    def facts(wants):
        assert {w['status'] for w in wants} == expected
    return facts


def _any_solved(wants):
    assert any(w['status'] == 0 for w in wants)


def _all_solved(wants):
    assert all(w['status'] == 0 for w in wants)


def _bad_case_variants(grid, ok_s, ok_g, variants, T, name):
    """Case 0 and the last are legal; between them one illegal start / goal each (off the map, on the obstacle, a
    duplicate) and two illegal orders (not a permutation, out of range).  Decided in the kernel, case by case."""
    made = []
    for k, v in variants:
        s, g = ok_s.copy(), ok_g.copy()
        (s if k == 's' else g)[0] = v
        made.append((s, g))
    starts = np.stack([ok_s] + [s for s, _ in made] + [ok_s, ok_s, ok_s])
    goals = np.stack([ok_g] + [g for _, g in made] + [ok_g, ok_g, ok_g])
    C = len(starts)
    orders = np.tile(np.array([[0, 1, 2], [2, 1, 0]]), (C, 1, 1))
    orders[-3, 1] = [0, 0, 2]                                   # not a permutation
    orders[-2, 0] = [0, 1, 3]                                   # out of range

    def facts(wants):
        for c, w in enumerate(wants):
            assert (w['status'] == BAD_CASE) == (c not in (0, C - 1)), c
        assert wants[0]['status'] == 0 and wants[-1]['status'] == 0
    return make_case(name, grid, starts, goals, T, orders, facts)


def _reversed_order_case(name, grid, starts, goals):
    """The index order fails (agent 0 parks in the corridor agent 1 must cross), the reversed order solves the case;
    restart 2 repeats restart 1: the tie keeps restart 1."""
    orders = np.array([[[0, 1], [1, 0], [1, 0]]])

    def facts(wants):
        assert plan_order(grid, starts, goals, [0, 1], 10)[0] == NO_PATH
        assert wants[0]['restart'] == 1 and wants[0]['status'] == 0 and wants[0]['arrival'].tolist() == [2, 2]
    return make_case(name, grid, starts, goals, 10, orders, facts, structured=True)


def _same_grid_cases(rng, grid, count, N):
    cases = []
    for _ in range(count):
        free = np.argwhere(grid == 0)
        idx = rng.choice(len(free), 2 * N, replace=False)
        cases.append((grid, free[idx[:N]], free[idx[N:]]))
    return cases


# -- gnnpp_mapf_solve: one wave per case, maps of up to 64 x 64 -------------------------------------------------
@_case(ONE_WAVE)
def random_10x10():
    return case_of_list('random_10x10', random_cases(np.random.default_rng(5), 6, 6, 10, density=0.15),
                        default_horizon(10, 10), facts=_any_solved)


@_case(ONE_WAVE)
def crowded_cases_with_failures():
    """Dense maps and many agents: some cases end with NO_PATH, the agents after the failing one left unplanned."""
    return case_of_list('crowded_cases_with_failures', random_cases(np.random.default_rng(8), 6, 10, 7, density=0.25),
                        20, facts=_status_set({0, NO_PATH}))


@_case(ONE_WAVE)
def agent_on_its_goal_steps_aside_and_comes_back():
    grid = np.array([[1, 1, 0, 1, 1],
                     [0, 0, 0, 0, 0],
                     [1, 1, 1, 1, 1]], np.uint8)

    def facts(wants):
        assert wants[0]['arrival'].tolist() == [4, 3]
        assert wants[0]['schedule'][1:4, 1].tolist() == [[0, 2], [0, 2], [1, 2]]
    return make_case('agent_on_its_goal_steps_aside_and_comes_back', grid, [[1, 0], [1, 2]], [[1, 4], [1, 2]], 12,
                     facts=facts, structured=True)


@_case(ONE_WAVE)
def target_conflict():
    def facts(wants):
        assert wants[0]['arrival'].tolist() == [6, 4]           # not 1: agent 0 crosses the goal at t = 3
    return make_case('target_conflict', np.zeros((3, 7), np.uint8), [[1, 0], [0, 3]], [[1, 6], [1, 3]], 20,
                     facts=facts, structured=True)


@_case(ONE_WAVE)
def swap_is_not_a_shortcut():
    def facts(wants):
        assert wants[0]['arrival'].tolist() == [1, 3]           # the swap would have taken 1 step
    return make_case('swap_is_not_a_shortcut', np.zeros((2, 2), np.uint8), [[0, 0], [0, 1]], [[0, 1], [0, 0]], 8,
                     facts=facts, structured=True)


@_case(ONE_WAVE)
def walled_in_agent_stops_the_plan():
    grid = np.zeros((6, 6), np.uint8)
    grid[3:6, 3] = 1
    grid[3, 3:6] = 1                                            # (4,4), (4,5), (5,4), (5,5) walled in

    def facts(wants):
        w = wants[0]
        assert w['status'] == NO_PATH and w['failing'] == 1
        assert w['arrival'][2:].tolist() == [-1, -1] and (w['schedule'][:, 1:] == -1).all()
        assert w['makespan'] == -1 and w['flowtime'] == -1
    return make_case('walled_in_agent_stops_the_plan', grid, [[0, 0], [5, 5], [0, 5], [2, 0]],
                     [[1, 1], [0, 3], [2, 5], [1, 0]], 30, facts=facts, structured=True)


@_case(ONE_WAVE)
def bad_cases_flag_only_themselves():
    grid = np.zeros((5, 5), np.uint8)
    grid[2, 2] = 1
    return _bad_case_variants(grid, np.array([[0, 0], [4, 4], [0, 4]]), np.array([[4, 0], [0, 0], [4, 4]]),
                              (('s', [-1, 0]), ('s', [0, 5]), ('g', [5, 1]), ('g', [1, -1]), ('s', [2, 2]),
                               ('g', [2, 2]), ('s', [4, 4]), ('g', [0, 0])), 16, 'bad_cases_flag_only_themselves')


@_every(ONE_WAVE, 'widest_and_tallest_maps', [(64, 64), (5, 64), (64, 5)], '%dx%d')
def widest_and_tallest_maps(name, H, W):
    """Bit 63 of a row and lane 63 of the wave."""
    grid = np.zeros((H, W), np.uint8)
    grid[H // 2, 1:W - 1] = 1
    return make_case(name, grid, [[0, 0], [H - 1, 0], [0, W - 1]], [[H - 1, W - 1], [0, W - 1], [H - 1, 0]],
                     2 * (H + W), facts=_all_solved, structured=True)


def _non_square_calls():
    """Three 7 x 13 cases, then three 13 x 7 cases, drawn from one generator."""
    rng = np.random.default_rng(13)
    return random_cases(rng, 3, 5, 7, 13, density=0.1), random_cases(rng, 3, 5, 13, 7, density=0.1)


@_case(ONE_WAVE)
def non_square_7x13():
    return case_of_list('non_square_7x13', _non_square_calls()[0], 40)


@_case(ONE_WAVE)
def non_square_13x7():
    return case_of_list('non_square_13x7', _non_square_calls()[1], 40)


@_case(ONE_WAVE)
def restarts_pick_the_best_and_ties_the_lowest():
    rng = np.random.default_rng(21)
    cases = random_cases(rng, 4, 8, 8, density=0.2)
    N = 8
    orders = np.stack([np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(3)]) for _ in cases])
    orders[1, 2] = orders[1, 0]                                 # restart 2 repeats restart 0: a tie
    orders[2, 1:] = orders[2, 0]                                # every restart the same order

    def facts(wants):
        assert wants[2]['restart'] == 0 and wants[1]['restart'] != 2
    return case_of_list('restarts_pick_the_best_and_ties_the_lowest', cases, 32, orders=orders, facts=facts)


@_case(ONE_WAVE)
def only_the_reversed_order_solves():
    grid = np.array([[0, 0, 0],
                     [1, 0, 1]], np.uint8)
    return _reversed_order_case('only_the_reversed_order_solves', grid, np.array([[1, 1], [0, 0]]),
                                np.array([[0, 1], [0, 2]]))


@_case(ONE_WAVE)
def batched_grid_next_to_shared_grid():
    """Three cases on one map: the call gives the same bytes for the map passed once and passed per case."""
    rng = np.random.default_rng(34)
    grid, _, _ = random_cases(rng, 1, 5, 9)[0]
    return case_of_list('batched_grid_next_to_shared_grid', _same_grid_cases(rng, grid, 3, 5), 36)


# -- gnnpp_mapf_team_solve: one workgroup per case, rows of several 64-bit words, several waves of rows ---------
@_case(TEAM)
def more_than_128_agents_on_one_word_rows():
    """129 agents on 20 x 20: an open map where all of them are planned, and one with obstacles where a late agent
    finds no path (more than 128 agents have been looked at by then or not: both are the yardstick's answer)."""
    cases = random_cases(np.random.default_rng(40), 1, 129, 20, density=0.0) + \
        random_cases(np.random.default_rng(41), 1, 129, 20, density=0.1)

    def facts(wants):
        assert wants[0]['status'] == 0 and (wants[0]['arrival'] >= 0).all()
        assert wants[1]['status'] == NO_PATH and wants[1]['failing'] > 64
    return case_of_list('more_than_128_agents_on_one_word_rows', cases, default_horizon(20, 20), facts=facts,
                        poison_ws=True)


@_every(TEAM, 'random_cases_on_rows_of_several_words', [(65,), (128,), (129,)], 'W%d')
def random_cases_on_rows_of_several_words(name, W):
    cases = random_cases(np.random.default_rng(100 + W), 2, 12, 5, W, density=0.1)

    def facts(wants):
        assert any(w['status'] == 0 for w in wants)
        if W >= 128:                                            # (W = 65: one column beyond the boundary; the corridor
            crossed = False                                     # case below forces the crossing there)
            for w, (_, s, g) in zip(wants, cases):
                n = int((w['arrival'] >= 0).sum())              # the planned agents: some go right, some left
                crossed |= bool(((s[:n, 1] // 64) < (g[:n, 1] // 64)).any() and
                                ((s[:n, 1] // 64) > (g[:n, 1] // 64)).any())
            assert crossed
    return case_of_list(name, cases, 2 * (5 + W), facts=facts, poison_ws=True)


@_every(TEAM, 'corridor_forces_the_crossing_both_ways', [(65,), (128,), (129,)], 'W%d')
def corridor_forces_the_crossing_both_ways(name, W):
    """Five rows; the middle one is a wall with two doors, one on each side of the last word boundary b (columns
    b - 1 and b).  Agent 0 goes from the top left to the bottom right corner, agent 1 from the top right to the bottom
    left: both must pass the boundary column, in opposite directions, whichever door they take.  For W = 65 and 129
    column b is the last word's only valid bit."""
    b = 64 if W < 129 else 128
    grid = np.zeros((5, W), np.uint8)
    grid[2, :] = 1
    grid[2, b - 1:b + 1] = 0

    def facts(wants):
        want = wants[0]
        assert want['status'] == 0
        for n, step in ((0, 1), (1, -1)):
            cols = want['schedule'][:want['arrival'][n] + 1, n, 1]
            k = int(np.nonzero(cols == (b if step > 0 else b - 1))[0][0])
            assert cols[k - 1] == cols[k] - step                # entered the boundary column from the other word
    return make_case(name, grid, [[0, 0], [0, W - 1], [1, 10], [4, 5]], [[4, W - 1], [4, 0], [0, W - 2], [0, 3]],
                     4 * W, facts=facts, structured=True, poison_ws=True)


@_case(TEAM)
def swap_refused_across_the_word_boundary():
    """Agents in columns 63 and 64 want each other's cell.  The swap over the boundary is no move: on a 2 x 2 block of
    free cells astride the boundary the second agent goes round (the 2 x 2 case of the one-wave cases, shifted)."""
    grid = np.ones((2, 66), np.uint8)
    grid[0:2, 63:65] = 0

    def facts(wants):
        assert wants[0]['status'] == 0 and wants[0]['arrival'].tolist() == [1, 3]  # the swap would have taken 1 step
    return make_case('swap_refused_across_the_word_boundary', grid, [[0, 63], [0, 64]], [[0, 64], [0, 63]], 12,
                     facts=facts, structured=True)


@_case(TEAM)
def no_way_round_on_the_1x66_strip():
    """With those two cells alone there is no way round: NO_PATH for agent 1, not a swap."""
    grid = np.ones((1, 66), np.uint8)
    grid[0, 63:65] = 0

    def facts(wants):
        assert wants[0]['status'] == NO_PATH and wants[0]['failing'] == 1
    return make_case('no_way_round_on_the_1x66_strip', grid, [[0, 63], [0, 64]], [[0, 64], [0, 63]], 12,
                     facts=facts, structured=True)


@_every(TEAM, 'more_than_one_wave_of_rows', [(65, 6), (70, 9), (66, 65)], '%dx%d')
def more_than_one_wave_of_rows(name, H, W):
    """The vertical exchange across waves: a wall with one door between rows 63 and 64."""
    grid = np.zeros((H, W), np.uint8)
    grid[63, :] = 1
    grid[63, W // 2] = 0
    return make_case(name, grid, [[0, 0], [H - 1, 0], [0, W - 1], [H - 1, W - 1]],
                     [[H - 1, W - 1], [0, W - 1], [H - 1, 0], [1, 1]], 2 * (H + W), facts=_all_solved, structured=True,
                     poison_ws=True)


@_case(TEAM)
def random_cases_on_tall_maps():
    return case_of_list('random_cases_on_tall_maps', random_cases(np.random.default_rng(67), 2, 10, 67, 7, density=0.1),
                        2 * (67 + 7))


@_case(TEAM)
def several_waves_of_rows_of_several_words():
    """70 x 130: 210 threads in four waves, rows of three words, 140 agents."""
    def facts(wants):
        assert (wants[0]['arrival'] >= 0).sum() > 128
    return case_of_list('several_waves_of_rows_of_several_words',
                        random_cases(np.random.default_rng(70130), 1, 140, 70, 130, density=0.1), 200, facts=facts,
                        poison_ws=True)


@_case(TEAM)
def given_orders_with_a_tie():
    rng = np.random.default_rng(21)
    cases = random_cases(rng, 3, 8, 6, 70, density=0.15)
    N = 8
    orders = np.stack([np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(2)]) for _ in cases])
    orders[1, 2] = orders[1, 0]                                 # a tie: the lower index wins
    return case_of_list('given_orders_with_a_tie', cases, 160, orders=orders)


@_case(TEAM)
def failing_restart_on_2x67():
    grid = np.ones((2, 67), np.uint8)
    grid[0, 63:66] = 0
    grid[1, 64] = 0
    return _reversed_order_case('failing_restart_on_2x67', grid, np.array([[1, 64], [0, 63]]),
                                np.array([[0, 64], [0, 65]]))


@_case(TEAM)
def crowded_cases_solved_and_failing():
    return case_of_list('crowded_cases_solved_and_failing',
                        random_cases(np.random.default_rng(8), 6, 10, 5, 66, density=0.2), 60,
                        facts=_status_set({0, NO_PATH}))


@_case(TEAM, 'bad_cases_flag_only_themselves')
def team_bad_cases_flag_only_themselves():
    grid = np.zeros((5, 70), np.uint8)
    grid[2, 66] = 1
    return _bad_case_variants(grid, np.array([[0, 0], [4, 69], [0, 68]]), np.array([[4, 0], [0, 0], [4, 69]]),
                              (('s', [-1, 0]), ('s', [0, 70]), ('g', [5, 1]), ('g', [1, -1]), ('s', [2, 66]),
                               ('g', [2, 66]), ('s', [4, 69]), ('g', [0, 0]), ('s', [0, 100]), ('g', [3, 127])), 160,
                              'team_bad_cases_flag_only_themselves')


@_case(TEAM, 'batched_grid_next_to_shared_grid')
def team_batched_grid_next_to_shared_grid():
    rng = np.random.default_rng(34)
    grid, _, _ = random_cases(rng, 1, 5, 4, 66)[0]
    return case_of_list('team_batched_grid_next_to_shared_grid', _same_grid_cases(rng, grid, 3, 5), 140)


@_case(TEAM)
def outputs_do_not_depend_on_the_slot_count():
    """Five cases of two orders each on 4 x 66: ten work items, planned with a slot each, with one slot for all of
    them, and with three."""
    rng = np.random.default_rng(55)
    cases = random_cases(rng, 5, 6, 4, 66, density=0.15)
    N = 6
    orders = np.stack([np.stack([np.arange(N), rng.permutation(N)]) for _ in cases])
    return case_of_list('outputs_do_not_depend_on_the_slot_count', cases, 60, orders=orders, poison_ws=True)


@_case(TEAM)
def zero_horizon_agent_on_its_goal():
    def facts(wants):
        assert wants[0]['status'] == 0 and wants[0]['arrival'][0] == 0
    return make_case('zero_horizon_agent_on_its_goal', np.zeros((2, 65), np.uint8), [[0, 64]], [[0, 64]], 0,
                     facts=facts, structured=True)


@_case(TEAM)
def zero_horizon_agent_off_its_goal():
    return make_case('zero_horizon_agent_off_its_goal', np.zeros((2, 65), np.uint8), [[0, 64]], [[1, 64]], 0,
                     facts=_status_set({NO_PATH}), structured=True)


# -- what both entry points accept: the same bytes from each ----------------------------------------------------
@_case(BOTH, 'random_10x10')
def both_random_10x10():
    return case_of_list('both_random_10x10', random_cases(np.random.default_rng(5), 4, 6, 10, density=0.15), 40,
                        poison_ws=True)


@_case(BOTH, 'crowded_with_failures')
def both_crowded_with_failures():
    return case_of_list('both_crowded_with_failures', random_cases(np.random.default_rng(8), 6, 10, 7, density=0.25),
                        20, facts=_status_set({0, NO_PATH}), poison_ws=True)


@_case(BOTH, 'restarts_with_a_bad_order')
def both_restarts_with_a_bad_order():
    rng = np.random.default_rng(21)
    cases = random_cases(rng, 3, 8, 8, density=0.2)
    orders = np.stack([np.stack([np.arange(8)] + [rng.permutation(8) for _ in range(2)]) for _ in cases])
    orders[2, 1] = [0, 0, 1, 2, 3, 4, 5, 6]

    def facts(wants):
        assert wants[2]['status'] == BAD_CASE
    return case_of_list('both_restarts_with_a_bad_order', cases, 32, orders=orders, facts=facts, poison_ws=True)


@_case(BOTH, 'widest_one_word_map')
def both_widest_one_word_map():
    grid = np.zeros((64, 64), np.uint8)
    grid[32, 1:63] = 1
    return make_case('both_widest_one_word_map', grid, [[0, 0], [63, 0], [0, 63]], [[63, 63], [0, 63], [63, 0]], 256,
                     facts=_all_solved, structured=True, poison_ws=True)


@_case(BOTH, '128_agents_on_16x16')
def both_128_agents_on_16x16():
    g, s, gl = random_cases(np.random.default_rng(77), 1, 128, 16, density=0.05)[0]
    return make_case('both_128_agents_on_16x16', g, s, gl, 64, poison_ws=True)


@_case(BOTH, 'unplanned_tail_past_one_wave_of_agents')
def both_unplanned_tail_past_one_wave_of_agents():
    """16 x 16, 72 agents, T_max + 1 = 41: agents 0 .. 69 are committed, agent 70 is walled into the corner, agent 71 is
    never planned -- the unplanned rows of the schedule and of the arrivals lie past the first 64 agents."""
    grid = np.zeros((16, 16), np.uint8)
    grid[13, 13:] = 1
    grid[13:, 13] = 1                                           # rows and columns 14, 15 walled in
    rng = np.random.default_rng(70)
    free = np.argwhere(grid == 0)
    free = free[(free[:, 0] < 13) | (free[:, 1] < 13)]
    idx = rng.choice(len(free), 2 * 72, replace=False)
    starts, goals = free[idx[:72]].copy(), free[idx[72:]].copy()
    starts[70] = (15, 15)

    def facts(wants):
        w = wants[0]
        assert w['status'] == NO_PATH and w['failing'] == 70
        assert (w['arrival'][:70] >= 0).all() and w['arrival'][70:].tolist() == [-1, -1]
        assert (w['schedule'][:, 70:] == -1).all() and (w['schedule'][:, :70] >= 0).all()
    return make_case('both_unplanned_tail_past_one_wave_of_agents', grid, starts, goals, 40, facts=facts, poison_ws=True)
