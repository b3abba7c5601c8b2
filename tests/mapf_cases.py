"""Yardstick of the device MAPF solver (csrc/mapf_kernels.hip, gnn_pathplanning_amd/mapf.py): a SEQUENTIAL numpy
restatement of the prioritized-planning contract of include/gnnpp.h (gnnpp_mapf), and two independent checks of it:

  bfs_arrival      a plain (cell, t) breadth-first search with a queue, given the earlier agents' actual paths: the
                   smallest arrival an agent can have (or None), to confirm each a_i is the minimum and each failure
                   genuine;
  check_plans      a validator for moves, obstacles, vertex, swap and parking conflicts, and replay_through_simulator:
                   the schedule played through the reference simulator (oracle.rollout_oracle.move_step), which must
                   flag no collision and reproduce every position.
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
