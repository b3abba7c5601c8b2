"""Yardstick for the schedule -> training-sample transformer: a plain numpy restatement of the reference's
onlineExpert/DataTransformer_local_onlineExpert.py (obtainSchedule, computeAdjacencyMatrix, toSeqInputTensor),
SEQUENTIAL as the reference writes it -- the radius is carried from step to step and the final one rebuilds every
step -- not the per-step-maximum form the kernels use.  tests/golden/expert_schedules.npz (the real reference, through
tools/gen_expert_golden.py) pins this restatement; it then serves random cases beyond the golden set.

Also the synthetic solved cases both use: random obstacle maps, shortest paths with random waits as the "expert".
"""
from collections import deque

import numpy as np

from oracle.rollout_oracle import _connected, build_observations

DELTA = [[-1, 0], [0, -1], [1, 0], [0, 1], [0, 0]]          # up, left, down, right, stop (the reference's order)


def schedule_targets(goal, schedule):
    """[T,N,5] one-hot of schedule[t+1] - schedule[t]; after the last state comes the goal (obtainSchedule).
    ValueError on any other move, like the reference's list.index."""
    T, N = schedule.shape[:2]
    nxt = np.concatenate([schedule[1:], np.asarray(goal)[None]], 0)
    out = np.zeros((T, N, 5), dtype=np.float64)
    for t in range(T):
        for n in range(N):
            out[t, n, DELTA.index([int(nxt[t, n, 0] - schedule[t, n, 0]), int(nxt[t, n, 1] - schedule[t, n, 1])])] = 1
    return out


def schedule_gso(schedule, radius0=5.0):
    """computeAdjacencyMatrix: (W [T,N,N] float64, final radius, times the radius grew)."""
    pos = np.asarray(schedule, dtype=np.float64)
    T, N = pos.shape[:2]
    threshold, growth = radius0, 0

    def adjacency(t, r):
        d = np.sqrt(((pos[t][:, None, :] - pos[t][None, :, :]) ** 2).sum(-1))
        A = (d < r).astype(np.float64)
        np.fill_diagonal(A, 0.0)
        return A

    for t in range(T):
        while not _connected(adjacency(t, threshold)):
            threshold = threshold * 1.1
            growth += 1
    W = np.zeros((T, N, N))
    for t in range(T):
        A = adjacency(t, threshold)
        s = np.sqrt(1. / A.sum(axis=1))
        W[t] = (s[:, None] * A) * s[None, :]
    return W, threshold, growth


def reference_samples(grid, goal, schedule, radius0=5.0):
    """dict(input [T,N,3,11,11] f32, GSO [T,N,N] f64, target [T,N,5] f32, radius, growth) of one case."""
    schedule = np.asarray(schedule, dtype=np.int64)
    W, radius, growth = schedule_gso(schedule, radius0)
    obs = np.stack([build_observations(np.asarray(grid), goal, schedule[t]) for t in range(len(schedule))])
    return {'input': obs, 'GSO': W, 'target': schedule_targets(goal, schedule).astype(np.float32),
            'radius': radius, 'growth': growth}


# ---- synthetic solved cases -------------------------------------------------------------------------
def _bfs_path(grid, start, goal):
    H, W = grid.shape
    prev = {tuple(start): None}
    q = deque([tuple(start)])
    while q:
        c = q.popleft()
        if c == tuple(goal):
            break
        for dx, dy in DELTA[:4]:
            n = (c[0] + dx, c[1] + dy)
            if 0 <= n[0] < H and 0 <= n[1] < W and not grid[n] and n not in prev:
                prev[n] = c
                q.append(n)
    if tuple(goal) not in prev:
        return None
    path, c = [], tuple(goal)
    while c is not None:
        path.append(c)
        c = prev[c]
    return path[::-1]


def expert_paths(rng, grid, starts, goals, wait=0.15, max_steps=None):
    """Every agent's path: a shortest path with random waits, ending on its goal; agents ignore each other (the
    transformer does not care).  None when a goal cannot be reached.  max_steps caps the path lengths: goals[n] is
    then MOVED to where the walk stops."""
    paths = []
    for n in range(len(starts)):
        p = _bfs_path(grid, starts[n], goals[n])
        if p is None:
            return None
        walk = []
        for c in p[:-1]:
            walk.append(c)
            while rng.random() < wait:
                walk.append(c)
        walk.append(p[-1])
        if max_steps is not None and len(walk) > max_steps:
            walk = walk[:max_steps]
            goals[n] = walk[-1]
        paths.append(walk)
    return paths


def random_map(rng, N, H, W, density=0.1, box=None):
    """(grid [H,W] uint8, starts [N,2], goals [N,2]) on distinct free cells.  box = (x0, y0, side): starts and goals
    are drawn inside that square (a team that stays together)."""
    while True:
        grid = (rng.random((H, W)) < density).astype(np.uint8)
        free = np.argwhere(grid == 0)
        if box is not None:
            x0, y0, side = box
            free = free[(free[:, 0] >= x0) & (free[:, 0] < x0 + side) & (free[:, 1] >= y0) & (free[:, 1] < y0 + side)]
        if len(free) < 2 * N:
            continue
        idx = rng.choice(len(free), size=2 * N, replace=False)
        return grid, free[idx[:N]].astype(np.int64), free[idx[N:]].astype(np.int64)


def random_case(rng, N, H, W, density=0.1, wait=0.15, box=None, max_steps=None):
    """(grid, goal [N,2], paths) of a solvable synthetic case."""
    while True:
        grid, starts, goals = random_map(rng, N, H, W, density, box)
        paths = expert_paths(rng, grid, starts, goals, wait, max_steps)
        if paths is not None:
            return grid, goals, paths


def schedule_of(paths, goal):
    """[makespan + 1, N, 2]: agents that arrive early wait on their goal (obtainSchedule)."""
    T = max(len(p) for p in paths)
    out = np.zeros((T, len(paths), 2), dtype=np.int64)
    for n, p in enumerate(paths):
        for t in range(T):
            out[t, n] = p[t] if t < len(p) else goal[n]
    return out


def solution_yaml(paths):
    """The solver's output file as the reference reads it (statistics.makespan, schedule.agentK = [{x, y, t}])."""
    lines = ['statistics:', '  cost: %d' % sum(len(p) - 1 for p in paths),
             '  makespan: %d' % (max(len(p) for p in paths) - 1), 'schedule:']
    for n, p in enumerate(paths):
        lines.append('  agent%d:' % n)
        for t, (x, y) in enumerate(p):
            lines += ['    - x: %d' % x, '      y: %d' % y, '      t: %d' % t]
    return '\n'.join(lines) + '\n'


# ---- the golden file --------------------------------------------------------------------------------
def load_golden():
    """[(meta, dict of arrays)] of tests/golden/expert_schedules.npz (tools/gen_expert_golden.py: the real reference)."""
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'expert_schedules.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    keys = ('grid', 'goal', 'failure_yaml', 'solution_yaml', 'schedule', 'input', 'GSO', 'target', 'rollout_start')
    return [(m, {k: z['c%d_%s' % (ci, k)] for k in keys if 'c%d_%s' % (ci, k) in z.files}) for ci, m in enumerate(meta)]


# ---- hand-built calls: defined once, run under the host emulation and on the device ---------------------------
# A call is dict(name, grids [H,W] | [C,H,W], goals [C,N,2], schedules [C x [T_c,N,2]], fp64 (whether the call is given
# an S64 output), status [C x (how, bits)]): ('eq', 0) -- the case is built and must equal reference_samples;
# ('eq', bits) / ('has', bits) -- its status is / contains the bits and none of its rows is written.
BAD_MOVE, BAD_STATE = 1, 2                               # GNNPP_SCHEDULE_* status bits


def make_call(name, grids, goals, schedules, status=None, fp64=True, radius0=5.0):
    return {'name': name, 'grids': np.ascontiguousarray(grids, dtype=np.uint8),
            'goals': np.ascontiguousarray(np.stack(goals), dtype=np.int32),
            'schedules': [np.ascontiguousarray(s, dtype=np.int32) for s in schedules],
            'status': status or [('eq', 0)] * len(schedules), 'fp64': fp64, 'radius0': radius0}


def flipped(grid, goal, schedule):
    """The case turned by 180 degrees: another map, the same distances."""
    shape = np.array(grid.shape)
    return np.ascontiguousarray(grid[::-1, ::-1]), (shape - 1 - goal).astype(np.int32), \
        (shape - 1 - schedule).astype(np.int32)


def ragged_call(ci=0):
    """Cases of 25, 7 and 3 steps share a call: golden case ci, its first 7 steps and its last 3 (each a schedule of
    its own, with its own radius).  A schedule cut at step T is a schedule whose "goal" is the state that followed."""
    m, g = load_golden()[ci]
    sched = g['schedule']
    return make_call('ragged_%d' % ci, g['grid'], [g['goal'], sched[7], g['goal']], [sched, sched[:7], sched[-3:]])


def ragged_call_with_a_map_per_case(ci, fp64=True):
    """ragged_call with a map per case, the middle case turned by 180 degrees (24 agents: 16-byte stores; 10 agents:
    4-byte stores)."""
    m, g = load_golden()[ci]
    sched = g['schedule']
    other, fgoal, fpart = flipped(g['grid'], sched[7], sched[:7])
    return make_call('ragged_maps_%d_%s' % (ci, 'fp64' if fp64 else 'fp32'), np.stack([g['grid'], other, g['grid']]),
                     [g['goal'], fgoal, g['goal']], [sched, fpart, sched[-3:]], fp64=fp64)


def batched_maps_call_without_fp64_copy(ci):
    """One map per case (grid_batched), S64 = NULL: golden case ci turned by 180 degrees, then itself."""
    m, g = load_golden()[ci]
    other, fgoal, fsched = flipped(g['grid'], g['goal'], g['schedule'])
    return make_call('batched_maps_%d' % ci, np.stack([other, g['grid']]), [fgoal, g['goal']], [fsched, g['schedule']],
                     fp64=False)


def status_bits_call():
    """Golden case 2 six times: legal, a diagonal move, a state on an obstacle, a state off the map, a last state two
    cells from the goal, legal.  The flags are the kernel's; the legal cases next to them are built as if alone."""
    m, g = load_golden()[2]
    sched = g['schedule'].copy()
    jump = sched.copy()
    diag = next(d for d in ([1, 1], [1, -1], [-1, 1], [-1, -1]) if g['grid'][tuple(jump[2, 1] + d)] == 0)
    jump[3, 1] = jump[2, 1] + diag                      # a diagonal move into step 3, onto a free cell
    obstacle = np.argwhere(g['grid'] != 0)[0]
    stuck = sched.copy()
    stuck[1, 0] = obstacle                              # a state on an obstacle (also breaks the moves around it)
    off = sched.copy()
    off[0, 4] = [-1, 3]                                 # a state off the map
    late = sched.copy()
    late[-1, 2] = g['goal'][2] + [2, 0]                 # the last state is two cells from the goal
    return make_call('status_bits', g['grid'], [g['goal']] * 6, [sched, jump, stuck, off, late, sched],
                     [('eq', 0), ('eq', BAD_MOVE), ('has', BAD_STATE), ('has', BAD_STATE), ('has', BAD_MOVE), ('eq', 0)])


def calls_without_stage():
    """128 agents (both halves of every lane pair) and a 230 x 230 map: the occupancy grid leaves no room for the LDS
    output stage, the rows go straight to memory."""
    rng = np.random.default_rng(11)
    grid, goal, paths = random_case(rng, 128, 30, 30, density=0.1, max_steps=3)
    full = make_call('128_agents_on_30x30', grid, [goal], [schedule_of(paths, goal)])
    grid, goal, paths = random_case(rng, 3, 230, 230, density=0.05, max_steps=2)
    return full, make_call('3_agents_on_230x230', grid, [goal], [schedule_of(paths, goal)])


def team_growths_call():
    """A team of 132 spread over the map and one kept in a box share a call, without an S64 output: each gets its own
    radius."""
    rng = np.random.default_rng(77)
    N, side = 132, 48
    wide = random_case(rng, N, side, side, density=0.05, max_steps=3)
    tight = random_case(rng, N, side, side, density=0.05, box=(8, 8, 20), max_steps=2)
    scheds = [schedule_of(paths, goal) for _, goal, paths in (wide, tight)]
    return make_call('team_growths', np.stack([wide[0], tight[0]]), [wide[1], tight[1]], scheds, fp64=False)


def integer_bounds(radius0, growth):
    """The integer thresholds (largest d2 with sqrt(d2) < r) of the radii radius0 * 1.1^k, k = 0 .. growth."""
    out, r = [], radius0
    for _ in range(growth + 1):
        t = int(np.ceil(r * r))
        while t >= 0 and not np.sqrt(float(t)) < r:
            t -= 1
        out.append(t)
        r = r * 1.1
    return out


def repeated_bounds_call():
    """radius0 = 1.0, where consecutive radii share an integer threshold (1.1, 1.21, 1.331 all admit d2 <= 1 only): trips
    that build nothing new and still count.  Two cases of two standing steps each on an empty 3 x 24 map: seven agents
    in a row three cells apart (connected from 1.1^12 on) and ten agents two cells apart (from 1.1^8 on)."""
    def standing(N, gap):
        pos = np.stack([np.ones(N, np.int64), gap * np.arange(N)], 1)
        return pos, np.stack([pos, pos])
    (g3, s3), (g2, s2) = standing(7, 3), standing(10, 2)
    pad = np.array([[1, 19], [1, 20], [1, 21]])        # (the call's N is 10: three more behind the chain's end at column 18)
    g3, s3 = np.concatenate([g3, pad]), np.concatenate([s3, np.stack([pad, pad])], 1)
    call = make_call('repeated_bounds', np.zeros((3, 24), np.uint8), [g3, g2], [s3, s2], radius0=1.0)
    wants = call_wants(call)
    assert [w['growth'] for w in wants] == [12, 8]
    for w in wants:
        b = integer_bounds(1.0, w['growth'])
        assert sum(x == y for x, y in zip(b, b[1:])) >= 4, b                  # the same bound on consecutive trips
    return call


def lane_boundary_calls():
    """64 and 65 agents: the last team without and the first with a second agent per lane of the one-wave kernels."""
    rng = np.random.default_rng(64)
    calls = []
    for N in (64, 65):
        grid, goal, paths = random_case(rng, N, 26, 26, density=0.05, max_steps=2)
        calls.append(make_call('%d_agents_on_26x26' % N, grid, [goal], [schedule_of(paths, goal)]))
    return calls


def team_status_bits_call():
    """140 agents, four steps, six times: legal, a diagonal move of agent 133, agent 70 on an obstacle, agent 139 off
    the map at step 0, agent 0 beyond the last column at step 2, legal."""
    rng = np.random.default_rng(5)
    N = 140
    grid, goal, paths = random_case(rng, N, 44, 44, density=0.1, max_steps=4)
    sched = schedule_of(paths, goal).astype(np.int32)
    assert len(sched) == 4
    jump = sched.copy()
    diag = next(d for d in ([1, 1], [1, -1], [-1, 1], [-1, -1])
                if 0 <= min(jump[2, 133] + d) and max(jump[2, 133] + d) < 44 and grid[tuple(jump[2, 133] + d)] == 0)
    jump[3, 133] = jump[2, 133] + diag                  # a diagonal move into step 3, onto a free cell
    stuck = sched.copy()
    stuck[1, 70] = np.argwhere(grid != 0)[0]            # a state on an obstacle (also breaks the moves around it)
    off = sched.copy()
    off[0, 139] = [-1, 3]                               # a state off the map
    off2 = sched.copy()
    off2[2, 0] = [5, 44]
    return make_call('team_status_bits', grid, [goal] * 6, [sched, jump, stuck, off, off2, sched],
                     [('eq', 0), ('eq', BAD_MOVE), ('has', BAD_STATE), ('has', BAD_STATE), ('has', BAD_STATE), ('eq', 0)])


# ---- thin maps: a coordinate difference of up to 65 535 (team call) and 16 383 (the one-wave call's limit) -----------
# d2 reaches 65535^2 = 4 294 836 225: above 2^31, below 2^32 (tests/rollout_team_sim_cases.py has the simulator's twins).
# Every schedule has 2 or 3 steps: the restatement's cost is the first step's radius search, the later steps carry it.
THIN_SIDE = 65536                                        # GNNPP_ROLLOUT_TEAM_MAX_CELLS as one row or one column
ONE_WAVE_SIDE = 16384                                    # schedule_samples_launch: H, W <= 16384
HUGE_RADII = (65535.5, 65536.0, 70000.0, 3.0e9, 3.1e9, 1e10, 1e154, 1e155, 9e299)


def thin_shapes(side):
    return ((1, side), (side, 1))


def _on_strip(H, cells):
    """[..., 2] positions of `cells` along the long side of an H x W map of one row or one column."""
    cells = np.asarray(cells, np.int64)
    pos = np.zeros(cells.shape + (2,), np.int64)
    pos[..., 1 if H == 1 else 0] = cells
    return pos


def _spread(N, side):
    """N cells spread evenly over 0 .. side - 1, both ends occupied."""
    return np.round(np.linspace(0, side - 1, N)).astype(np.int64)


def _two_ends(N, side):
    """One half of the team on the first cells, the other on the last (N = 2: the two end cells)."""
    return np.concatenate([np.arange(N // 2), side - (N - N // 2) + np.arange(N - N // 2)])


def _standing(H, W, cells, steps=2):
    """(grid, goal, schedule) of a team that waits on `cells` of an empty strip."""
    pos = _on_strip(H, cells)
    assert len(set(np.asarray(cells).tolist())) == len(cells) and min(cells) >= 0 and max(cells) < max(H, W)
    return np.zeros((H, W), np.uint8), pos, np.stack([pos] * steps)


def _d2(pos):
    p = np.asarray(pos, np.int64)
    return ((p[:, None] - p[None]) ** 2).sum(-1)


def _assert_wrapping_inputs(pos, name):
    """Some pair has d2 above 2^31, and some pair has 2^31 - 2^17 < d2 mod 2^32: what a wrapped product gets wrong
    (rollout_team_sim_cases._check_wrapping_inputs)."""
    d2 = _d2(pos)
    assert (d2 > 2 ** 31).any() and (d2 % 2 ** 32 > 2 ** 31 - 2 ** 17).any() and d2.max() < 2 ** 32, name


def growth_to_span(radius0, gap):
    """The multiplications by 1.1, in fp64 as the reference makes them, until sqrt(gap^2) < radius: (growth, radius)."""
    r, k = radius0, 0
    while not np.sqrt(float(gap * gap)) < r:
        r, k = r * 1.1, k + 1
    return k, r


def both_ends_call(H, W, fp64=True):
    """Two agents on the two end cells of the strip, two standing steps.  On 65 536 cells the radius grows exactly 100
    times to 5 * 1.1^100; the last bound but one lies above 2^31 (the signed range) and the last above 2^32: the
    0xffffffff clamp of dist2_bound."""
    side = max(H, W)
    grid, goal, sched = _standing(H, W, _two_ends(2, side))
    call = make_call('both_ends_%dx%d' % (H, W), grid, [goal], [sched], fp64=fp64)
    want = call_wants(call)[0]
    assert (want['growth'], want['radius']) == growth_to_span(5.0, side - 1)
    if side == THIN_SIDE:
        assert want['growth'] == 100 and want['radius'] == 68903.06169911187
        assert (want['radius'] / 1.1) ** 2 > 2 ** 31 and want['radius'] ** 2 > 2 ** 32
        _assert_wrapping_inputs(sched[0], call['name'])
    assert (want['GSO'] == np.array([[0.0, 1.0], [1.0, 0.0]])).all()
    return call


def two_ends_call(H, W, N, fp64=True, radius0=5.0):
    """One half of the team on the first cells of the strip, the other on the last; two standing steps.  Each half is a
    chain from radius0 on; the halves meet only when the radius spans the gap between them.  A squared distance that
    wrapped would join them early: a smaller growth."""
    side = max(H, W)
    cells = _two_ends(N, side)
    grid, goal, sched = _standing(H, W, cells)
    call = make_call('two_ends_%dx%d_N%d_%s_r%r' % (H, W, N, 'fp64' if fp64 else 'fp32', radius0), grid, [goal], [sched],
                     fp64=fp64, radius0=radius0)
    want = call_wants(call)[0]
    h = N // 2
    gap = int(cells[h] - cells[h - 1])
    assert gap == side - N + 1 and (want['growth'], want['radius']) == growth_to_span(radius0, gap)
    if side == THIN_SIDE:
        _assert_wrapping_inputs(sched[0], call['name'])
        assert _d2(sched[0])[:h, h:].min() > 2 ** 31
    # no edge between the halves at any growth below the final one, and the restatement's graph has them at the final one
    assert not np.sqrt(float(gap * gap)) < want['radius'] / 1.1
    G = want['GSO'][0]
    assert G[h - 1, h] != 0 and (G[:h, h:] != 0).sum() >= 1 and (G[:h, :h] != 0).any(1).all()
    return call


def spread_call(H, W, N, radius0=5.0, fp64=True):
    """The team evenly spaced over the strip, both ends occupied; two standing steps.  The growth is set by the widest
    gap between neighbours (512 cells at N = 129 on 65 536)."""
    side = max(H, W)
    cells = _spread(N, side)
    grid, goal, sched = _standing(H, W, cells)
    call = make_call('spread_%dx%d_N%d_r%r' % (H, W, N, radius0), grid, [goal], [sched], fp64=fp64, radius0=radius0)
    want = call_wants(call)[0]
    gap = int(np.diff(cells).max())
    assert cells[0] == 0 and cells[-1] == side - 1 and ((N, side) != (129, THIN_SIDE) or gap == 512)
    assert (want['growth'], want['radius']) == growth_to_span(radius0, gap)
    if side == THIN_SIDE:
        _assert_wrapping_inputs(sched[0], call['name'])
    return call


def walk_case(H, W, N):
    """(grid, goal, schedule [3,N,2]) on the strip: the team spread over it; every third agent waits on its goal, the
    others walk three cells towards the middle, the third move taking them onto their goal (the last state is one legal
    move from it).  Four cells on either side of every waiting agent -- inside its field of view, on nobody's way -- an
    obstacle."""
    side = max(H, W)
    cells = _spread(N, side)
    assert np.diff(cells).min() >= 16
    waits = np.arange(N) % 3 == 0
    step = np.where(waits, 0, np.where(np.arange(N) < N / 2, 1, -1))
    sched = _on_strip(H, np.stack([cells + t * step for t in range(3)]))
    goal = _on_strip(H, cells + 3 * step)
    rocks = np.concatenate([cells[waits] - 4, cells[waits] + 4])
    rocks = rocks[(rocks >= 0) & (rocks < side)]
    assert len(rocks) >= 1 and waits.any() and (step != 0).any()
    grid = np.zeros(side, np.uint8)
    grid[rocks] = 1
    visited = np.concatenate([cells + t * step for t in range(4)])
    assert not grid[visited].any()
    return grid.reshape(H, W), goal, sched


def walk_call(H, W, N, fp64=True, extra=()):
    """walk_case and the same case turned by 180 degrees, a map per case (grid_batched, C = 2): the maps differ, so a
    step that read the other case's map -- c * H * W with H * W up to 65 536 -- shows in channel 0.  Targets along the
    strip's axis in both directions, and 'stop'.  extra: further (grid, goal, schedule) cases."""
    grid, goal, sched = walk_case(H, W, N)
    other, fgoal, fsched = flipped(grid, goal, sched)
    assert (grid != other).any() and grid.any() and other.any()
    cases = [(grid, goal, sched), (other, fgoal, fsched)] + list(extra)
    call = make_call('walk_%dx%d_N%d_%s%s' % (H, W, N, 'fp64' if fp64 else 'fp32', '+%d' % len(extra) if extra else ''),
                     np.stack([c[0] for c in cases]), [c[1] for c in cases], [c[2] for c in cases], fp64=fp64)
    axis = (1, 3) if H == 1 else (0, 2)
    hot = np.concatenate([want['target'].argmax(-1).reshape(-1) for want in call_wants(call)[:2]])
    assert set(np.unique(hot).tolist()) == {axis[0], axis[1], 4}
    return call


def thin_status_bits_call(N=129):
    """walk_case on 1 x 65 536 five times: legal, agent 7 at row 1 of the one-row map in step 1, agent N - 1 at column
    65 536 in step 0, agent 1's last move a diagonal one (its goal at row 1: a one-row map cannot host a legal one),
    legal."""
    grid, goal, sched = walk_case(1, THIN_SIDE, N)
    sched = sched.astype(np.int32)
    below = sched.copy()
    below[1, 7, 0] = 1
    beyond = sched.copy()
    assert beyond[0, N - 1, 1] == THIN_SIDE - 1
    beyond[0, N - 1, 1] = THIN_SIDE
    diag = goal.copy()
    assert (goal[1] - sched[-1, 1]).tolist() == [0, 1]
    diag[1, 0] = 1
    return make_call('thin_status_bits_N%d' % N, grid, [goal, goal, goal, diag, goal], [sched, below, beyond, sched, sched],
                     [('eq', 0), ('has', BAD_STATE), ('has', BAD_STATE), ('eq', BAD_MOVE), ('eq', 0)])


def one_wave_limit_call(H, W, N):
    """The one-wave call at its map limit (a side of 16 384): walk, walk turned by 180 degrees and the team on the two
    ends of an empty strip, a map per case."""
    grid, goal, sched = _standing(H, W, _two_ends(N, max(H, W)), steps=3)
    return walk_call(H, W, N, extra=[(grid, goal, sched)])


def beyond_one_wave_limit_call(H, W):
    """Two agents on the ends of a strip one cell longer than the one-wave call takes."""
    assert max(H, W) == ONE_WAVE_SIDE + 1
    grid, goal, sched = _standing(H, W, _two_ends(2, max(H, W)))
    return make_call('beyond_one_wave_%dx%d' % (H, W), grid, [goal], [sched])


def huge_radius_calls(radius0):
    """(three agents on 1 x 40, the 129-agent spread on 1 x 65 536) at a radius0 beyond every distance of the map: the
    restatement says growth 0, radius = radius0, every pair an edge, S64 = sqrt(1 / (N - 1))^2."""
    assert radius0 in HUGE_RADII
    grid, goal, sched = _standing(1, 40, np.array([0, 17, 39]))
    tiny = make_call('huge_radius_tiny_r%r' % radius0, grid, [goal], [sched], radius0=radius0)
    thin = spread_call(1, THIN_SIDE, 129, radius0=radius0)
    for call in (tiny, thin):
        want = call_wants(call)[0]
        N = call['goals'].shape[1]
        s = np.sqrt(1. / (N - 1))
        full = np.full((N, N), (s * 1.0) * s)
        np.fill_diagonal(full, 0.0)
        assert want['growth'] == 0 and want['radius'] == radius0 and (want['GSO'] == full).all()
    # 65535.5 is the first of the radii to span the strip: the ends are 65 535 apart, and a radius of 65 535.0 would not
    d = np.sqrt(float(_d2(thin['schedules'][0][0]).max()))
    assert d == 65535.0 and not d < 65535.0 and d < min(HUGE_RADII) == 65535.5
    return tiny, thin


_CALL_WANTS = {}


def call_wants(call):
    """reference_samples of every case of the call that is to be built (None for the flagged ones), computed once."""
    if call['name'] not in _CALL_WANTS:
        grids = call['grids']
        _CALL_WANTS[call['name']] = [
            reference_samples(grids if grids.ndim == 2 else grids[c], call['goals'][c], call['schedules'][c],
                              call['radius0'])
            if call['status'][c] == ('eq', 0) else None for c in range(len(call['schedules']))]
    return _CALL_WANTS[call['name']]


def assert_call_outputs(out, call, poison, untouched=('obs', 'S')):
    """out: host arrays obs, S, S64 (None when the call has no fp64 copy), target, radius, growth, status, step_info.
    Every built case equals the restatement, element for element; a flagged case shows its bits and `poison` still
    fills its rows of the `untouched` outputs."""
    bounds = np.cumsum([0] + [len(s) for s in call['schedules']])
    for c, want in enumerate(call_wants(call)):
        a, b = int(bounds[c]), int(bounds[c + 1])
        how, bits = call['status'][c]
        if want is None:
            assert (out['status'][c] == bits) if how == 'eq' else (out['status'][c] & bits), (c, out['status'][c])
            for k in untouched:
                rows = out[k][a:b]
                assert (np.isnan(rows) if np.isnan(poison) else rows == poison).all(), (c, k)
            continue
        assert out['status'][c] == 0, (c, out['status'][c])
        assert out['radius'][c] == want['radius'] and out['growth'][c] == want['growth'], c
        assert np.array_equal(out['obs'][a:b], want['input']), c
        assert np.array_equal(out['target'][a:b], want['target']), c
        assert np.array_equal(out['S'][a:b], want['GSO'].astype(np.float32)), c
        if out.get('S64') is not None:
            assert np.array_equal(out['S64'][a:b], want['GSO']), c
        info = out['step_info'][a:b]
        assert (info >> 16 == 0).all() and (info & 0xffff).max() == want['growth'], c
