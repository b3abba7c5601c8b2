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
