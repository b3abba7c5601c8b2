"""TEST INFRASTRUCTURE ONLY: the hand-built instances of the simulator's move step (csrc/rollout_kernels.hip for teams
of up to 128 agents, csrc/rollout_team_kernels.hip beyond), with their joint actions and what the sequential oracle
(oracle.rollout_oracle.move_step / loop_step) makes of them.  Each case is defined once here and run twice: under the
host emulation (tests/test_emu_rollout.py, tests/test_emu_rollout_team.py) and on the device
(tests/test_gpu_rollout_cases.py).

A case is dict(name, grids [B,H,W], starts / goals [B,N,2], maxstep [B], actions [T,B,N], loop, check): `loop` cases
are stepped with loop_step (episodes freeze once their own loop has ended) and `check(trace)` asserts, on the oracle's
trace alone, that the case is as hard as its name says (a floor on the number of tie-breaks and the like)."""
import functools
import random

import numpy as np

from oracle import rollout_oracle as ro
from rollout_team_cases import Recorder, corridor_instance, make_instances


def _case(name, grids, starts, goals, maxstep, actions, loop=False, check=None):
    B = len(starts)
    return {'name': name, 'grids': np.ascontiguousarray(grids, dtype=np.uint8),
            'starts': np.ascontiguousarray(starts, dtype=np.int32), 'goals': np.ascontiguousarray(goals, dtype=np.int32),
            'maxstep': np.broadcast_to(np.asarray(maxstep, np.int32), (B,)).copy(),
            'actions': np.ascontiguousarray(actions, dtype=np.int32), 'loop': loop, 'check': check}


def _dense_instance(rng, B, N, W):
    """Crowded little maps: N agents on W x W cells, starts and goals drawn independently.  A map of more than 100
    columns keeps its agents in one 5 x 5 corner, so that they still collide."""
    grids = (rng.random((B, W, W)) < 0.04).astype(np.uint8)
    starts = np.zeros((B, N, 2), np.int32)
    goals = np.zeros((B, N, 2), np.int32)
    for b in range(B):
        if W > 100:
            grids[b, :5, :5] = 0
        free = np.argwhere(grids[b] == 0)
        if W > 100:
            free = free[(free[:, 0] < 5) & (free[:, 1] < 5)]
        while len(free) < N:
            grids[b] = 0
            free = np.argwhere(grids[b] == 0)
        starts[b] = free[rng.choice(len(free), N, replace=False)]
        goals[b] = free[rng.choice(len(free), N, replace=False)]
    return grids, starts, goals


def _tie_break_floor(floor):
    def check(trace):
        assert trace['calls'].sum() > floor, (int(trace['calls'].sum()), floor)
    return check


DENSE_SHAPES = ((24, 9, 4), (12, 14, 5), (6, 70, 10), (3, 14, 182))


@functools.lru_cache(None)
def dense_conflict_cases():
    """(B, N, W) of DENSE_SHAPES, six steps of random joint actions each: lots of vertex conflicts, chains of
    fall-backs and swaps per step.  The last: a map of more than 32 768 cells has no LDS cell-count map -- the collision
    candidates come from the all-pairs scan.  More than 20 B / 6 tie-breaks each."""
    rng = np.random.default_rng(21)
    cases = []
    for (B, N, W) in DENSE_SHAPES:
        grids, starts, goals = _dense_instance(rng, B, N, W)
        acts = np.stack([rng.integers(0, 5, size=(B, N)) for _ in range(6)])
        cases.append(_case('dense_%dx%d_on_%d' % (B, N, W), grids, starts, goals, 50, acts,
                           check=_tie_break_floor(20 * B // 6)))
    return cases


TEAM_DENSE_FLOOR = 500


@functools.lru_cache(None)
def team_dense_conflict_case():
    """The large-team kernels' counterpart: 129 agents on 16 x 16 (256 cells, just under 2 per agent; the next smaller
    square, 15 x 15, is 1.7), two episodes, six steps of random joint actions.  The oracle alone, on the CPU, counts 541
    tie-breaks on this instance (34 to 71 per episode and step): the floor is 500."""
    rng = np.random.default_rng(129)
    B, N, W = 2, 129, 16
    grids, starts, goals = _dense_instance(rng, B, N, W)
    acts = np.stack([rng.integers(0, 5, size=(B, N)) for _ in range(6)])
    return _case('team_dense_2x129_on_16', grids, starts, goals, 50, acts, check=_tie_break_floor(TEAM_DENSE_FLOOR))


@functools.lru_cache(None)
def team_corridor_case():
    """200 agents packed head to tail in the lanes of rollout_team_cases.corridor_instance, mostly pushing forward: the
    fall-backs chain through many repeat passes of the collision check and the all-stop branch fires."""
    B, N, H, W = 2, 200, 24, 36
    grids, starts, goals = corridor_instance(B, N, H, W)
    rng = np.random.default_rng(5)
    acts = np.stack([np.where(rng.random((B, N)) < 0.8, 3, rng.integers(0, 5, size=(B, N))) for _ in range(4)])

    def check(trace):
        assert trace['all_stop'] > 0 and trace['most_passes'] >= 4, (trace['all_stop'], trace['most_passes'])
    return _case('team_corridor_2x200_on_24x36', grids, starts, goals, 50, acts, check=check)


def _first_episode_one_step_from_goal(trace, N):
    assert trace['stats'][0].tolist() == [1, N]         # ended by allReachGoal, long before its maxstep
    assert trace['done'][-1].all()


@functools.lru_cache(None)
def mixed_maxstep_case():
    """Six episodes of five agents with limits of their own; episode 0: every agent one step (action 3) from its
    goal, so all arrive at call 1 and call 2 sees allReachGoal and ends the loop."""
    rng = np.random.default_rng(3)
    B, N, W = 6, 5, 7
    grids = (rng.random((B, W, W)) < 0.05).astype(np.uint8)
    starts = np.zeros((B, N, 2), np.int32)
    goals = np.zeros((B, N, 2), np.int32)
    for b in range(B):
        free = np.argwhere(grids[b] == 0)
        pick = rng.choice(len(free), 2 * N, replace=False)
        starts[b], goals[b] = free[pick[:N]], free[pick[N:]]
    grids[0] = 0
    starts[0] = [[i, 0] for i in range(N)]
    goals[0] = [[i, 1] for i in range(N)]
    acts = np.stack([rng.integers(0, 5, size=(B, N)) for _ in range(10)])
    acts[0, 0] = 3
    return _case('mixed_maxstep_6x5_on_7', grids, starts, goals, [6, 2, 3, 8, 1, 5], acts, loop=True,
                 check=lambda trace: _first_episode_one_step_from_goal(trace, N))


@functools.lru_cache(None)
def team_mixed_maxstep_case():
    """Per-episode limits at N = 160: an episode past its own maxstep, or whose loop broke after allReachGoal, is
    frozen."""
    rng = np.random.default_rng(4)
    B, N, W = 3, 160, 32
    grids, starts, goals = make_instances(rng, B, N, W, W, 0.04)
    grids[0] = 0                                        # episode 0: every agent one step (action 3) from its goal
    starts[0] = [[i // 16, 2 * (i % 16)] for i in range(N)]
    goals[0] = starts[0] + [0, 1]
    acts = np.stack([rng.integers(0, 5, size=(B, N)) for _ in range(6)])
    acts[0, 0] = 3
    return _case('team_mixed_maxstep_3x160_on_32', grids, starts, goals, [5, 2, 3], acts, loop=True,
                 check=lambda trace: _first_episode_one_step_from_goal(trace, N))


_TRACES = {}


def _steps(values):
    return [-1 if v is None else int(v) for v in values]


def oracle_trace(case, tie='lowest', seed=0):
    """What the oracle makes of the case, episode by episode and step by step (computed once): flags [T,B,3], pos
    [T,B,N,2], reached / start_step / end_step [T,B,N] (-1: not set), calls [T,B] (tie-breaks: 0 for an episode that is
    frozen), done [T,B], for a `loop` case the final stats [B,2], and the all-stop branches and the most passes of the
    collision check in one step.  tie: 'lowest' (the lowest agent index moves) or 'mt19937'
    (random.Random(seed + b).choice for episode b)."""
    from unittest import mock
    key = (case['name'], tie, seed)
    if key in _TRACES:
        return _TRACES[key]
    T, B, N = case['actions'].shape
    eps = [ro.EpisodeState(case['grids'][b], case['goals'][b], case['starts'][b], case['maxstep'][b]) for b in range(B)]
    picks = [(lambda c: c[0]) if tie == 'lowest' else random.Random(seed + b).choice for b in range(B)]
    out = {'flags': np.zeros((T, B, 3), np.int32), 'pos': np.zeros((T, B, N, 2), np.int32),
           'reached': np.zeros((T, B, N), np.int32), 'start_step': np.zeros((T, B, N), np.int32),
           'end_step': np.zeros((T, B, N), np.int32), 'calls': np.zeros((T, B), np.int32),
           'done': np.zeros((T, B), bool), 'all_stop': 0, 'most_passes': 0}
    passes = mock.Mock(wraps=ro._inter_robot_collision)  # (counts the passes of the collision check)
    step = ro.loop_step if case['loop'] else ro.move_step
    with mock.patch.object(ro, '_inter_robot_collision', passes):
        for t in range(T):
            for b in range(B):
                rec = Recorder(eps[b], picks[b])
                passes.reset_mock()
                f = step(eps[b], case['actions'][t, b], t + 1, rec)
                out['flags'][t, b] = [int(v) for v in f]
                out['pos'][t, b] = eps[b].cur
                out['reached'][t, b] = [int(v) for v in eps[b].reached]
                out['start_step'][t, b] = _steps(eps[b].start_step)
                out['end_step'][t, b] = _steps(eps[b].end_step)
                out['calls'][t, b] = rec.calls
                out['done'][t, b] = eps[b].done
                out['all_stop'] += rec.all_stop
                out['most_passes'] = max(out['most_passes'], passes.call_count)
    if case['loop']:
        out['stats'] = np.array([[ep.makespan, ep.flowtime] for ep in eps], np.int32)
    if case['check'] is not None:
        case['check'](out)
    _TRACES[key] = out
    return out
