"""TEST INFRASTRUCTURE ONLY: the shared cases of the rollout trace (include/gnnpp_rollout_trace.h) and a numpy yardstick of
its record rule.  Each case is defined once here and run under the host emulation (tests/test_emu_rollout_trace.py) and on
the device (tests/test_gpu_rollout_trace.py).

The yardstick knows nothing of the code under test: it takes the positions after every move (the golden `pos` of the real
simulator's traces, the sequential oracle's trace, or an unrecorded twin's read-backs), the actions that were asked for and
which episodes were frozen at entry of each move, and says what a trace must hold."""
import functools

import numpy as np

DELTA = {0: (-1, 0), 1: (0, -1), 2: (1, 0), 3: (0, 1)}       # every other id: (0, 0)
POISON = 0x5a5a5a5a


def first_max(logits):
    """The move kernels' decode, `l[k] > best` from k = 1 on: the lowest index wins a tie, a NaN never wins."""
    logits = np.asarray(logits, np.float32)
    key = np.zeros(logits.shape[:-1], np.int64)
    best = logits[..., 0].copy()
    for k in range(1, logits.shape[-1]):
        with np.errstate(invalid='ignore'):
            better = logits[..., k] > best
        best = np.where(better, logits[..., k], best)
        key = np.where(better, k, key)
    return key


def record_rule(rows, asked, frozen, T_cap=None):
    """rows [T+1,B,N,2]: the positions before the first move and after each; asked [T,B,N]: action ids; frozen [T,B]: the
    episode was frozen at entry of move t + 1.  -> dict(path [B,T_cap+1,N,2] (rows beyond T: -1, never compared), action
    [B,T_cap,N] int8, moves, shielded [B,N], steps [B])."""
    rows, asked, frozen = np.asarray(rows, np.int64), np.asarray(asked, np.int64), np.asarray(frozen, bool)
    T, B, N = asked.shape
    T_cap = T if T_cap is None else T_cap
    out = {'path': np.full((B, T_cap + 1, N, 2), -1, np.int32), 'action': np.full((B, T_cap, N), -1, np.int8),
           'moves': np.zeros((B, N), np.int32), 'shielded': np.zeros((B, N), np.int32), 'steps': np.zeros(B, np.int32)}
    out['path'][:, :T + 1] = rows.transpose(1, 0, 2, 3)
    for t in range(T):
        for b in range(B):
            if frozen[t, b]:
                continue
            out['steps'][b] = t + 1
            for n in range(N):
                a = int(asked[t, b, n])
                out['action'][b, t, n] = np.int64(a).astype(np.int8)
                step = rows[t + 1, b, n] - rows[t, b, n]
                out['moves'][b, n] += int(step.any())
                if a != 4:
                    out['shielded'][b, n] += int(tuple(step) != DELTA.get(a, (0, 0)))
    return out


def golden_expectation(z, ci, m):
    """What the trace of the replayed golden case ci must hold: the reference's own path_predict and actions (independent
    of the code under test), never frozen (the recorded loop ends with its last call)."""
    pos = z['t%d_pos' % ci].astype(np.int64)[:, None]                  # [T+1,1,N,2]
    asked = z['t%d_actions' % ci].astype(np.int64)[:, None]            # [T,1,N]
    assert (asked[:, 0] == first_max(z['t%d_logits' % ci])).all()       # the golden files agree with themselves
    return record_rule(pos, asked, np.zeros((m['T'], 1), bool))


def golden_conflicts(z, ci, m):
    """(vertex, swap) counts of include/gnnpp_mapf_audit.h taken from the golden `pos`: flagged (step, agent) pairs.  A
    swap is examined only on a transition whose two layers hold no vertex flag."""
    pos = z['t%d_pos' % ci].astype(np.int64)
    W = int(pos.max()) + 2
    cell = pos[..., 0] * W + pos[..., 1]                              # [T+1,N]
    shared = np.array([[(row == c).sum() > 1 for c in row] for row in cell])
    vertex = int(shared.sum())
    swap = 0
    for t in range(len(cell) - 1):
        if shared[t].any() or shared[t + 1].any():
            continue
        for i in range(cell.shape[1]):
            if cell[t + 1, i] != cell[t, i]:
                swap += int(((cell[t] == cell[t + 1, i]) & (cell[t + 1] == cell[t, i])).any())
    return vertex, swap


def _free_cells(rng, grid, count):
    free = np.argwhere(grid == 0)
    return free[rng.choice(len(free), count, replace=False)]


@functools.lru_cache(None)
def frozen_case():
    """B = 4 episodes of 5 agents on 8 x 8 with limits [3, 7, 12, 12], 12 steps of random joint actions.  Episode 2 starts
    on its goals and asks for the map's edge (an agent that never asks to move has no start step in the reference: the
    oracle refuses it; call 1 counts the arrivals, call 2 sees allReachGoal and ends the loop); episode 3 never
    arrives (its goals are walled in)."""
    import rollout_cases as rc
    rng = np.random.default_rng(77)
    B, N, W, T = 4, 5, 8, 12
    grids = (rng.random((B, W, W)) < 0.06).astype(np.uint8)
    grids[3, :3, :3] = 0
    grids[3, 3, :4] = 1
    grids[3, :4, 3] = 1                                           # a closed 3 x 3 room in the corner
    starts = np.zeros((B, N, 2), np.int32)
    goals = np.zeros((B, N, 2), np.int32)
    for b in range(B):
        cells = _free_cells(rng, grids[b], 2 * N)
        starts[b], goals[b] = cells[:N], cells[N:]
    grids[2, 0, :N] = 0
    starts[2] = [[0, i] for i in range(N)]                    # along the top edge, and every step asks to go up: shielded
    goals[2] = starts[2]
    room = np.argwhere(grids[3, :3, :3] == 0)
    goals[3] = room[:N]
    outside = np.argwhere(grids[3] == 0)
    outside = outside[(outside[:, 0] > 3) | (outside[:, 1] > 3)]
    starts[3] = outside[rng.choice(len(outside), N, replace=False)]
    acts = rng.integers(0, 5, size=(T, B, N))
    acts[:, 2] = 0

    def check(trace):
        assert trace['done'][:, 2].tolist() == [False] + [True] * 11
        assert not trace['done'][:-1, 3].any() and not trace['reached'][-1, 3].any()
    return rc._case('trace_frozen_4x5_on_8', grids, starts, goals, [3, 7, 12, 12], acts, loop=True, check=check)


EDGE_SHAPES = ((3, 1, 16, 16), (2, 128, 16, 16), (2, 129, 16, 16), (1, 1024, 64, 64))     # (B, N, H, W)


@functools.lru_cache(None)
def edge_cases():
    """Hand-made action ids (0 .. 4 and, for one agent, an id that is none of them), 4 steps: one agent, either side of the
    seam between the one-wave and the team kernels, and the largest team."""
    rng = np.random.default_rng(1024)
    cases = []
    for (B, N, H, W) in EDGE_SHAPES:
        grids = (rng.random((B, H, W)) < 0.03).astype(np.uint8)
        starts = np.zeros((B, N, 2), np.int32)
        goals = np.zeros((B, N, 2), np.int32)
        for b in range(B):
            starts[b] = _free_cells(rng, grids[b], N)         # (drawn independently: 129 agents fill half of 16 x 16)
            goals[b] = _free_cells(rng, grids[b], N)
        acts = rng.integers(0, 5, size=(4, B, N)).astype(np.int32)
        acts[1, 0, 0] = 7                                       # none of the five: the move kernels leave the agent in place
        cases.append({'name': 'edge_%dx%d_on_%dx%d' % (B, N, H, W), 'grids': grids, 'starts': starts, 'goals': goals,
                      'maxstep': np.full(B, 50, np.int32), 'actions': acts})
    return cases


def frozen_at_entry(done_after, maxstep):
    """done_after [T,B]: done[b] as each move left it; -> frozen [T,B] at entry of move t + 1, the move kernels' condition."""
    done_after = np.asarray(done_after, bool)
    T, B = done_after.shape
    before = np.concatenate([np.zeros((1, B), bool), done_after[:-1]], 0)
    return before | (np.arange(1, T + 1)[:, None] > np.asarray(maxstep)[None, :])


def assert_trace_equals(got, want, T, what=''):
    """got: dict of host arrays of a trace; want: record_rule's.  Rows 0 .. T of path, all of the rest, exactly."""
    assert np.array_equal(got['steps'], want['steps']), (what, got['steps'], want['steps'])
    assert np.array_equal(got['path'][:, :T + 1], want['path'][:, :T + 1]), what
    assert np.array_equal(got['action'][:, :T], want['action'][:, :T]), what
    assert (got['action'][:, T:] == -1).all(), what
    assert np.array_equal(got['moves'], want['moves']), (what, got['moves'], want['moves'])
    assert np.array_equal(got['shielded'], want['shielded']), (what, got['shielded'], want['shielded'])
