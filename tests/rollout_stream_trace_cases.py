"""TEST INFRASTRUCTURE ONLY: what the trace of a streamed rollout (include/gnnpp_rollout_stream_trace.h) must hold for the
shared case table of streamed rollouts (tests/rollout_stream_cases.py, imported and not edited), for the host emulation
(tests/test_emu_rollout_stream_trace.py) and the device (tests/test_gpu_rollout_stream_trace_cases.py).

The expected value of every case is the PLAIN per-case rollout (B = C) of the same scripts, recorded by the existing
recorder (gnnpp_rollout_trace_begin / _record); two named cases of the hand table carry every value written out by hand;
and `model` restates the record rule in numpy from a log of what each move left, with two switchable faults, so that the
tests can show that the table tells a wrong row index and a missing comparison with the seat."""
import numpy as np

KEYS = ('path', 'action', 'moves', 'shielded', 'steps')

# tests/rollout_stream_cases.py::hand_table_6x6, derived from its docstring and scripts (3 = right (0,+1), 1 = left (0,-1),
# 4 = stay; an empty 6 x 6 map, the two agents never meet):
#   'stays_on_goal' (case 5, limit 9): agent 0 sits on its goal (1,1) and stays; agent 1 walks (2,0) -> (2,1) -> (2,2) ->
#       (2,3) = its goal.  The call of step 4 finds everybody arrived and ends the loop; it is not frozen at entry, so it is
#       recorded: steps 4, row 4 repeats row 3, and its asked actions are the script's stays.  Nothing is ever shielded.
#   'never_moved' (case 6, limit 3): agent 0 stays on (1,1), agent 1 steps (3,0) -> (3,1) -> (3,0) and then stays; the
#       third call is the limit: steps 3.
HAND = {
    'stays_on_goal': {'steps': 4, 'moves': [0, 3], 'shielded': [0, 0],
                      'path': [[[1, 1], [2, 0]], [[1, 1], [2, 1]], [[1, 1], [2, 2]], [[1, 1], [2, 3]], [[1, 1], [2, 3]]],
                      'action': [[4, 3], [4, 3], [4, 3], [4, 4]]},
    'never_moved': {'steps': 3, 'moves': [0, 2], 'shielded': [0, 0],
                    'path': [[[1, 1], [3, 0]], [[1, 1], [3, 1]], [[1, 1], [3, 0]], [[1, 1], [3, 0]]],
                    'action': [[4, 3], [4, 1], [4, 4]]},
}
DELTA = {0: (-1, 0), 1: (0, -1), 2: (1, 0), 3: (0, 1)}       # every other id: (0, 0)


def t_cap(tab):
    return int(tab['maxstep'].max())


def assert_case_traces(tab, got, want, lived=None):
    """got: the stream's per-case tables; want: the plain recorded rollout's (B = C).  steps, moves, shielded, rows
    0 .. steps[c] of path and rows 0 .. steps[c] - 1 of action exactly; the rows beyond are what begin left: 0 / -1."""
    name = tab['name']
    assert np.array_equal(got['steps'], want['steps']), (name, got['steps'], want['steps'])
    assert (got['steps'] >= 1).all(), (name, got['steps'])
    if lived is not None:                                    # the stream's own count of moves that were not frozen
        assert np.array_equal(got['steps'], lived), (name, got['steps'], lived)
    assert np.array_equal(got['moves'], want['moves']), (name, got['moves'], want['moves'])
    assert np.array_equal(got['shielded'], want['shielded']), (name, got['shielded'], want['shielded'])
    for c, s in enumerate(int(v) for v in got['steps']):
        assert np.array_equal(got['path'][c, :s + 1], want['path'][c, :s + 1]), (name, 'path', c)
        assert np.array_equal(got['action'][c, :s], want['action'][c, :s]), (name, 'action', c)
        assert (got['action'][c, :s] >= 0).all(), (name, 'action recorded', c)
        assert (got['path'][c, s + 1:] == 0).all() and (got['action'][c, s:] == -1).all(), (name, 'beyond steps', c)
        assert np.array_equal(got['path'][c, 0], tab['starts'][c]), (name, 'row 0', c)
    for key, c in tab['named'].items():
        if key in HAND:
            assert_hand(got, c, key)


def assert_hand(got, c, key):
    h = HAND[key]
    s = h['steps']
    assert int(got['steps'][c]) == s and got['moves'][c].tolist() == h['moves'] and \
        got['shielded'][c].tolist() == h['shielded'], (key, got['steps'][c], got['moves'][c], got['shielded'][c])
    assert got['path'][c, :s + 1].tolist() == h['path'], (key, got['path'][c, :s + 1].tolist())
    assert got['action'][c, :s].tolist() == h['action'], (key, got['action'][c, :s].tolist())


def model(tab, log, B, mutant=None):
    """The record rule in numpy.  log: one entry per move, dict(t, case [B], t0 [B], maxstep [B], actions [B,N], pos
    [B,N,2] and done [B] as the move left them).  mutant: None, 'global_rows' (rows indexed by the global step t instead
    of t - t0) or 'no_t0' (frozen decided by seen_done != 0 && seen_done < t, the fixed-batch recorder's rule, with the
    word never rewound).  -> the per-case tables and seen_done."""
    C, N = tab['starts'].shape[:2]
    T = t_cap(tab)
    out = {'path': np.zeros((C, T + 1, N, 2), np.int32), 'action': np.full((C, T, N), -1, np.int8),
           'moves': np.zeros((C, N), np.int32), 'shielded': np.zeros((C, N), np.int32), 'steps': np.full(C, -1, np.int32),
           'seen_done': np.zeros(B, np.int32)}
    seen_done = out['seen_done']
    for e in log:
        t = int(e['t'])
        for b in range(B):
            c = int(e['case'][b])
            if c < 0:
                continue
            t0 = int(e['t0'][b])
            k, seen = t - t0, int(seen_done[b])
            if mutant == 'no_t0':
                frozen = (seen != 0 and seen < t) or t > int(e['maxstep'][b])
            else:
                frozen = (seen > t0 and seen < t) or t > int(e['maxstep'][b])
            row = t if mutant == 'global_rows' else k
            if not frozen and 1 <= row <= T:
                for n in range(N):
                    prev = tab['starts'][c, n] if k == 1 else out['path'][c, row - 1, n].copy()
                    if k == 1:
                        out['path'][c, row - 1, n] = prev
                    cur = e['pos'][b, n]
                    out['path'][c, row, n] = cur
                    a = int(e['actions'][b, n])
                    out['action'][c, row - 1, n] = np.int64(a).astype(np.int8)
                    step = tuple(int(v) for v in cur - prev)
                    out['moves'][c, n] += int(step != (0, 0))
                    if a != 4:
                        out['shielded'][c, n] += int(step != DELTA.get(a, (0, 0)))
                out['steps'][c] = row
            fresh = seen == 0 if mutant == 'no_t0' else not seen > t0
            if fresh and e['done'][b] != 0:
                seen_done[b] = t
    return out


def tells(a, b, c):
    """Do two sets of per-case tables differ in case c?"""
    return any(not np.array_equal(a[k][c], b[k][c]) for k in KEYS)


def successors(slot, t0, lived):
    """[(case, previous tenant of its slot, gap)] for every case seated into a slot that held a case before; gap = t0 of
    the case minus the step count at which the previous tenant's episode ended (0: it ended in the move right before the
    seat)."""
    out = []
    for c in np.argsort(t0, kind='stable'):
        before = [p for p in range(len(t0)) if slot[p] == slot[c] and t0[p] < t0[c]]
        if before:
            p = max(before, key=lambda q: t0[q])
            out.append((int(c), int(p), int(t0[c] - (t0[p] + lived[p]))))
    return out
