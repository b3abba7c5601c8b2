"""TEST INFRASTRUCTURE ONLY: the shared case table of streamed rollouts (include/gnnpp_rollout_stream.h).  Each table is
defined once here and run under the host emulation (tests/test_emu_rollout_stream.py) and on the device
(tests/test_gpu_rollout_stream_cases.py), through one driver over a small `engine` interface.

A table is a queue of C cases of one shape, a slot count and a reseat period.  Every case carries a SCRIPT: the action
every agent asks for at each step of its own episode.  The driver gathers each slot's action from the case it holds and
the step count at which that case was seated.  The expected value of every case is the PLAIN per-case rollout of the same
script (gnnpp_rollout_* with B = C, per-case maxstep, tie mode 'lowest': the path the simulator's own traces pin down),
and two tiny cases carry makespan and flowtime derived by hand below, so the table is not only self-referential.  The
seating order is predicted by a few lines of Python from the expected episode lengths alone (`expected_seating`).

engine:  B, C, N; reseat(now); move(actions [B,N] int32, step); read(name) -> numpy copy of a slot array ('case', 't0',
         'assign', 'done', 'cursor', 'obs', 'S', 'radius', 'pos', 'goal', 'reached', 'start_step', 'end_step', 'maxstep',
         and 'grid' when maps are per case); tables() -> dict of the per-case result tables as numpy arrays."""
import functools

import numpy as np

STAY = 4
COMM_R = 6.0
TABLE_KEYS = ('reached', 'start_step', 'end_step', 'pos', 'radius', 'makespan', 'flowtime', 'lived')
SLOT_STATE = ('obs', 'S', 'radius', 'pos', 'goal', 'reached', 'start_step', 'end_step', 'maxstep')


def _cells(rng, grid, count):
    free = np.argwhere(grid == 0)
    return free[rng.choice(len(free), count, replace=False)]


def _random_table(name, seed, C, N, H, W, slots, reseat_every, batched, density=0.08, lo=2, hi=12):
    """Random maps, starts, goals, scripts and limits lo .. hi; every third case starts on its goals and only stays (an
    episode of two steps), so lengths differ widely."""
    rng = np.random.default_rng(seed)
    grids = (rng.random((C, H, W)) < density).astype(np.uint8) if batched else \
        (rng.random((H, W)) < density).astype(np.uint8)
    starts = np.zeros((C, N, 2), np.int32)
    goals = np.zeros((C, N, 2), np.int32)
    maxstep = rng.integers(lo, hi + 1, size=C).astype(np.int32)
    scripts = rng.integers(0, 5, size=(C, hi, N)).astype(np.int32)
    for c in range(C):
        g = grids[c] if batched else grids
        starts[c] = _cells(rng, g, N)
        goals[c] = _cells(rng, g, N)
        if c % 3 == 1:
            goals[c] = starts[c]
            scripts[c] = STAY
            maxstep[c] = hi
    return {'name': name, 'grids': grids, 'starts': starts, 'goals': goals, 'maxstep': maxstep, 'scripts': scripts,
            'slots': slots, 'reseat_every': reseat_every, 'hand': {}, 'named': {}}


def _walk(script, c, n, moves):
    script[c, :len(moves), n] = moves


@functools.lru_cache(None)
def hand_table_6x6():
    """N = 2 on one shared, empty 6 x 6 map, 9 cases through 3 slots.  Cases 0 .. 2 are long (limit 9, never arrive), so
    the named cases below are all seated at t0 > 0.

    case 5 'stays_on_goal': agent 0 starts ON its goal (1,1) and only ever stays; agent 1 walks (2,0) -> (2,3) in three
        steps.  Step 1 counts agent 0's arrival (end 1; it never asked to move: start -1, counted as 0), agent 1 arrives
        at step 3 having asked at step 1 (start 0).  makespan = max end - min start = 3 - 0 = 3, flowtime = (1 - 0) +
        (3 - 0) = 4, and the call of step 4 ends the loop: lived 4.  Read from r->stats in a slot seated at t0 the
        flowtime is (t0 + 1 - 0) + 3: wrong by t0.
    case 6 'never_moved': limit 3; agent 0 never asks to move and is not on its goal, agent 1 steps right once and back.
        At the limit both get end = 3; agent 0's missing start is written as 0 by the move kernel.  makespan = 3 - 0 = 3,
        flowtime = (3 - 0) + (3 - 0) = 6, lived 3.  The 0 is a GLOBAL step: relative it must stay 0, not go negative."""
    C, N, L = 9, 2, 9
    grids = np.zeros((6, 6), np.uint8)
    starts = np.zeros((C, N, 2), np.int32)
    goals = np.zeros((C, N, 2), np.int32)
    scripts = np.full((C, L, N), STAY, np.int32)
    maxstep = np.full(C, 9, np.int32)
    rng = np.random.default_rng(5)
    for c in range(C):
        starts[c] = [[0, 0], [5, 5]]
        goals[c] = [[5, 0], [0, 5]]
        scripts[c] = rng.integers(0, 5, size=(L, N))
        maxstep[c] = rng.integers(3, 8)
    for c in (0, 1, 2):                                      # long, never arrive: up and down along their columns
        scripts[c, :, 0] = [2, 0] * 4 + [2]
        scripts[c, :, 1] = [0, 2] * 4 + [0]
        maxstep[c] = 9
    starts[5], goals[5], maxstep[5] = [[1, 1], [2, 0]], [[1, 1], [2, 3]], 9
    scripts[5] = STAY
    _walk(scripts, 5, 1, [3, 3, 3])
    starts[6], goals[6], maxstep[6] = [[1, 1], [3, 0]], [[4, 4], [3, 5]], 3
    scripts[6] = STAY
    _walk(scripts, 6, 1, [3, 1])
    return {'name': 'hand_n2_6x6', 'grids': grids, 'starts': starts, 'goals': goals, 'maxstep': maxstep,
            'scripts': scripts, 'slots': 3, 'reseat_every': 1, 'named': {'stays_on_goal': 5, 'never_moved': 6},
            'hand': {5: {'makespan': 3, 'flowtime': 4, 'lived': 4, 'start_step': [-1, 0], 'end_step': [1, 3]},
                     6: {'makespan': 3, 'flowtime': 6, 'lived': 3, 'start_step': [0, 0], 'end_step': [3, 3]}}}


@functools.lru_cache(None)
def corridor_table():
    """Two agents in a 1 x 5 corridor, 8 cases through 3 slots, reseat every 4 steps.

    case 7 'corridor': agent 0 walks (0,0) -> (0,2), agent 1 (0,4) -> (0,3).  Step 1: agent 1 arrives (end 1), step 2:
        agent 0 arrives (end 2); both asked at step 1 (start 0).  makespan = 2 - 0 = 2, flowtime = (2 - 0) + (1 - 0) = 3,
        and the call of step 3 ends the loop: lived 3."""
    C, N, L = 8, 2, 7
    grids = np.zeros((1, 5), np.uint8)
    starts = np.tile(np.array([[0, 0], [0, 4]], np.int32), (C, 1, 1))
    goals = np.tile(np.array([[0, 4], [0, 0]], np.int32), (C, 1, 1))          # they block each other: never arrive
    rng = np.random.default_rng(15)
    scripts = rng.choice([1, 3, 4], size=(C, L, N)).astype(np.int32)
    maxstep = rng.integers(2, L + 1, size=C).astype(np.int32)
    goals[7], maxstep[7] = [[0, 2], [0, 3]], 7
    scripts[7] = STAY
    _walk(scripts, 7, 0, [3, 3])
    _walk(scripts, 7, 1, [1])
    return {'name': 'corridor_n2_1x5', 'grids': grids, 'starts': starts, 'goals': goals, 'maxstep': maxstep,
            'scripts': scripts, 'slots': 3, 'reseat_every': 4, 'named': {'corridor': 7},
            'hand': {7: {'makespan': 2, 'flowtime': 3, 'lived': 3, 'start_step': [0, 0], 'end_step': [2, 1]}}}


@functools.lru_cache(None)
def growth_table():
    """N = 3 on one shared, empty 24 x 24 map: the starts are far apart, so the radius search of a seat multiplies the
    radius several times before the graph is connected ('needs_growth': case 4, the widest, seated late)."""
    t = _random_table('growth_n3_24x24', 31, 8, 3, 24, 24, 3, 1, False, density=0.0, lo=2, hi=6)
    t['starts'][4] = [[0, 0], [0, 23], [23, 11]]
    t['starts'][5] = [[0, 0], [12, 12], [23, 23]]
    t['named'] = {'needs_growth': 4}
    return t


@functools.lru_cache(None)
def tables():
    return [
        _random_table('n1_6x6', 1, 8, 1, 6, 6, 3, 1, True),
        hand_table_6x6(),
        corridor_table(),
        _random_table('n4_6x6_every4', 4, 10, 4, 6, 6, 3, 4, True, lo=2, hi=14),
        _random_table('n33_12x12', 33, 8, 33, 12, 12, 3, 1, True, hi=8),            # beyond fused_sim_max_agents
        _random_table('n65_16x16_shared_every4', 65, 8, 65, 16, 16, 3, 4, False, hi=8),   # the wave's second half
        _random_table('n128_16x16', 128, 8, 128, 16, 16, 3, 1, True, hi=6),
        growth_table(),
        _random_table('c2_lt_slots', 2, 2, 4, 6, 6, 3, 1, True),                    # C < slots: two slots in all
        _random_table('c3_eq_slots', 3, 3, 4, 6, 6, 3, 4, False),                   # C = slots: nothing is ever reseated
    ]


TABLE_NAMES = ('n1_6x6', 'hand_n2_6x6', 'corridor_n2_1x5', 'n4_6x6_every4', 'n33_12x12', 'n65_16x16_shared_every4',
               'n128_16x16', 'growth_n3_24x24', 'c2_lt_slots', 'c3_eq_slots')


def table(name):
    return tables()[TABLE_NAMES.index(name)]


def batched(tab):
    return tab['grids'].ndim == 3


def script_actions(tab, case, t0, now):
    """[B,N] actions of the move at global step now + 1: slot b's case asks for row now - t0[b] of its script (a slot
    that is empty, or past its script, stays)."""
    scripts = tab['scripts']
    C, L, N = scripts.shape
    out = np.full((len(case), N), STAY, np.int32)
    for b, c in enumerate(case):
        k = now - int(t0[b])
        if c >= 0 and 0 <= k < L:
            out[b] = scripts[c, k]
    return out


def plain_expectation(plain):
    """plain: the plain per-case rollout's read-backs -- dict(reached, start_step, end_step, pos [C,N,..], stats [C,2],
    radius [C], frozen [T,C] = the episode was frozen at entry of move t + 1) -> the per-case tables a stream must hold."""
    return {'reached': plain['reached'], 'start_step': plain['start_step'], 'end_step': plain['end_step'],
            'pos': plain['pos'], 'radius': plain['radius'], 'makespan': plain['stats'][:, 0],
            'flowtime': plain['stats'][:, 1], 'lived': (~np.asarray(plain['frozen'], bool)).sum(0).astype(np.int32)}


def plain_actions(tab, t):
    """[C,N] actions of the plain rollout's move t + 1 (every case is seated at 0)."""
    C = tab['scripts'].shape[0]
    return script_actions(tab, np.arange(C), np.zeros(C, np.int64), t)


def expected_seating(tab, lived):
    """(slot [C], t0 [C]) by the prefix rule: at every reseat (step counts that are multiples of reseat_every) the free
    slots, in slot order, take the next cases of the queue; a case seated at t0 that lives `lived` moves has ended when
    the step count reaches t0 + lived."""
    C = len(lived)
    B, every = min(tab['slots'], C), tab['reseat_every']
    free_at = [0] * B
    slot, t0 = np.full(C, -1, np.int32), np.full(C, -1, np.int32)
    cursor, now = 0, 0
    while cursor < C:
        for b in range(B):
            if cursor < C and free_at[b] <= now:
                slot[cursor], t0[cursor] = b, now
                free_at[b] = now + int(lived[cursor])
                cursor += 1
        now += every
    return slot, t0


def run_stream(eng, tab, fresh=None):
    """Drive an engine through a table.  fresh: None, or dict(obs, S, radius [C,...]) of every case's step 0 alone; then a
    freshly seated slot must hold exactly that, and a slot the reseat gave nothing must keep its bytes.  Returns
    (tables, seats) with seats = [(now, slot, case), ...] in the order they happened."""
    C, every = eng.C, tab['reseat_every']
    now, seats = 0, []
    bound = int(tab['maxstep'].sum()) + (C + 1) * every + 8
    state = SLOT_STATE + (('grid',) if batched(tab) else ())
    while True:
        if now % every == 0:
            before = {k: eng.read(k) for k in state} if fresh is not None else None
            done_before = eng.read('done') != 0
            eng.reseat(now)
            assign = eng.read('assign')
            assert ((assign >= 0) <= done_before).all(), 'a live slot was given a case'
            for b in np.flatnonzero(assign >= 0):
                seats.append((now, int(b), int(assign[b])))
            if fresh is not None:
                after = {k: eng.read(k) for k in state}
                for b, c in enumerate(assign):
                    if c >= 0:
                        for k in ('obs', 'S', 'radius'):
                            assert after[k][b].tobytes() == np.ascontiguousarray(fresh[k][c]).tobytes(), \
                                (tab['name'], 'seat', k, now, b, c)
                        assert np.array_equal(after['pos'][b], tab['starts'][c]) and \
                            np.array_equal(after['goal'][b], tab['goals'][c]) and \
                            after['maxstep'][b] == now + tab['maxstep'][c], (tab['name'], now, b, c)
                        if batched(tab):
                            assert np.array_equal(after['grid'][b], tab['grids'][c]), (tab['name'], 'map', now, b, c)
                    else:
                        for k in state:
                            assert after[k][b].tobytes() == before[k][b].tobytes(), (tab['name'], 'kept', k, now, b)
        if int(eng.read('cursor')[0]) >= C and (eng.read('done') != 0).all():
            break
        eng.move(script_actions(tab, eng.read('case'), eng.read('t0'), now), now + 1)
        now += 1
        assert now <= bound, 'the queue does not drain'
    eng.reseat(now)                                          # the final harvest (nothing left to seat)
    assert (eng.read('case') == -1).all() and (eng.read('assign') == -1).all()
    return eng.tables(), seats


def assert_tables(tab, got, want):
    """Every per-case table exactly, the hand-derived values, and the seating order."""
    for k in TABLE_KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (tab['name'], k, got[k], want[k])
    for c, hand in tab['hand'].items():
        for k, v in hand.items():
            assert np.array_equal(np.asarray(got[k][c]), np.asarray(v)), (tab['name'], 'hand', c, k, got[k][c], v)
    slot, t0 = expected_seating(tab, want['lived'])
    assert np.array_equal(got['slot'], slot) and np.array_equal(got['t0'], t0), (tab['name'], got['slot'], slot, got['t0'], t0)
    if len(want['lived']) >= 8:
        assert all((t0[slot == b] > 0).any() for b in range(tab['slots'])), (tab['name'], 'a slot was never reseated')


def assert_seats(tab, seats, got):
    """The log of the reseats is the prefix rule: cases in queue order, slots ascending inside one reseat, and it agrees
    with the tables' slot / t0 columns."""
    assert [c for (_, _, c) in seats] == list(range(len(got['slot'])))
    for (n0, b0, _), (n1, b1, _) in zip(seats, seats[1:]):
        assert n1 > n0 or (n1 == n0 and b1 > b0), seats
    for now, b, c in seats:
        assert got['slot'][c] == b and got['t0'][c] == now
