"""TEST INFRASTRUCTURE ONLY: the shared case tables of streamed rollouts of LARGE teams
(include/gnnpp_rollout_team_stream.h), run under the host emulation (tests/test_emu_rollout_team_stream.py) and on the device
(tests/test_gpu_rollout_team_stream_cases.py), on the dense graph and on the neighbour lists.

The driver (`run_stream`), the seating prediction (`expected_seating`), `plain_expectation` and the assertions are those of
tests/rollout_stream_cases.py, imported, not restated; so is the random table builder.  A table here carries its own
`commR`.  The engine interface is the one described there; with the lists graph, read('S') returns `lists_slots` of the
block: one row of bytes per slot, so the driver's byte comparisons apply unchanged.

Shapes, the smallest at which these kernels can still go wrong: N = 129 (three waves, 63 idle lanes in the last), 192 (an
exact multiple of the wave), 257; a shared 20 x 20 map and per-case 21 x 19 maps (399 cells: the byte-copy path of the map,
an LDS map rounded to 16 bytes); 5 - 9 cases through 2 - 3 slots, C < slots and C = slots; reseat_every 1 and 4; commR 6.0
and a table at commR 1.0 whose seats multiply the radius many times."""
import functools

import numpy as np

import rollout_stream_cases as sc
from rollout_stream_cases import (STAY, TABLE_KEYS, assert_seats, assert_tables, batched, expected_seating,  # noqa: F401
                                  plain_actions, plain_expectation, run_stream, script_actions)


def _table(name, seed, C, N, H, W, slots, every, per_case, commR=6.0, hi=5):
    t = dict(sc._random_table(name, seed, C, N, H, W, slots, every, per_case, lo=2, hi=hi))
    t['commR'] = commR
    return t


@functools.lru_cache(None)
def first_table():
    """N = 129 on one shared map, 9 cases through 3 slots.  Case 5 'never_moves': nobody ever asks to move and nobody stands
    on its goal, so the episode ends at its limit with every start_step written as 0 by the move kernel."""
    t = _table('n129_20x20_shared', 129, 9, 129, 20, 20, 3, 1, False)
    t['scripts'][5] = STAY
    t['maxstep'][5] = 3
    assert (t['starts'][5] != t['goals'][5]).any(axis=1).all()
    t['named'] = {'never_moves': 5}
    return t


@functools.lru_cache(None)
def hand_table():
    """N = 129 on one shared, empty 20 x 20 map, 5 cases through 2 slots; cases 0 .. 3 run to their limit of 4, so case 4
    is seated at t0 = 8.

    case 4 'one_walker': agents 0 and 2 .. 128 start ON their goals (cell (n // 16, n % 16)) and only ever stay; agent 1
        walks (19,0) -> (19,3) over three free cells.  By the move rule (tests/rollout_stream_cases.py, case 5 of the 6 x 6
        table) step 1 counts every staying agent's arrival (end 1; it never asked to move: start -1, counted as 0) and agent
        1 arrives at step 3 having asked at step 1 (start 0).  makespan = max end - min start = 3 - 0 = 3, flowtime =
        128 * (1 - 0) + (3 - 0) = 131, and the call of step 4 ends the loop: lived 4.  Read from r->stats in a slot seated at
        t0 the flowtime is 128 * (t0 + 1) + 3: wrong by 128 t0."""
    C, N, L = 5, 129, 4
    rng = np.random.default_rng(29)
    grids = np.zeros((20, 20), np.uint8)
    starts = np.zeros((C, N, 2), np.int32)
    goals = np.zeros((C, N, 2), np.int32)
    scripts = rng.integers(0, 5, size=(C, L, N)).astype(np.int32)
    for c in range(C):
        starts[c] = sc._cells(rng, grids, N)
        goals[c] = sc._cells(rng, grids, N)
    maxstep = np.full(C, 4, np.int32)
    n = np.arange(N)
    starts[4] = np.stack([n // 16, n % 16], 1)
    starts[4, 1] = [19, 0]
    goals[4] = starts[4]
    goals[4, 1] = [19, 3]
    scripts[4] = STAY
    scripts[4, :3, 1] = 3
    maxstep[4] = 9
    start_step = np.full(N, -1, np.int32)
    start_step[1] = 0
    end_step = np.ones(N, np.int32)
    end_step[1] = 3
    return {'name': 'hand_n129_20x20', 'grids': grids, 'starts': starts, 'goals': goals, 'maxstep': maxstep,
            'scripts': scripts, 'slots': 2, 'reseat_every': 1, 'commR': 6.0, 'named': {'one_walker': 4},
            'hand': {4: {'makespan': 3, 'flowtime': 131, 'lived': 4, 'start_step': start_step, 'end_step': end_step}}}


@functools.lru_cache(None)
def tables():
    return [
        first_table(),
        hand_table(),
        _table('n129_21x19_every4', 130, 7, 129, 21, 19, 2, 4, True),
        _table('n192_21x19', 192, 6, 192, 21, 19, 2, 1, True),
        _table('n257_20x20_shared_every4', 257, 6, 257, 20, 20, 2, 4, False),
        _table('growth_n129_commR1', 131, 6, 129, 20, 20, 2, 1, False, commR=1.0),
        _table('c2_lt_slots_n129', 132, 2, 129, 21, 19, 3, 1, True),               # C < slots: two slots in all
        _table('c3_eq_slots_n129', 133, 3, 129, 20, 20, 3, 4, False),              # C = slots: nothing is ever reseated
    ]


TABLE_NAMES = ('n129_20x20_shared', 'hand_n129_20x20', 'n129_21x19_every4', 'n192_21x19', 'n257_20x20_shared_every4',
               'growth_n129_commR1', 'c2_lt_slots_n129', 'c3_eq_slots_n129')
GRAPHS = ('dense', 'lists')


def table(name):
    return tables()[TABLE_NAMES.index(name)]


def lists_bytes(graphs, N):
    """Size of a lists block (cnt | idx | val, each section rounded up to 16 bytes): gnnpp_team_lists_bytes."""
    Np = (N + 3) & ~3
    up = lambda v: (v + 15) & ~15                                                        # noqa: E731
    return up(graphs * N * 4) + up(graphs * N * Np * 2) + up(graphs * N * Np * 4)


def lists_slots(block, graphs, N):
    """[graphs, bytes] uint8: each graph's columns of a lists block (numpy uint8) in one row -- its counts, then its indices
    and its weights (as bits) with everything behind a column's last written group of four zeroed: a list is written up to
    its count rounded up to 4, what lies behind is nobody's."""
    Np = (N + 3) & ~3
    up = lambda v: (v + 15) & ~15                                                        # noqa: E731
    block = np.ascontiguousarray(block)
    idx_o = up(graphs * N * 4)
    val_o = idx_o + up(graphs * N * Np * 2)
    cnt = block[:graphs * N * 4].view(np.int32).reshape(graphs, N)
    idx = block[idx_o:idx_o + graphs * N * Np * 2].view(np.uint16).reshape(graphs, N, Np)
    val = block[val_o:val_o + graphs * N * Np * 4].view(np.uint32).reshape(graphs, N, Np)
    live = np.arange(Np)[None, None, :] < ((np.clip(cnt, 0, N) + 3) & ~3)[:, :, None]   # (a slot never written: any bytes)
    parts = [cnt, np.where(live, idx, 0).astype(np.uint16), np.where(live, val, 0).astype(np.uint32)]
    return np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(graphs, -1) for a in parts], 1)
