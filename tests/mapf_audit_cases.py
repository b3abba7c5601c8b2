"""Yardstick of the schedule audit (include/gnnpp_mapf_audit.h, csrc/mapf_audit_kernels.hip, mapf.audit): a SEQUENTIAL
numpy restatement of the header's contract -- one case, one layer, one agent at a time, with Python dicts where the kernel
has its owner table; written from the header, not from the kernel -- and the table of named calls that the host emulation
(tests/test_emu_mapf_audit.py) and the device (tests/test_gpu_mapf_audit.py) both run.

A case is one call: dict(name, grid [H,W] | [C,H,W] uint8, start [C,N,2] | None, goal [C,N,2], schedule [C,T+1,N,2] int32,
steps [C] int32 | None, facts).  facts(want) asserts what the restatement must answer for the case to be the edge case its
name says.  run(call, name) makes the call twice on poisoned outputs and compares every element with the restatement, and
the two calls' bytes with each other; `call(case, out)` fills the poisoned host arrays of `out`.
"""
import numpy as np

import mapf_cases as mc

CHUNK = 32                                               # GNNPP_MAPF_AUDIT_CHUNK (test_mapf_audit_abi.py holds them equal)
STATE, VERTEX, MOVE, SWAP, BAD_START, NOT_AT_GOAL, SKIPPED = 1, 2, 4, 8, 16, 32, 64
C_STATE, C_VERTEX, C_MOVE, C_SWAP = 0, 1, 2, 3
POISON = -7
OUTPUTS = ('status', 'arrival', 'makespan', 'flowtime', 'counts', 'first')
FIVE = {(-1, 0), (0, -1), (1, 0), (0, 1), (0, 0)}


# ---- the contract, restated ------------------------------------------------------------------------------------------
def audit_one(grid, start, goal, sched, steps, T_max):
    """One case: grid [H,W], start [N,2] | None, goal [N,2], sched [T_max+1,N,2], steps int | None -> dict of OUTPUTS."""
    N = sched.shape[1]
    L = T_max if steps is None else int(steps)
    if L < 0:
        return {'status': SKIPPED, 'arrival': np.full(N, -1), 'makespan': -1, 'flowtime': -1, 'counts': np.full(4, -1),
                'first': np.full(4, -1)}
    L = min(L, T_max)
    H, W = grid.shape
    pos = [[(int(sched[t, i, 0]), int(sched[t, i, 1])) for i in range(N)] for t in range(L + 1)]
    flagged, others, dirty = [], {}, []
    for t in range(L + 1):
        bad = [i for i, (x, y) in enumerate(pos[t]) if not (0 <= x < H and 0 <= y < W) or grid[x, y] != 0]
        if bad:
            flagged += [(t, C_STATE, i) for i in bad]
            dirty.append(True)
            continue
        at = {}
        for i, p in enumerate(pos[t]):
            at.setdefault(p, []).append(i)
        shared = [i for i, p in enumerate(pos[t]) if len(at[p]) > 1]
        for i in shared:
            flagged.append((t, C_VERTEX, i))
            others[(t, C_VERTEX, i)] = min(j for j in at[pos[t][i]] if j != i)
        dirty.append(bool(shared))
    for t in range(L):
        if dirty[t] or dirty[t + 1]:
            continue
        jumps = [i for i in range(N) if (pos[t + 1][i][0] - pos[t][i][0], pos[t + 1][i][1] - pos[t][i][1]) not in FIVE]
        if jumps:
            flagged += [(t, C_MOVE, i) for i in jumps]
            continue
        for i in range(N):
            if pos[t + 1][i] == pos[t][i]:
                continue
            swaps = [j for j in range(N) if j != i and pos[t][j] == pos[t + 1][i] and pos[t + 1][j] == pos[t][i]]
            if swaps:
                flagged.append((t, C_SWAP, i))
                others[(t, C_SWAP, i)] = min(swaps)
    counts = np.zeros(4, dtype=np.int64)
    for _, cls, _ in flagged:
        counts[cls] += 1
    first = np.full(4, -1)
    if flagged:
        f = min(flagged)
        first = np.array([f[0], f[1], f[2], others.get(f, -1)])
    arrival = np.full(N, -1)
    for i in range(N):
        g = (int(goal[i, 0]), int(goal[i, 1]))
        t = L + 1
        while t > 0 and pos[t - 1][i] == g:
            t -= 1
        arrival[i] = t if t <= L else -1
    status = sum(1 << cls for cls in range(4) if counts[cls])
    if start is not None and any(pos[0][i] != (int(start[i, 0]), int(start[i, 1])) for i in range(N)):
        status |= BAD_START
    away = bool((arrival < 0).any())
    if away:
        status |= NOT_AT_GOAL
    return {'status': status, 'arrival': arrival, 'makespan': -1 if away else int(arrival.max()),
            'flowtime': -1 if away else int(arrival.sum()), 'counts': counts, 'first': first}


def audit(case):
    """The call's outputs [C, ...] as int64 arrays."""
    C = case['schedule'].shape[0]
    T_max = case['schedule'].shape[1] - 1
    one = [audit_one(case['grid'] if case['grid'].ndim == 2 else case['grid'][c],
                     None if case['start'] is None else case['start'][c], case['goal'][c], case['schedule'][c],
                     None if case['steps'] is None else case['steps'][c], T_max) for c in range(C)]
    return {k: np.stack([np.asarray(o[k], dtype=np.int64) for o in one]) for k in OUTPUTS}


# ---- cases -----------------------------------------------------------------------------------------------------------
CASES = {}
_WANTS = {}


def make_case(name, grid, goal, schedule, start='row0', steps=None, facts=None):
    schedule = np.asarray(schedule, dtype=np.int32)
    if schedule.ndim == 3:
        schedule = schedule[None]
    goal = np.asarray(goal, dtype=np.int32).reshape(schedule.shape[0], schedule.shape[2], 2)
    if isinstance(start, str):
        start = schedule[:, 0].copy()
    elif start is not None:
        start = np.asarray(start, dtype=np.int32).reshape(goal.shape)
    return {'name': name, 'grid': np.ascontiguousarray(grid, dtype=np.uint8), 'start': start,
            'goal': np.ascontiguousarray(goal), 'schedule': np.ascontiguousarray(schedule),
            'steps': None if steps is None else np.asarray(steps, dtype=np.int32), 'facts': facts}


def _case(name=None):
    def deco(fn):
        key = name or fn.__name__
        CASES[key] = lambda: fn(key)
        return fn
    return deco


def _every(stem, params, label):
    def deco(fn):
        for prm in params:
            key = '%s_%s' % (stem, label(*prm))
            CASES[key] = (lambda key=key, prm=prm: fn(key, *prm))
        return fn
    return deco


def wants_of(name):
    if name not in _WANTS:
        case = CASES[name]()
        want = audit(case)
        if case['facts'] is not None:
            case['facts'](want)
        _WANTS[name] = (case, want)
    return _WANTS[name]


def poisoned(C, N):
    return {'status': np.full(C, POISON, np.int32), 'arrival': np.full((C, N), POISON, np.int32),
            'makespan': np.full(C, POISON, np.int32), 'flowtime': np.full(C, POISON, np.int32),
            'counts': np.full((C, 4), POISON, np.int32), 'first': np.full((C, 4), POISON, np.int32)}


def assert_equal(name, out, want):
    for k in OUTPUTS:
        got = np.asarray(out[k])
        assert got.shape == want[k].shape, (name, k, got.shape, want[k].shape)
        if not np.array_equal(got, want[k]):
            c = int(np.nonzero((got != want[k]).reshape(len(got), -1).any(1))[0][0])
            raise AssertionError('%s: %s of case %d is %s, the restatement says %s' % (name, k, c, got[c], want[k][c]))


def run(call, name):
    """The named call, twice, each time on poisoned outputs: equal to the restatement, and the same bytes both times."""
    case, want = wants_of(name)
    C, _, N, _ = case['schedule'].shape
    a, b = poisoned(C, N), poisoned(C, N)
    call(case, a)
    assert_equal(name, a, want)
    call(case, b)
    for k in OUTPUTS:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (name, k)
    return a


# ---- builders ---------------------------------------------------------------------------------------------------------
def walkers(N, T, W=None):
    """A clean plan on an open map of 2 N rows: agent i walks right along row 2 i, one cell per step.  (grid, sched)."""
    W = W or T + 4
    sched = np.zeros((T + 1, N, 2), dtype=np.int64)
    sched[:, :, 0] = 2 * np.arange(N)[None]
    sched[:, :, 1] = np.arange(T + 1)[:, None]
    return np.zeros((2 * N, W), np.uint8), sched


def pacers(N, T, H, W, cells=None):
    """A clean plan of any length on a map of a few cells: agent i stands on cell `cells[i]` (default i) of an open H x W
    map and never moves.  (grid, sched)."""
    q = np.arange(N) if cells is None else np.asarray(cells)
    sched = np.zeros((T + 1, N, 2), dtype=np.int64)
    sched[:, :, 0] = (q // W)[None]
    sched[:, :, 1] = (q % W)[None]
    return np.zeros((H, W), np.uint8), sched


def counts_are(*counts, first=None, status=None):
    def facts(want):
        assert want['counts'][0].tolist() == list(counts), want['counts'][0]
        if first is not None:
            assert want['first'][0].tolist() == list(first), want['first'][0]
        if status is not None:
            assert int(want['status'][0]) == status, want['status'][0]
    return facts


# ---- clean plans of the yardstick solver ---------------------------------------------------------------------------------
def _solved_set(name, seed, count, N, H, W):
    cases = mc.random_cases(np.random.default_rng(seed), count, N, H, W, density=0.15)
    T = mc.default_horizon(H, W)
    sols = [mc.solve_case(g, s, gl, T) for g, s, gl in cases]

    def facts(want):
        assert any(s['status'] == 0 for s in sols)
        for c, s in enumerate(sols):
            if s['status'] != 0:
                assert int(want['status'][c]) == SKIPPED
                continue
            assert int(want['status'][c]) == 0 and (want['counts'][c] == 0).all() and (want['first'][c] == -1).all()
            assert np.array_equal(want['arrival'][c], s['arrival'])
            assert (int(want['makespan'][c]), int(want['flowtime'][c])) == (s['makespan'], s['flowtime'])
            g, st, gl = cases[c]
            mc.check_plans(g, st, gl, s['schedule'][:s['makespan'] + 1], s['arrival'])      # the two validators agree
    return make_case(name, np.stack([c[0] for c in cases]), np.stack([c[2] for c in cases]),
                     np.stack([s['schedule'] for s in sols]), start=np.stack([c[1] for c in cases]),
                     steps=[s['makespan'] for s in sols], facts=facts)


@_every('solver_plans', [(101, 6, 5, 10, 10), (102, 5, 8, 10, 10), (103, 5, 6, 7, 13)],
        lambda seed, count, N, H, W: '%dx%d_N%d' % (H, W, N))
def solver_plans(name, seed, count, N, H, W):
    return _solved_set(name, seed, count, N, H, W)


# ---- one offence of each class, at t = 0, in the middle and at L ------------------------------------------------------
T_ONE = 8
WHEN = [(0,), (4,), (T_ONE,)]


@_every('state_off_the_map', [(t, side) for (t,) in WHEN for side in ('up', 'down', 'left', 'right')],
        lambda t, side: '%s_t%d' % (side, t))
def state_off_the_map(name, t, side):
    grid, sched = walkers(3, T_ONE)
    H, W = grid.shape
    sched[t, 1] = {'up': (-1, 3), 'down': (H, 3), 'left': (2, -1), 'right': (2, W)}[side]
    return make_case(name, grid, sched[T_ONE], sched, start=walkers(3, T_ONE)[1][0],
                     facts=counts_are(1, 0, 0, 0, first=(t, C_STATE, 1, -1)))


@_every('state_on_an_obstacle', WHEN, lambda t: 't%d' % t)
def state_on_an_obstacle(name, t):
    grid, sched = walkers(3, T_ONE)
    grid[3, 5] = 1
    sched[t, 2] = (3, 5)
    return make_case(name, grid, sched[T_ONE], sched, facts=counts_are(1, 0, 0, 0, first=(t, C_STATE, 2, -1)))


@_every('vertex', WHEN, lambda t: 't%d' % t)
def vertex(name, t):
    grid, sched = walkers(3, T_ONE)
    sched[t, 2] = sched[t, 0]
    return make_case(name, grid, sched[T_ONE], sched, facts=counts_are(0, 2, 0, 0, first=(t, C_VERTEX, 0, 2)))


@_every('move', [(t, kind) for t in (0, 4, T_ONE - 1) for kind in ('diagonal', 'jump2')], lambda t, kind: '%s_t%d' % (kind, t))
def move(name, t, kind):
    """The transition t -> t + 1 of agent 1 is a diagonal step / a jump of two cells; every later position follows."""
    grid, sched = walkers(3, T_ONE)
    sched[t + 1:, 1] += (1, 0) if kind == 'diagonal' else (0, 1)
    return make_case(name, grid, sched[T_ONE], sched, facts=counts_are(0, 0, 1, 0, first=(t, C_MOVE, 1, -1), status=MOVE))


def _swap_case(name, H, W, a, b, t, T=T_ONE, extra=()):
    """Agents 0 and 1 stand on the adjacent cells a and b and exchange them on the transition t -> t + 1."""
    sched = np.zeros((T + 1, 2 + len(extra), 2), dtype=np.int64)
    sched[:t + 1, 0], sched[:t + 1, 1] = a, b
    sched[t + 1:, 0], sched[t + 1:, 1] = b, a
    for n, cell in enumerate(extra):
        sched[:, 2 + n] = cell
    return make_case(name, np.zeros((H, W), np.uint8), sched[T], sched,
                     facts=counts_are(0, 0, 0, 2, first=(t, C_SWAP, 0, 1), status=SWAP))


@_every('swap', [(t, way) for t in (0, 4, T_ONE - 1) for way in ('horizontal', 'vertical')], lambda t, way: '%s_t%d' % (way, t))
def swap(name, t, way):
    b = (2, 3) if way == 'horizontal' else (3, 2)
    return _swap_case(name, 5, 5, (2, 2), b, t, extra=[(0, 0)])


@_case()
def swap_on_the_1x2_map(name):
    return _swap_case(name, 1, 2, (0, 0), (0, 1), 1, T=3)


@_case()
def swap_across_columns_63_64_of_the_1x66_strip(name):
    return _swap_case(name, 1, 66, (0, 63), (0, 64), 2, T=4, extra=[(0, 0), (0, 65)])


# ---- not offences ------------------------------------------------------------------------------------------------------
@_case()
def following_into_a_vacated_cell(name):
    sched = np.zeros((5, 3, 2), dtype=np.int64)
    for i in range(3):                                   # a train on row 1: cells 2 - i + t
        sched[:, i, 0] = 1
        sched[:, i, 1] = 2 - i + np.arange(5)
    return make_case(name, np.zeros((3, 8), np.uint8), sched[4], sched, facts=counts_are(0, 0, 0, 0, status=0))


@_case()
def rotation_of_four_round_a_block(name):
    ring = [(0, 0), (0, 1), (1, 1), (1, 0)]
    sched = np.array([[ring[(i + t) % 4] for i in range(4)] for t in range(6)])
    return make_case(name, np.zeros((2, 2), np.uint8), sched[5], sched, facts=counts_are(0, 0, 0, 0, status=0))


@_case()
def agent_steps_off_its_goal_and_comes_back(name):
    path0 = [(0, 0), (0, 1), (0, 2), (0, 2), (0, 3), (0, 2), (0, 2)]     # on its goal (0, 2) at 2 and 3, for good at 5
    sched = np.zeros((7, 2, 2), dtype=np.int64)
    sched[:, 0] = path0
    sched[:, 1] = (2, 2)

    def facts(want):
        assert want['arrival'][0].tolist() == [5, 0] and int(want['makespan'][0]) == 5 and int(want['flowtime'][0]) == 5
        assert int(want['status'][0]) == 0
    return make_case(name, np.zeros((3, 5), np.uint8), [(0, 2), (2, 2)], sched, facts=facts)


# ---- shielding -----------------------------------------------------------------------------------------------------------
@_case()
def state_layer_with_a_duplicate_cell_counts_no_vertex(name):
    grid, sched = walkers(3, T_ONE)
    sched[3, 0] = (-1, 0)
    sched[3, 2] = sched[3, 1]
    return make_case(name, grid, sched[T_ONE], sched, facts=counts_are(1, 0, 0, 0, first=(3, C_STATE, 0, -1), status=STATE))


@_case()
def vertex_layer_followed_by_a_jump_counts_no_move(name):
    grid, sched = walkers(3, T_ONE)
    sched[3, 2] = sched[3, 1]                            # agent 2 jumps onto agent 1 and back: two jumps, both shielded
    return make_case(name, grid, sched[T_ONE], sched, facts=counts_are(0, 2, 0, 0, first=(3, C_VERTEX, 1, 2), status=VERTEX))


@_case()
def jump_that_is_also_a_swap_is_a_move_only(name):
    sched = np.zeros((4, 3, 2), dtype=np.int64)
    sched[:2, 0], sched[:2, 1] = (0, 0), (0, 2)
    sched[2:, 0], sched[2:, 1] = (0, 2), (0, 0)
    sched[:, 2] = (1, 1)
    return make_case(name, np.zeros((2, 3), np.uint8), sched[3], sched,
                     facts=counts_are(0, 0, 2, 0, first=(1, C_MOVE, 0, -1), status=MOVE))


@_case()
def move_flag_shields_a_swap_of_other_agents(name):
    """Agents 0 and 1 swap on the transition where agent 2 jumps: the transition holds a MOVE flag, no SWAP is counted."""
    sched = np.zeros((3, 3, 2), dtype=np.int64)
    sched[:2, 0], sched[:2, 1], sched[:2, 2] = (0, 0), (0, 1), (2, 0)
    sched[2:, 0], sched[2:, 1], sched[2:, 2] = (0, 1), (0, 0), (2, 3)
    return make_case(name, np.zeros((3, 4), np.uint8), sched[2], sched,
                     facts=counts_are(0, 0, 1, 0, first=(1, C_MOVE, 2, -1), status=MOVE))


# ---- race independence: many agents on one cell ------------------------------------------------------------------------
CROWDS = [(3,), (64,), (65,), (1024,)]


@_every('crowd_on_one_cell', CROWDS, lambda n: 'N%d' % n)
def crowd_on_one_cell(name, n):
    """Layer 1: all n agents on the cell of the LAST agent (the emulation's race winner is the highest thread, the
    device's is anybody): counts n, the first pair is (1, VERTEX, 0, 1)."""
    grid, sched = pacers(n, 2, 32, 33)
    sched[1] = sched[1, n - 1]
    return make_case(name, grid, sched[2], sched, facts=counts_are(0, n, 0, 0, first=(1, C_VERTEX, 0, 1), status=VERTEX))


@_every('two_crowded_cells', CROWDS, lambda n: 'N%d' % n)
def two_crowded_cells(name, n):
    """Layer 1: agent 0 alone; the odd agents on agent 1's cell, the even ones from 2 on agent 2's cell.  (Three agents
    make one crowd only: 1 and 2 together.)"""
    grid, sched = pacers(n, 2, 32, 33)
    if n == 3:
        sched[1, 2] = sched[1, 1]
        return make_case(name, grid, sched[2], sched, facts=counts_are(0, 2, 0, 0, first=(1, C_VERTEX, 1, 2)))
    sched[1, 1::2] = sched[1, 1]
    sched[1, 2::2] = sched[1, 2]
    return make_case(name, grid, sched[2], sched, facts=counts_are(0, n - 1, 0, 0, first=(1, C_VERTEX, 1, 3)))


# ---- seams ---------------------------------------------------------------------------------------------------------------
LENGTHS = [(0,), (1,), (CHUNK - 1,), (CHUNK,), (CHUNK + 1,), (2 * CHUNK,)]


@_every('clean_plan_of_length', LENGTHS, lambda L: 'L%d' % L)
def clean_plan_of_length(name, L):
    grid, sched = walkers(3, L)

    def facts(want):
        assert int(want['status'][0]) == 0 and want['arrival'][0].tolist() == [L] * 3
        assert int(want['makespan'][0]) == L and int(want['flowtime'][0]) == 3 * L
    return make_case(name, grid, sched[L], sched, facts=facts)


@_every('offence_at_the_last_row_of_length', LENGTHS, lambda L: 'L%d' % L)
def offence_at_the_last_row_of_length(name, L):
    """A vertex conflict on layer L, rows of garbage behind it in a longer buffer."""
    T = L + 3
    grid, sched = walkers(3, T, W=T + 6)
    sched[L, 2] = sched[L, 0]
    sched[L + 1:] = 10 ** 6
    return make_case(name, grid, sched[L], sched, steps=[L],
                     facts=counts_are(0, 2, 0, 0, first=(L, C_VERTEX, 0, 2)))


@_every('seam', [('state',), ('vertex',), ('move',), ('swap',)], lambda cls: cls)
def seam(name, cls):
    """An offence on the transition CHUNK - 1 -> CHUNK (MOVE, SWAP) or on layer CHUNK (STATE, VERTEX), counted once."""
    T = 2 * CHUNK + 1
    if cls == 'swap':
        case = _swap_case(name, 3, 3, (1, 1), (1, 2), CHUNK - 1, T=T, extra=[(0, 0)])
        return case
    grid, sched = walkers(3, T)
    if cls == 'state':
        sched[CHUNK, 1] = (-1, 0)
        facts = counts_are(1, 0, 0, 0, first=(CHUNK, C_STATE, 1, -1), status=STATE)
    elif cls == 'vertex':
        sched[CHUNK, 1] = sched[CHUNK, 0]
        facts = counts_are(0, 2, 0, 0, first=(CHUNK, C_VERTEX, 0, 1), status=VERTEX)
    else:
        sched[CHUNK:, 1] += (1, 0)
        facts = counts_are(0, 0, 1, 0, first=(CHUNK - 1, C_MOVE, 1, -1), status=MOVE)
    return make_case(name, grid, sched[T], sched, facts=facts)


@_case()
def offences_on_both_sides_of_a_seam(name):
    """A swap on CHUNK - 2 -> CHUNK - 1, a vertex conflict on layer CHUNK + 1, a jump on 2 CHUNK -> 2 CHUNK + 1: three
    chunks with one class each; the first pair is the swap's."""
    T = 2 * CHUNK + 2
    sched = np.zeros((T + 1, 4, 2), dtype=np.int64)
    sched[:, 0], sched[:, 1], sched[:, 2], sched[:, 3] = (0, 0), (0, 1), (2, 0), (2, 2)
    sched[CHUNK - 1:, 0], sched[CHUNK - 1:, 1] = (0, 1), (0, 0)
    sched[CHUNK + 1, 3] = (2, 0)
    sched[2 * CHUNK + 1:, 2] = (2, 4)
    return make_case(name, np.zeros((3, 5), np.uint8), sched[T], sched,
                     facts=counts_are(0, 2, 1, 2, first=(CHUNK - 2, C_SWAP, 0, 1), status=VERTEX | MOVE | SWAP))


@_every('last_step_off_the_goal', [(CHUNK - 1,), (CHUNK,)], lambda t: 't%d' % t)
def last_step_off_the_goal(name, t):
    T = 2 * CHUNK
    sched = np.zeros((T + 1, 2, 2), dtype=np.int64)
    sched[:, 1] = (2, 0)
    sched[:t + 1, 0] = (0, 1)                            # agent 0 waits next to its goal (0, 0) up to t

    def facts(want):
        assert want['arrival'][0].tolist() == [t + 1, 0] and int(want['status'][0]) == 0
    return make_case(name, np.zeros((3, 3), np.uint8), [(0, 0), (2, 0)], sched, facts=facts)


# ---- team sizes and maps -------------------------------------------------------------------------------------------------
@_every('team_of', [(1,), (2,), (63,), (64,), (65,), (1024,)], lambda n: 'N%d' % n)
def team_of(name, n):
    """n agents on an open 32 x 34 map, all stepping right at once and back; the last agent is off the map at t = 2."""
    grid, sched = pacers(n, 4, 32, 34, cells=np.arange(n) + np.arange(n) // 33)      # (column 33 stays empty)
    sched[1::2, :, 1] += 1
    sched[2, n - 1] = (-1, 0)
    return make_case(name, grid, sched[4], sched,
                     facts=counts_are(1, 0, 0, 0, first=(2, C_STATE, n - 1, -1), status=STATE))


@_case()
def one_by_one_map(name):
    sched = np.zeros((3, 1, 2), dtype=np.int64)
    return make_case(name, np.zeros((1, 1), np.uint8), [(0, 0)], sched, facts=counts_are(0, 0, 0, 0, status=0))


@_every('thin_map', [(1, 256), (256, 1)], lambda H, W: '%dx%d' % (H, W))
def thin_map(name, H, W):
    """Five agents along the strip, each pacing one cell forth and back; the two at the far end swap."""
    T = 4
    q = np.array([0, 100, 200, 254, 255])
    sched = np.zeros((T + 1, 5, 2), dtype=np.int64)
    axis = 1 if H == 1 else 0
    sched[:, :, axis] = q[None]
    sched[1::2, :3, axis] += 1
    sched[3:, 3, axis], sched[3:, 4, axis] = 255, 254
    return make_case(name, np.zeros((H, W), np.uint8), sched[T], sched,
                     facts=counts_are(0, 0, 0, 2, first=(2, C_SWAP, 3, 4), status=SWAP))


@_every('largest_map', [(2,), (1024,)], lambda n: 'N%d' % n)
def largest_map(name, n):
    """256 x 256, the 128 KB owner table: agents on cells 0 and 65 535 (and, for the full team, along the last rows); the
    agent on the last cell is joined there by agent 0 at t = 1."""
    cells = np.concatenate([[0], 65535 - np.arange(n - 1)[::-1]])
    grid, sched = pacers(n, 2, 256, 256, cells=cells)
    sched[1, 0] = (255, 255)
    return make_case(name, grid, sched[2], sched,
                     facts=counts_are(0, 2, 0, 0, first=(1, C_VERTEX, 0, n - 1), status=VERTEX))


@_case()
def zero_horizon(name):
    """T_max = 0: one row, three cases -- clean, a vertex conflict, an agent off its goal."""
    sched = np.zeros((3, 1, 2, 2), dtype=np.int64)
    sched[:, 0, 1] = (1, 1)
    sched[1, 0, 1] = (0, 0)
    goal = np.array([[(0, 0), (1, 1)]] * 3)
    goal[2, 0] = (0, 1)

    def facts(want):
        assert want['status'].tolist() == [0, VERTEX | NOT_AT_GOAL, NOT_AT_GOAL]
        assert want['arrival'].tolist() == [[0, 0], [0, -1], [-1, 0]] and want['makespan'].tolist() == [0, -1, -1]
    return make_case(name, np.zeros((2, 2), np.uint8), goal, sched, start=None, facts=facts)


# ---- lengths, starts, goals, grids ---------------------------------------------------------------------------------------
@_case()
def mixed_steps_in_one_call(name):
    """steps = -1 (skipped), 3, 100 (clamped to T_max = 6), 2 with garbage behind, 0, -5 (skipped): the neighbours of a
    skipped case are unaffected."""
    grid, one = walkers(3, 6)
    sched = np.stack([one] * 6)
    sched[0] = 10 ** 6                                   # never read
    sched[3, 3:] = -(10 ** 6)
    sched[1, 2, 1] = sched[1, 2, 0]                      # a vertex conflict inside steps = 3
    sched[1, 5, 1] = sched[1, 5, 0]                      # ... and one behind it
    goal = np.stack([one[6], one[3], one[6], one[2], one[0], one[6]])

    def facts(want):
        assert want['status'].tolist() == [SKIPPED, VERTEX, 0, 0, 0, SKIPPED]
        assert (want['arrival'][0] == -1).all() and (want['counts'][0] == -1).all() and (want['first'][5] == -1).all()
        assert want['makespan'].tolist() == [-1, 3, 6, 2, 0, -1] and want['counts'][1].tolist() == [0, 2, 0, 0]
    return make_case(name, grid, goal, sched, start=np.stack([one[0]] * 6), steps=[-1, 3, 100, 2, 0, -5], facts=facts)


@_case()
def steps_null_means_the_whole_buffer(name):
    grid, one = walkers(2, 5)
    sched = np.stack([one, one])
    sched[1, 5, 1] = (0, 0)                              # a jump on the last transition of case 1
    return make_case(name, grid, np.stack([one[5], one[5]]), sched, start=np.stack([one[0]] * 2),
                     facts=lambda want: _is(want['status'].tolist(), [0, MOVE | NOT_AT_GOAL]))


@_every('wrong_start', [(True,), (False,)], lambda given: 'given' if given else 'null')
def wrong_start(name, given):
    grid, sched = walkers(3, 4)
    start = sched[0].copy()
    start[1] = (5, 5)

    def facts(want):
        assert int(want['status'][0]) == (BAD_START if given else 0) and (want['counts'][0] == 0).all()
    return make_case(name, grid, sched[4], sched, start=start if given else None, facts=facts)


@_case()
def not_at_goal_keeps_the_other_arrivals(name):
    grid, sched = walkers(3, 5)
    goal = sched[5].copy()
    goal[1] = (2, 0)                                     # agent 1 leaves its goal at once and never returns
    sched[3:, 2] = sched[3, 2]                           # agent 2 stops early, on its goal
    goal[2] = sched[3, 2]

    def facts(want):
        assert want['arrival'][0].tolist() == [5, -1, 3] and int(want['status'][0]) == NOT_AT_GOAL
        assert int(want['makespan'][0]) == -1 and int(want['flowtime'][0]) == -1
    return make_case(name, grid, goal, sched, facts=facts)


def _grid_pair():
    grid, one = walkers(2, 4)
    grids = np.stack([grid, grid])
    grids[1, 0, 2] = 1                                   # agent 0 of case 1 walks over an obstacle at t = 2
    return grids, one


@_case()
def batched_grid(name):
    grids, one = _grid_pair()
    return make_case(name, grids, np.stack([one[4]] * 2), np.stack([one] * 2),
                     facts=lambda want: _is(want['status'].tolist(), [0, STATE]))


@_case()
def shared_grid(name):
    grids, one = _grid_pair()
    return make_case(name, grids[1], np.stack([one[4]] * 2), np.stack([one] * 2),
                     facts=lambda want: _is(want['status'].tolist(), [STATE, STATE]))


def _is(got, want):
    assert got == want, (got, want)


# ---- random degenerate schedules -----------------------------------------------------------------------------------------
@_every('random_walks_8x8', [(10, 7001), (130, 7002)], lambda N, seed: 'N%d' % N)
def random_walks_8x8(name, N, seed):
    """Seeded random walks that ignore one another, with injected jumps, off-map states and wrong starts: several classes
    meet in one case, across two seams (T_max = 70, steps mixed)."""
    rng = np.random.default_rng(seed)
    C, T, H, W = 6, 70, 8, 8
    grid = (rng.random((H, W)) < 0.1).astype(np.uint8)
    free = np.argwhere(grid == 0)
    sched = np.zeros((C, T + 1, N, 2), dtype=np.int64)
    steps_all = [(0, -1), (0, 1), (-1, 0), (1, 0), (0, 0)]
    for c in range(C):
        idle = 0.97 if N == 10 else 0.5                  # (N = 10: few moves, so clean layers and swaps do occur)
        pick = rng.permutation(len(free))[:N] if N <= len(free) else rng.integers(0, len(free), N)
        sched[c, 0] = free[pick]
        for t in range(T):
            for i in range(N):
                x, y = sched[c, t, i]
                dx, dy = steps_all[rng.integers(0, 4)] if rng.random() > idle else (0, 0)
                if not (0 <= x + dx < H and 0 <= y + dy < W) or grid[x + dx, y + dy]:
                    dx, dy = 0, 0
                sched[c, t + 1, i] = (x + dx, y + dy)
        for _ in range(rng.integers(0, 4)):              # injected: a jump that stays, a state off the map for one step
            t, i = rng.integers(1, T), rng.integers(0, N)
            if rng.random() < 0.5:
                sched[c, t:, i] = free[rng.integers(0, len(free))]
            else:
                sched[c, t, i] = (-1, rng.integers(0, W))
    goal = sched[:, T].copy()
    goal[:, 0] = free[0]
    start = sched[:, 0].copy()
    start[1, N - 1] += 1
    steps = [T, 40, -1, CHUNK, 2 * CHUNK - 1, 500]

    def facts(want):
        assert int(want['status'][2]) == SKIPPED
        seen = 0
        for c in (0, 1, 3, 4, 5):
            seen |= int(want['status'][c])
        assert seen & VERTEX and seen & STATE and int(want['status'][1]) & BAD_START
    return make_case(name, grid, goal, sched, start=start, steps=steps, facts=facts)


@_case()
def sparse_walkers_meet_every_class(name):
    """Ten slow walkers on 8 x 8, T_max = 70: hand-placed offences of all four classes in one case, each in another chunk,
    next to a clean copy of the same plan."""
    grid, base = pacers(10, 70, 8, 8, cells=np.arange(10) * 6)
    sched = np.stack([base, base.copy()])
    s = sched[1]
    s[5, 3] = s[5, 2]                                    # VERTEX at 5 (and the jumps round it are shielded)
    s[20, 4] = (8, 0)                                    # STATE at 20
    s[40:, 5] += (1, 1)                                  # MOVE on 39 -> 40
    a, b = s[0, 0].copy(), s[0, 0] + (0, 1)
    s[:, 9] = b
    s[66:, 0], s[66:, 9] = b, a                          # SWAP on 65 -> 66
    goal = np.stack([base[70], s[70]])

    def facts(want):
        assert want['status'].tolist() == [0, STATE | VERTEX | MOVE | SWAP]
        assert want['counts'][1].tolist() == [1, 2, 1, 2] and want['first'][1].tolist() == [5, C_VERTEX, 2, 3]
    return make_case(name, grid, goal, sched, facts=facts)


# names the host emulation leaves out (more than about 10 s there); at most 10 % of the table
EMU_LEFT_OUT = ()
EMU_CASES = sorted(n for n in CASES if n not in EMU_LEFT_OUT)
