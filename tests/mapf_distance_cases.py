"""Yardstick and cases of the MAPF solver's goal distances and planning orders (include/gnnpp_mapf_distance.h,
csrc/mapf_distance_kernels.hip, gnn_pathplanning_amd/mapf.py distances / heuristic_orders).

  bfs_distances   a plain breadth-first search with a queue over the cells of one map (nothing of the kernel's
                  bit-parallel layers), and want_distances: dist, lower_makespan and lower_flowtime of a call;
  rank_orders     the four ranking rules restated with np.lexsort, and order_hash: the counter hash of the 'hashed'
                  rule restated from the header's words.

CASES holds the calls themselves (name -> builder of dict(name, grid [H,W] | [C,H,W], starts / goals [C,N,2], facts)),
each built once and run under the host emulation (tests/test_emu_mapf_distance.py) and on the device
(tests/test_gpu_mapf_distance.py).  All values are integers and every comparison is exact equality.

The shapes are the smallest at which the kernel can go wrong: one thread (1 x 1, 1 x 2), rows that end one bit before,
on and one bit behind a word boundary (W = 63, 64, 65, 128, 129: an item of up to 15 threads in a wave of 64), exactly
one wave (64 x 64: four items share a workgroup and finish at different steps), 1024 threads (256 x 256), more items
than the persistent grid takes at once (kGrid workgroups of kWaveItems items).

The serpentine: a step bound borrowed from the solver's horizon 4 (H + W) would cut a long corridor short.  On 9 x 9
no distance can exceed 4 (H + W) = 72 -- a shortest path is an induced path of the grid and a corridor with its walls
leaves 49 free cells, so the 9 x 9 serpentine's distance is 48, three times the Manhattan distance -- so the bound is
crossed on the smallest square serpentine that can: rows 0, 2, .. free and joined at alternating ends have distance
(n - 1)(n + 3) / 2, which first exceeds 8 n at n = 15 (126 > 120).  Both are cases here.
"""
from collections import deque

import numpy as np

UNREACHABLE, INVALID = -1, -2
RULES = {'index': 0, 'longest_first': 1, 'shortest_first': 2, 'hashed': 3}
kGrid, kWaveItems = 1024, 4                            # csrc/mapf_distance_kernels.hip: kMapfDistGrid, kMapfDistWaveItems
POISON = -7


# ---- the yardstick -------------------------------------------------------------------------------------------------
def bfs_distances(grid, start):
    """[H,W] int64: steps of a shortest 4-connected obstacle-free path from `start` to every cell, -1 where none."""
    H, W = grid.shape
    dist = np.full((H, W), -1, dtype=np.int64)
    dist[start] = 0
    q = deque([start])
    while q:
        x, y = q.popleft()
        for dx, dy in ((-1, 0), (0, -1), (1, 0), (0, 1)):
            nx, ny = x + dx, y + dy
            if 0 <= nx < H and 0 <= ny < W and grid[nx, ny] == 0 and dist[nx, ny] < 0:
                dist[nx, ny] = dist[x, y] + 1
                q.append((nx, ny))
    return dist


def want_distances(grid, starts, goals):
    """(dist [C,N], lower_makespan [C], lower_flowtime [C]) int64 of a call; one search per distinct (map, start)."""
    grid, starts, goals = np.asarray(grid), np.asarray(starts), np.asarray(goals)
    C, N = starts.shape[:2]
    dist = np.zeros((C, N), dtype=np.int64)
    maps = {}
    for c in range(C):
        g = grid if grid.ndim == 2 else grid[c]
        H, W = g.shape
        for n in range(N):
            s, t = tuple(int(v) for v in starts[c, n]), tuple(int(v) for v in goals[c, n])
            if not all(0 <= p[0] < H and 0 <= p[1] < W and g[p] == 0 for p in (s, t)):
                dist[c, n] = INVALID
                continue
            key = (0 if grid.ndim == 2 else c, s)
            if key not in maps:
                maps[key] = bfs_distances(g, s)
            dist[c, n] = maps[key][t]
    bad = (dist < 0).any(1)
    return dist, np.where(bad, -1, dist.max(1)), np.where(bad, -1, dist.sum(1))


def _mix(x):
    """mix() of include/gnnpp_mapf_distance.h on uint64 arrays holding uint32 values."""
    m = np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & m
    return x ^ (x >> np.uint64(16))


def order_hash(seed, c, r, N):
    """[N] uint64 (values < 2^32): hash = mix(seed ^ mix(c * 0x9E3779B9 + r * 0x85EBCA6B + i)) mod 2^32."""
    m = np.uint64(0xffffffff)
    i = np.arange(N, dtype=np.uint64)
    inner = (np.uint64((c * 0x9E3779B9) & 0xffffffff) + np.uint64((r * 0x85EBCA6B) & 0xffffffff) + i) & m
    return _mix(np.uint64(seed & 0xffffffff) ^ _mix(inner))


def rank_orders(dist, rules, seed=0):
    """[C,R,N] int64: row (c, r) = the agents of case c sorted by rule rules[r] (names of RULES), ties by index."""
    dist = np.asarray(dist, dtype=np.int64)
    C, N = dist.shape
    idx = np.arange(N)
    out = np.zeros((C, len(rules), N), dtype=np.int64)
    for c in range(C):
        d = dist[c]
        for r, rule in enumerate(rules):
            if rule == 'index':
                key = idx
            elif rule == 'longest_first':               # negative keys first and alike, then descending
                key = np.where(d < 0, 0, 1 + (0x7fffffff - d))
            elif rule == 'shortest_first':              # negative keys first and alike, then ascending
                key = np.where(d < 0, 0, 1 + d)
            else:
                assert rule == 'hashed', rule
                key = order_hash(seed, c, r, N)
            out[c, r] = np.lexsort((idx, key))
    return out


def mixed_rules(restarts):
    """The rules of priorities='mixed'."""
    return ['index', 'longest_first', 'shortest_first'] + ['hashed'] * (max(int(restarts), 3) - 3)


# ---- the distance calls --------------------------------------------------------------------------------------------
CASES = {}


def make_case(name, grid, starts, goals, facts=None):
    starts, goals = np.asarray(starts), np.asarray(goals)
    if starts.ndim == 2:
        starts, goals = starts[None], goals[None]
    return {'name': name, 'grid': np.asarray(grid, np.uint8), 'starts': starts, 'goals': goals, 'facts': facts}


_WANTS = {}


def wants_of(case):
    """want_distances of the call (computed once per case name), the case's facts asserted on it."""
    if case['name'] not in _WANTS:
        want = want_distances(case['grid'], case['starts'], case['goals'])
        if case['facts'] is not None:
            case['facts'](*want)
        _WANTS[case['name']] = want
    return _WANTS[case['name']]


def assert_equal_to_yardstick(case, dist, lower_makespan, lower_flowtime):
    want = wants_of(case)
    for name, got, w in zip(('dist', 'lower_makespan', 'lower_flowtime'), (dist, lower_makespan, lower_flowtime), want):
        got = np.asarray(got)
        assert got.shape == w.shape, (name, got.shape, w.shape)
        bad = np.argwhere(got != w)
        assert len(bad) == 0, (case['name'], name, bad[:4].tolist(), got[tuple(bad[0])], w[tuple(bad[0])])


def _case(name=None):
    def register(fn):
        CASES[name or fn.__name__] = fn
        return fn
    return register


def _every(stem, params, label):
    def register(fn):
        for p in params:
            name = '%s_%s' % (stem, label % p)
            CASES[name] = (lambda name=name, p=p: fn(name, *p))
        return fn
    return register


@_case()
def one_cell_start_is_goal():
    def facts(dist, lm, lf):
        assert dist.tolist() == [[0]] and lm.tolist() == [0] and lf.tolist() == [0]
    return make_case('one_cell_start_is_goal', np.zeros((1, 1)), [[0, 0]], [[0, 0]], facts)


@_case()
def two_cells():
    def facts(dist, lm, lf):
        assert dist.tolist() == [[1, 1, 0]] and lm.tolist() == [1] and lf.tolist() == [2]
    return make_case('two_cells', np.zeros((1, 2)), [[0, 0], [0, 1], [0, 1]], [[0, 1], [0, 0], [0, 1]], facts)


WIDTHS = [(63,), (64,), (65,), (128,), (129,)]


@_every('strip', WIDTHS, 'W%d')
def strip(name, W):
    """One row: the only path runs through every word boundary of the row, by the carries of the one-bit shifts, to
    the right (agent 0) and to the left (agent 1); agent 2 starts on the last valid bit."""
    def facts(dist, lm, lf):
        assert dist.tolist() == [[W - 1, W - 1, W - 3]] and lm.tolist() == [W - 1] and lf.tolist() == [3 * W - 5]
    return make_case(name, np.zeros((1, W)), [[0, 0], [0, W - 1], [0, W - 1]], [[0, W - 1], [0, 0], [0, 2]], facts)


@_every('doors_at_the_word_boundaries', WIDTHS, 'W%d')
def doors_at_the_word_boundaries(name, W):
    """Five rows (W = 65: 10 threads, W = 129: 15); the middle one is a wall with a single gap of two cells at every
    word boundary b of the row, columns b - 1 and b (63 / 64, 127 / 128); a map without a boundary has its gap in the
    last two columns.  Agent 0 goes from the top left to the bottom right corner, agent 1 from the top right to the
    bottom left: both pass a gap and every boundary, in opposite directions.  Agents 2 and 3 start next to a gap on
    either side of the boundary and end below the other side."""
    grid = np.zeros((5, W), np.uint8)
    grid[2, :] = 1
    bounds = [b for b in (64, 128) if b < W] or [W - 1]
    for b in bounds:
        grid[2, b - 1:b + 1] = 0
    b = bounds[-1]

    def facts(dist, lm, lf):
        assert dist[0, :2].tolist() == [W - 1 + 4, W - 1 + 4]   # the gaps lie on the way: the Manhattan distance
        assert dist[0, 2:].tolist() == [3, 3] and (dist >= 0).all()
    return make_case(name, grid, [[0, 0], [0, W - 1], [1, b - 1], [1, b]], [[4, W - 1], [4, 0], [3, b], [3, b - 1]],
                     facts)


def _walled_box(grid, x0, y0):
    """A 3 x 3 ring of obstacles around the free cell (x0 + 1, y0 + 1)."""
    grid[x0:x0 + 3, y0:y0 + 3] = 1
    grid[x0 + 1, y0 + 1] = 0
    return (x0 + 1, y0 + 1)


@_case()
def one_wave_items_finish_at_different_steps():
    """64 x 64, exactly one wave per item and four items per workgroup: two cases of nine agents, 18 items in five
    workgroups; an item that ends at t = 0 and items without a path (-1) or with an invalid end (-2) share workgroups
    with searches of more than a hundred steps."""
    rng = np.random.default_rng(64)
    grids = (rng.random((2, 64, 64)) < 0.2).astype(np.uint8)
    starts, goals = np.zeros((2, 9, 2), np.int64), np.zeros((2, 9, 2), np.int64)
    for c in range(2):
        g = grids[c]
        g[32, 1:63] = 1                                 # a wall across the map, open at both ends
        g[:, 0] = g[:, 63] = g[0, :] = g[63, :] = g[31, :] = g[33, :] = 0
        box = _walled_box(g, 40, 40)
        free = np.argwhere(bfs_distances(g, (0, 0)) >= 0)      # cells that reach each other
        pick = free[rng.choice(len(free), 18, replace=False)]
        starts[c], goals[c] = pick[:9], pick[9:]
        starts[c, 0], goals[c, 0] = (0, 0), (63, 63)
        starts[c, 1], goals[c, 1] = (31, 31), (33, 31)         # round the wall: 2 + 2 * 31
        goals[c, 2] = starts[c, 2]                             # ends at t = 0
        goals[c, 3] = box                                      # walled in: -1
        starts[c, 4] = (32, 5)                                 # on the wall: -2
        goals[c, 5] = (64, 3)                                  # off the map: -2
        starts[c, 6], goals[c, 6] = box, box                   # inside the box, on its goal

    def facts(dist, lm, lf):
        assert dist[:, :2].tolist() == [[126, 64]] * 2
        assert dist[:, 2:7].tolist() == [[0, -1, -2, -2, 0]] * 2 and (dist[:, 7:] > 0).all()
        assert lm.tolist() == [-1, -1] and lf.tolist() == [-1, -1]
    return make_case('one_wave_items_finish_at_different_steps', grids, starts, goals, facts)


@_case()
def several_items_per_workgroup_end_one_bit_past_a_word():
    """7 x 65: an item is 14 threads of a wave of its own, four items per workgroup, seven items so the second batch
    is partial.  Row 3 is a wall whose only door is column 64, the one bit of word 1: every way between the halves
    passes it, in every item at its own place in the workgroup's image.  (6, 0) is walled in."""
    grid = np.zeros((7, 65), np.uint8)
    grid[3, :64] = 1
    grid[5, 0] = grid[6, 1] = 1

    def facts(dist, lm, lf):
        assert dist.tolist() == [[70, 3, -1, 0, 70, -1, 130]] and lm.tolist() == [-1] and lf.tolist() == [-1]
    return make_case('several_items_per_workgroup_end_one_bit_past_a_word', grid,
                     [[0, 0], [3, 64], [0, 5], [2, 64], [6, 64], [6, 0], [4, 0]],
                     [[6, 64], [0, 64], [6, 0], [2, 64], [0, 0], [0, 64], [2, 0]], facts)


@_case()
def largest_map_nearly_open():
    """256 x 256: 1024 threads, rows of four words; distances around 500."""
    grid = np.zeros((256, 256), np.uint8)
    grid[100, 3:250] = 1
    grid[5:200, 128] = 1

    def facts(dist, lm, lf):
        assert dist[0, 0] == 510 and dist[0, 1] == 510 and dist[0, 2] > 250
        assert lm.tolist() == [int(dist.max())] and lf.tolist() == [int(dist.sum())]
    return make_case('largest_map_nearly_open', grid, [[0, 0], [255, 0], [99, 127]], [[255, 255], [0, 255], [101, 129]],
                     facts)


@_case()
def largest_map_goal_walled_off():
    """The goal of agent 0 is walled in at the centre of an open 256 x 256 map: the search ends when the layer stops
    growing, after 510 steps, not after the H W = 65536 of the loop's bound.  Agent 1 is unaffected."""
    grid = np.zeros((256, 256), np.uint8)
    box = _walled_box(grid, 127, 127)

    def facts(dist, lm, lf):
        assert dist.tolist() == [[-1, 300]] and lm.tolist() == [-1] and lf.tolist() == [-1]
    return make_case('largest_map_goal_walled_off', grid, [[0, 0], [10, 10]], [box, [200, 120]], facts)


def _serpentine(n):
    grid = np.zeros((n, n), np.uint8)
    for k, x in enumerate(range(1, n, 2)):
        grid[x, :] = 1
        grid[x, n - 1 if k % 2 == 0 else 0] = 0
    return grid


@_every('serpentine', [(9,), (15,)], '%d')
def serpentine(name, n):
    """See the module's docstring: 48 steps on 9 x 9, and 126 > 4 (H + W) = 120 on 15 x 15."""
    want = (n - 1) * (n + 3) // 2
    end = [n - 1, n - 1 if ((n + 1) // 2) % 2 else 0]           # the far end of the last free row

    def facts(dist, lm, lf):
        assert dist.tolist() == [[want, want]] and (n < 15 or want > 4 * (n + n))
    return make_case(name, _serpentine(n), [[0, 0], end], [end, [0, 0]], facts)


@_case()
def small_map_goal_walled_off():
    grid = np.zeros((6, 6), np.uint8)
    grid[3:6, 3] = 1
    grid[3, 3:6] = 1                                            # (4,4), (4,5), (5,4), (5,5) walled in

    def facts(dist, lm, lf):
        assert dist.tolist() == [[-1, 2, -1, 4]]
    return make_case('small_map_goal_walled_off', grid, [[0, 0], [4, 4], [5, 5], [0, 0]],
                     [[5, 5], [5, 5], [0, 0], [2, 2]], facts)


@_case()
def invalid_ends_flag_only_themselves():
    """A start on an obstacle, a goal off the map (each side), in the middle case of three: the other cases and the
    other agents of the case keep their distances."""
    grid = np.zeros((3, 5, 7), np.uint8)
    grid[:, 2, 3] = 1
    ok_s, ok_g = np.array([[0, 0], [4, 6], [0, 6], [2, 2]]), np.array([[4, 6], [0, 0], [4, 0], [2, 4]])
    starts, goals = np.stack([ok_s] * 3), np.stack([ok_g] * 3)
    starts[1, 0] = (2, 3)
    goals[1, 1] = (5, 0)
    goals[1, 2] = (0, -1)

    def facts(dist, lm, lf):
        assert dist.tolist() == [[10, 10, 10, 4], [-2, -2, -2, 4], [10, 10, 10, 4]]
        assert lm.tolist() == [10, -1, 10] and lf.tolist() == [34, -1, 34]
    return make_case('invalid_ends_flag_only_themselves', grid, starts, goals, facts)


@_case()
def shared_grid_next_to_batched_grid():
    """Three cases on one map (the test passes it once and per case: the same bytes)."""
    import mapf_cases as mc
    rng = np.random.default_rng(34)
    grid, _, _ = mc.random_cases(rng, 1, 5, 9, 70, density=0.15)[0]
    cases = mc._same_grid_cases(rng, grid, 3, 5)
    return make_case('shared_grid_next_to_batched_grid', np.stack([c[0] for c in cases]),
                     np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases]))


@_case()
def more_items_than_the_persistent_grid():
    """1500 cases of 3 agents on one 8 x 8 map: 4500 items, more than the kGrid * kWaveItems = 4096 a launch takes at
    once, so workgroups come back for a second batch (and the last batch is not full: 4500 = 1125 * 4)."""
    rng = np.random.default_rng(8)
    grid = (rng.random((8, 8)) < 0.2).astype(np.uint8)
    cells = np.argwhere(np.ones((8, 8), bool))                  # obstacles included: some items are -2
    starts = cells[rng.integers(0, 64, (1500, 3))]
    goals = cells[rng.integers(0, 64, (1500, 3))]

    def facts(dist, lm, lf):
        assert dist.size > kGrid * kWaveItems
        assert {-2, 0} <= set(np.unique(dist).tolist())
        assert (dist > 5).any() and (lm >= 0).any() and (lm < 0).any()
    return make_case('more_items_than_the_persistent_grid', grid, starts, goals, facts)


# ---- the order calls -----------------------------------------------------------------------------------------------
ORDER_SIZES = [1, 2, 63, 65, 1023, 1024]
ALL_RULES = ['index', 'longest_first', 'shortest_first', 'hashed']


def synthetic_keys(N):
    """dist [3,N]: heavy ties (three distinct values at N = 1024), a mix of -1 and -2 with distances, and keys without
    ties that include the largest int32."""
    rng = np.random.default_rng(N)
    few = rng.choice(np.array([4, 9, 17]), N)
    mixed = rng.integers(-2, 6, N)
    spread = rng.permutation(N) * 2097151 + (0x7fffffff - 2097151 * (N - 1)) if N > 1 else np.array([0x7fffffff])
    return np.stack([few, mixed, spread]).astype(np.int64)


def assert_permutations(order, N):
    order = np.asarray(order)
    assert (np.sort(order, axis=-1) == np.arange(N)).all()


# ---- end to end ----------------------------------------------------------------------------------------------------
def corridor_2x4():
    """(grid, starts, goals, T): row 0 free, of row 1 only (1,1).  In the index order agent 0 parks on (0,2), in the
    corridor agent 1 must pass: NO_PATH, failing agent 1, arrivals [1,-1].  Longest first (distances 1 and 3) plans
    agent 1 first: solved, arrivals [3,3]."""
    grid = np.array([[0, 0, 0, 0],
                     [1, 0, 1, 1]], np.uint8)
    return grid, np.array([[0, 1], [0, 0]]), np.array([[0, 2], [0, 3]]), 16


def explicit_order_sets():
    """The seeded sets of the equality tests: (cases for solve: 6 of 10 agents on 20 x 20; cases for solve_team: 3 of
    130 agents on 40 x 70)."""
    import mapf_cases as mc
    return (mc.random_cases(np.random.default_rng(2010), 6, 10, 20, density=0.1),
            mc.random_cases(np.random.default_rng(4070), 3, 130, 40, 70, density=0.1))


MIXED_SET = dict(seed=1212, count=32, N=10, side=12, density=0.2)


def mixed_set():
    """32 cases of 10 agents on 12 x 12, density 0.2: under the index order some are solved and some are not."""
    import mapf_cases as mc
    return mc.random_cases(np.random.default_rng(MIXED_SET['seed']), MIXED_SET['count'], MIXED_SET['N'],
                           MIXED_SET['side'], density=MIXED_SET['density'])
