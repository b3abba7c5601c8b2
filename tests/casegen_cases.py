"""The yardstick and the named cases of gnnpp_casegen (include/gnnpp_casegen.h), shared by tests/test_emu_casegen.py (the
host emulation), tests/test_gpu_casegen.py (the device) and tests/test_casegen_yardstick.py (the yardstick alone).

The yardstick restates rules 1-5 of the header in plain numpy: the hashes on uint64 arrays, component labelling by a
queue-based breadth-first search over the cells in q order, np.lexsort for the ranks, the fix-up as the loop the header
writes out.  It shares no code with the kernel (no word layout, no floods, no radix select).  Every value is an integer and
every comparison with it is exact equality.

A named case is one call: dict(C, N, H, W, threshold, seed, grids) with grids None | [H,W] | [C,H,W], and `facts`, a
check made on the YARDSTICK's answer that the case shows what its name says -- so no test passes on an empty premise.
"""
from collections import deque

import numpy as np

OK, TOO_SMALL = 0, 1
POISON = -7
kGrid = 1024                                           # csrc/casegen_kernels.hip: kCasegenGrid


def threshold_of(density):
    return min(int(density * 2 ** 32), 2 ** 32 - 1)


# ---- the yardstick -------------------------------------------------------------------------------------------------
def _mix(x):
    """mix() of include/gnnpp_casegen.h on uint64 arrays holding uint32 values."""
    m = np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & m
    return x ^ (x >> np.uint64(16))


def keys(seed, s, c, cells):
    """[cells] uint64 (values < 2^32): key(s, c, q) = mix(seed ^ mix(c * 0x9E3779B9 + s * 0x85EBCA6B + q)) mod 2^32.
    mix is a bijection of the uint32 values, so the keys of one stream of one case are pairwise distinct."""
    m = np.uint64(0xffffffff)
    q = np.arange(cells, dtype=np.uint64)
    inner = (np.uint64((c * 0x9E3779B9) & 0xffffffff) + np.uint64((s * 0x85EBCA6B) & 0xffffffff) + q) & m
    return _mix(np.uint64(seed & 0xffffffff) ^ _mix(inner))


def components(raw):
    """Label the 4-connected components of the free cells of raw [H,W] (nonzero = obstacle) in the order of their lowest
    q: (label [H,W] int64, -1 on obstacles; sizes)."""
    H, W = raw.shape
    label = np.full((H, W), -1, dtype=np.int64)
    sizes = []
    for x0 in range(H):
        for y0 in range(W):
            if raw[x0, y0] != 0 or label[x0, y0] >= 0:
                continue
            k = len(sizes)
            label[x0, y0] = k
            n, queue = 1, deque([(x0, y0)])
            while queue:
                x, y = queue.popleft()
                for dx, dy in ((-1, 0), (0, -1), (1, 0), (0, 1)):
                    nx, ny = x + dx, y + dy
                    if 0 <= nx < H and 0 <= ny < W and raw[nx, ny] == 0 and label[nx, ny] < 0:
                        label[nx, ny] = k
                        n += 1
                        queue.append((nx, ny))
            sizes.append(n)
    return label, sizes


def generate(C, N, H, W, threshold=0, seed=0, grids=None):
    """What one gnnpp_casegen call writes: dict(grid [C,H,W], start, goal [C,N,2], cells, status [C]) int64, and what
    the facts look at: raw [C,H,W], components [C] (their number), exchanges [C] (fix-ups of rule 5, for N == 1 whether
    the rank-1 goal was taken), wrapped [C] (agent N-1 exchanged with agent 0)."""
    out = {'grid': np.ones((C, H, W), np.int64), 'start': np.full((C, N, 2), -1, np.int64),
           'goal': np.full((C, N, 2), -1, np.int64), 'cells': np.zeros(C, np.int64), 'status': np.zeros(C, np.int64),
           'raw': np.zeros((C, H, W), np.int64), 'components': np.zeros(C, np.int64),
           'exchanges': np.zeros(C, np.int64), 'wrapped': np.zeros(C, bool)}
    for c in range(C):
        if grids is None:                                                       # rule 1
            raw = (keys(seed, 0, c, H * W) < np.uint64(threshold)).reshape(H, W).astype(np.int64)
        else:
            g = np.asarray(grids)
            raw = (g if g.ndim == 2 else g[c]) != 0
            raw = raw.astype(np.int64)
        out['raw'][c] = raw
        label, sizes = components(raw)                                          # rule 2
        out['components'][c] = len(sizes)
        if not sizes:
            out['status'][c] = TOO_SMALL
            continue
        keep = int(np.argmax(sizes))                    # (the first of the largest: the one with the lowest q)
        kept = (label == keep).reshape(-1)
        out['grid'][c] = (~kept).reshape(H, W)
        cells = out['cells'][c] = sizes[keep]
        if cells < N or cells < 2:                                              # rule 3
            out['status'][c] = TOO_SMALL
            continue
        q = np.flatnonzero(kept)
        s = q[np.lexsort((q, keys(seed, 1, c, H * W)[q]))]                     # rule 4
        g = q[np.lexsort((q, keys(seed, 2, c, H * W)[q]))]                     # rule 5
        start = s[:N]
        if N == 1:
            goal = g[:1] if g[0] != start[0] else g[1:2]
            out['exchanges'][c] = int(g[0] == start[0])
        else:
            goal = g[:N].copy()
            for i in range(N):
                if goal[i] == start[i]:
                    e = (i + 1) % N
                    goal[i], goal[e] = goal[e], goal[i]
                    out['exchanges'][c] += 1
                    out['wrapped'][c] |= e == 0
        out['start'][c] = np.stack([start // W, start % W], 1)
        out['goal'][c] = np.stack([goal // W, goal % W], 1)
    return out


OUTPUTS = ('grid', 'start', 'goal', 'cells', 'status')


def assert_properties(out):
    """What rules 2-5 guarantee, on the outputs of a call alone (the yardstick's, the emulation's, the device's; raw:
    the raw map when the caller knows it): per OK case the starts pairwise distinct, the goals pairwise distinct, no
    agent on its own goal, every start and goal a free cell of `grid`, the free cells of `grid` ONE 4-connected
    component of `cells` cells; per too-small case every start and goal entry -1."""
    grid, start, goal = (np.asarray(out[k]).astype(np.int64) for k in ('grid', 'start', 'goal'))
    C, N = start.shape[:2]
    H, W = grid.shape[1:]
    for c in range(C):
        label, sizes = components(grid[c])
        assert len(sizes) <= 1 and int(out['cells'][c]) == sum(sizes), (c, sizes)
        if 'raw' in out:                                # grid = raw plus filled cells
            raw = np.asarray(out['raw'][c]) != 0
            assert (grid[c][raw] == 1).all(), c
            raw_label, raw_sizes = components(raw.astype(np.int64))
            assert sum(sizes) == max(raw_sizes, default=0), c
        if int(out['status'][c]) != OK:
            assert int(out['status'][c]) == TOO_SMALL and (sum(sizes) < N or sum(sizes) < 2), c
            assert (start[c] == -1).all() and (goal[c] == -1).all(), c
            continue
        assert sum(sizes) >= max(N, 2), c
        sq, gq = start[c, :, 0] * W + start[c, :, 1], goal[c, :, 0] * W + goal[c, :, 1]
        for pts in (start[c], goal[c]):
            assert (pts >= 0).all() and (pts[:, 0] < H).all() and (pts[:, 1] < W).all(), c
            assert (grid[c][pts[:, 0], pts[:, 1]] == 0).all(), c
        assert len(set(sq.tolist())) == N and len(set(gq.tolist())) == N and (sq != gq).all(), c


# ---- the named cases -----------------------------------------------------------------------------------------------
CASES = {}


def make_case(C, N, H, W, threshold=0, seed=0, grids=None, facts=None):
    grids = None if grids is None else np.ascontiguousarray(grids, dtype=np.uint8)
    return dict(C=C, N=N, H=H, W=W, threshold=threshold, seed=seed, grids=grids, facts=facts)


_WANTS = {}


def wants_of(name):
    """The yardstick's answer of a named case, computed once per process and never changed; its facts asserted."""
    if name not in _WANTS:
        case = CASES[name]()
        want = generate(case['C'], case['N'], case['H'], case['W'], case['threshold'], case['seed'], case['grids'])
        if case['facts'] is not None:
            case['facts'](want)
        for v in want.values():
            v.setflags(write=False)
        _WANTS[name] = want
    return _WANTS[name]


def assert_equal_to_yardstick(name, got):
    """got: the call's five outputs as arrays."""
    want = wants_of(name)
    for k in OUTPUTS:
        g = np.asarray(got[k]).astype(np.int64)
        assert g.shape == want[k].shape, (k, g.shape, want[k].shape)
        bad = np.argwhere(g != want[k])
        assert len(bad) == 0, '%s: %s differs at %s: got %s, want %s' % (
            name, k, bad[0].tolist(), g[tuple(bad[0])], want[k][tuple(bad[0])])


def _case(name=None):
    def deco(fn):
        CASES[name or fn.__name__] = fn
        return fn
    return deco


def _every(stem, params, label):
    def deco(fn):
        for prm in params:
            CASES[stem + '_' + label % prm] = (lambda prm=prm: fn(*prm))
        return fn
    return deco


@_case()
def one_by_two_single_agent_takes_the_rank_one_goal():
    """1 x 2, N = 1: in half of the cases the goal of rank 0 is the start, and the cell of rank 1 is taken."""
    def facts(w):
        assert (w['status'] == OK).all() and (w['cells'] == 2).all()
        assert (w['exchanges'] == 1).any() and (w['exchanges'] == 0).any()
    return make_case(16, 1, 1, 2, seed=4, facts=facts)


@_case()
def one_by_one_is_too_small():
    def facts(w):
        assert w['status'].tolist() == [TOO_SMALL] * 3 and w['cells'].tolist() == [1] * 3
    return make_case(3, 1, 1, 1, seed=1, facts=facts)


# seeds found by a search over the yardstick: a case of the call exchanges twice, the second time agent N-1 with agent 0
SEED_2X2, SEED_3X3 = 1, 2


@_case()
def two_by_two_three_agents_exchange_twice_with_the_wrap():
    def facts(w):
        assert (w['status'] == OK).all() and (w['cells'] == 4).all()
        assert ((w['exchanges'] == 2) & w['wrapped']).any() and (w['exchanges'] == 0).any()
    return make_case(64, 3, 2, 2, seed=SEED_2X2, facts=facts)


@_case()
def three_by_three_four_agents_exchange_twice_with_the_wrap():
    def facts(w):
        assert (w['status'] == OK).all() and (w['cells'] == 9).all()
        assert ((w['exchanges'] == 2) & w['wrapped']).any() and (w['exchanges'] == 0).any()
    return make_case(64, 4, 3, 3, seed=SEED_3X3, facts=facts)


def _two_rooms():
    """4 x 5, a wall down column 2 with no door: the left room has 8 cells, the right one 7 after one more obstacle."""
    g = np.zeros((4, 5), np.uint8)
    g[:, 2] = 1
    g[3, 4] = 1
    return g


@_case()
def team_fills_the_region_next_to_one_agent_too_many():
    """N = 8: case 0 keeps the 8-cell room and every cell of it is a start and a goal (N == cells); in case 1 that room
    has lost a cell, both rooms hold 7, the left one wins the tie, and N == cells + 1 is too small; case 2 is case 0."""
    a, b = _two_rooms(), _two_rooms()
    b[0, 0] = 1

    def facts(w):
        assert w['cells'].tolist() == [8, 7, 8] and w['status'].tolist() == [OK, TOO_SMALL, OK]
        assert sorted((w['start'][0] @ [5, 1]).tolist()) == sorted((w['goal'][0] @ [5, 1]).tolist()) == [0, 1, 5, 6, 10, 11, 15, 16]
        assert w['grid'][1, :, :2].sum() == 1 and (w['grid'][1, :, 2:] == 1).all()
        assert not np.array_equal(w['start'][0], w['start'][2])        # the case index is part of every hash
    return make_case(3, 8, 4, 5, seed=2, grids=np.stack([a, b, a]), facts=facts)


@_case()
def equal_components_keep_the_lowest_cell():
    """3 x 8: rooms of 6, 6 and 2 cells (columns 1-2, columns 4-5, the lower two cells of column 7): the first is kept."""
    g = np.ones((3, 8), np.uint8)
    g[:, 1:3] = 0
    g[:, 4:6] = 0
    g[1:, 7] = 0

    def facts(w):
        assert w['components'].tolist() == [3, 3] and w['cells'].tolist() == [6, 6]
        assert (w['grid'][:, :, 1:3] == 0).all() and w['grid'].sum() == 2 * (24 - 6)
    return make_case(2, 3, 3, 8, seed=5, grids=g, facts=facts)


@_case()
def larger_component_without_the_first_free_cell():
    """65 x 9 (two waves of rows): a 21-cell corridor down column 0 holds the first free cell, the 65-cell corridor down
    column 4 is kept -- its flood crosses from row 63 to row 64."""
    g = np.ones((65, 9), np.uint8)
    g[:21, 0] = 0
    g[:, 4] = 0

    def facts(w):
        assert w['cells'].tolist() == [65] * 2 and (w['grid'][:, :, 4] == 0).all() and w['grid'].sum() == 2 * (65 * 9 - 65)
        assert (w['start'][:, :, 1] == 4).all() and (w['goal'][:, :, 1] == 4).all()
    return make_case(2, 40, 65, 9, seed=6, grids=g, facts=facts)


@_case()
def map_without_a_free_cell():
    def facts(w):
        assert w['cells'].tolist() == [0, 0] and w['status'].tolist() == [TOO_SMALL] * 2 and (w['grid'] == 1).all()
    return make_case(2, 2, 3, 5, seed=7, grids=np.ones((3, 5), np.uint8), facts=facts)


@_case()
def checkerboard_is_the_worst_case_of_the_closure():
    """8 x 8, every free cell a component of its own: 32 floods of one cell, the loop's bound; cell 1 is kept."""
    g = (np.add.outer(np.arange(8), np.arange(8)) % 2 == 0).astype(np.uint8)

    def facts(w):
        assert w['components'].tolist() == [32] and w['cells'].tolist() == [1] and w['status'].tolist() == [TOO_SMALL]
        assert w['grid'][0, 0, 1] == 0 and w['grid'].sum() == 63
    return make_case(1, 1, 8, 8, seed=8, grids=g, facts=facts)


def _serpentine_rows(W):
    """5 x W: rows 1 and 3 are walls with one door each, at the last and at the first column -- the flood runs right
    along row 0, left along row 2, right along row 4, across every word boundary in both directions."""
    g = np.zeros((5, W), np.uint8)
    g[1, :-1] = 1
    g[3, 1:] = 1
    return g


WIDTHS = [(63,), (64,), (65,), (129,)]


@_every('serpentine_shared', WIDTHS, 'W%d')
def serpentine_shared(W):
    """One caller map shared by four cases: the same grid, different agents."""
    def facts(w):
        assert w['cells'].tolist() == [3 * W + 2] * 4 and (w['grid'] == _serpentine_rows(W)).all()
        assert len({w['start'][c].tobytes() for c in range(4)}) == 4
    return make_case(4, 50, 5, W, seed=9, grids=_serpentine_rows(W), facts=facts)


@_every('hashed_rows', WIDTHS, 'W%d')
def hashed_rows(W):
    """Hashed maps at density 0.25 on 5 x W: components on both sides of the word boundaries, no bit at columns >= W."""
    def facts(w):
        assert (w['status'] == OK).all() and (w['components'] > 1).any()
        assert w['raw'].mean() > 0.15 and (w['grid'].sum((1, 2)) + w['cells'] == 5 * W).all()
    return make_case(3, 24, 5, W, threshold=threshold_of(0.25), seed=10, facts=facts)


@_case()
def hashed_tall_map_of_two_waves():
    def facts(w):
        assert (w['status'] == OK).all() and (w['grid'][:, 64] == 0).any() and (w['components'] > 1).any()
    return make_case(2, 30, 65, 9, threshold=threshold_of(0.2), seed=11, facts=facts)


@_case()
def many_components_at_density_045():
    def facts(w):
        assert w['components'].max() >= 20 and (w['status'] == OK).all()
    return make_case(8, 4, 16, 16, threshold=int(0.45 * 2 ** 32), seed=12, facts=facts)


@_case()
def caller_maps_batched():
    """The raw maps of many_components_at_density_045, handed in as the caller's own: the same closure, the same agents."""
    raw = generate(8, 4, 16, 16, int(0.45 * 2 ** 32), 12)['raw']

    def facts(w):
        other = wants_of('many_components_at_density_045')
        assert all(np.array_equal(w[k], other[k]) for k in OUTPUTS)
    return make_case(8, 4, 16, 16, threshold=123, seed=12, grids=raw, facts=facts)


@_case()
def random_20x20():
    def facts(w):
        assert (w['status'] == OK).all() and (w['components'] > 1).any() and w['cells'].min() > 300
    return make_case(64, 10, 20, 20, threshold=threshold_of(0.1), seed=13, facts=facts)


@_case()
def random_40x40():
    def facts(w):
        assert (w['status'] == OK).all() and (w['components'] > 1).any()
    return make_case(8, 64, 40, 40, threshold=threshold_of(0.1), seed=14, facts=facts)


@_case()
def empty_map_threshold_zero():
    def facts(w):
        assert (w['raw'] == 0).all() and w['cells'].tolist() == [42] * 2 and (w['exchanges'] >= 0).all()
    return make_case(2, 42, 6, 7, threshold=0, seed=15, facts=facts)


@_case()
def more_cases_than_the_persistent_grid():
    """kGrid + 3 cases of 6 x 6: three workgroups generate a second case."""
    def facts(w):
        assert (w['status'] == OK).all() and len({w['start'][c].tobytes() for c in (0, 1, kGrid, kGrid + 1)}) == 4
    return make_case(kGrid + 3, 5, 6, 6, threshold=threshold_of(0.1), seed=17, facts=facts)


EMU_CASES = sorted(CASES)                              # every case above runs under the host emulation and on the device


@_case()
def largest_map_largest_team():
    """256 x 256 with 1024 agents: 1024 threads, rows of four words, every limit of the call at once (device only)."""
    def facts(w):
        assert (w['status'] == OK).all() and (w['components'] > 1).all() and w['cells'].min() > 55000
    return make_case(2, 1024, 256, 256, threshold=threshold_of(0.1), seed=16, facts=facts)
