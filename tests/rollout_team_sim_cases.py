"""TEST INFRASTRUCTURE ONLY: the large-team simulator (csrc/rollout_team_kernels.hip, csrc/rollout_team_lists_kernel.hip:
teams of 129 to 1024 agents) at its map and team-size edges, and the thin maps (1 x 65 536, 65 536 x 1) on which a squared
distance passes 2^31, at every team size.  The cases are built once here, with the facts the sequential oracle's answer must
show, and run through the runner of tests/rollout_sim_cases.py (imported, not copied: SimState, run_case, run_unsupported,
the check functions), which for N > 128 reaches the team kernels through the same gnnpp_rollout_* calls: separate launches
against oracle.rollout_oracle, the twin through gnnpp_rollout_gso_observe / gnnpp_rollout_step, poisoned outputs, sentinel
margins, every call twice, inputs unchanged, all of it as equality of bytes.  The neighbour-list call runs through
run_lists_case of tests/rollout_lists_cases.py.  Backends: the host emulation (tests/test_emu_rollout_team_sim.py) and the
device (tests/test_gpu_rollout_team_sim_cases.py).  A plain helper module, not a conftest.

Tie rule 'lowest' and the limits [50, 3, 2][:B] everywhere, with one exception: a case of one episode that takes two steps
or fewer (N >= 1023, and the device-only LDS table at N = 1024) gets the limit of its last step, so that the statistics
of the episode's end are computed by a full workgroup too."""
import functools

import numpy as np

import rollout_lists_cases as lc
import rollout_sim_cases as sc
from rollout_sim_cases import _case, _check_graph, _check_non_square, _check_tie_breaks, _graph_case


def _random(seed, *args, **kw):
    """sc._random, drawn again (seed + 10 000) while an agent starts on its own goal: such an agent reaches it without ever
    having started, and the reference cannot compute the statistics of an episode that ends with one."""
    while True:
        inst = sc._random(seed, *args, **kw)
        if not (inst[1] == inst[2]).all(-1).any():
            return inst
        seed += 10000


# ---- non-square maps ----------------------------------------------------------------------------------------------------
NON_SQUARE_SHAPES = ((7, 300, 129), (300, 7, 192), (12, 90, 257), (90, 12, 130))


@functools.lru_cache(None)
def non_square_cases():
    cases = []
    for k, (H, W, N) in enumerate(NON_SQUARE_SHAPES):
        for shared in (False, True):
            inst = _random(1100 + k, 2, N, H, W, 0.12, shared=shared)
            cases.append(_case('team_sim/non_square/%dx%d/N%d/%s' % (H, W, N, 'shared' if shared else 'batched'), *inst,
                               check=_check_non_square))
    return cases


# ---- maps inside or barely outside the 11 x 11 frame ---------------------------------------------------------------------
FOV_SHAPES = ((12, 11, 129), (11, 12, 130), (9, 15, 131))


@functools.lru_cache(None)
def fov_cases():
    """132, 132 and 135 cells for 129, 130 and 131 agents, no obstacles: nearly every move conflicts."""
    return [_case('team_sim/fov/%dx%d/N%d' % (H, W, N), *_random(1200 + k, 2, N, H, W, 0.0), check=_check_tie_breaks)
            for k, (H, W, N) in enumerate(FOV_SHAPES)]


# ---- team sizes at the kernels' seams ------------------------------------------------------------------------------------
# team_threads rounds the workgroup up to 64 threads (191 / 192 / 193, 255 / 256 / 257, 511 / 513, 1023 / 1024), an agent
# set has kTeamWords = 16 words of 64 bits (team_next_todo, team_any: the same sizes), observe takes 16 agents per
# workgroup (129 = 8 x 16 + 1, 193, 257, 513).
TEAM_SIZES = (129, 191, 192, 193, 255, 256, 257, 511, 513, 1023, 1024)


def _team_map(N):
    return 24 if N <= 257 else 40 if N <= 513 else 48


@functools.lru_cache(None)
def team_size_cases():
    """4 % obstacles, the starts packed into a corner box at about two cells per agent; every episode breaks a tie.  Two
    episodes and four steps; one episode and two steps from N = 1023 on (the sequential oracle is the slow part)."""
    cases = []
    for N in TEAM_SIZES:
        W, side = _team_map(N), int(np.ceil(np.sqrt(2 * N)))
        assert side <= W
        big = N >= 1023
        cases.append(_case('team_sim/team/N%d/on_%d' % (N, W),
                           *_random(1300 + N, 1 if big else 2, N, W, W, 0.04, T=2 if big else 4, box=(side, side)),
                           maxstep=[2] if big else [50, 3], check=_check_tie_breaks))
    return cases


# The oracle alone, on the CPU, counts on these instances
#   129 agents on 12 x 12, two episodes, four steps:   764 tie-breaks (393 and 371 per episode);
#   1024 agents on 34 x 34, one episode, two steps:    1627 tie-breaks.
# The floors lie a little below.
TEAM_DENSE_COUNTS = {129: 764, 1024: 1627}
TEAM_DENSE_FLOORS = {129: 700, 1024: 1500}


@functools.lru_cache(None)
def team_dense_cases():
    def check(case, tr):
        N = case['starts'].shape[1]
        assert tr['choice_count'].sum() > TEAM_DENSE_FLOORS[N], (N, int(tr['choice_count'].sum()))
    return [_case('team_sim/team/N129/dense_on_12', *_random(1401, 2, 129, 12, 12, 0.0), maxstep=[50, 50], check=check),
            _case('team_sim/team/N1024/dense_on_34', *_random(1402, 1, 1024, 34, 34, 0.0, T=2), maxstep=[2], check=check)]


# ---- the three map-load paths of observe_stage at N = 129 ----------------------------------------------------------------
MAP_LOAD_SHAPES = ((16, 20), (18, 14), (15, 17))       # 320 cells: 16 per load; 252: 4 per load; 255: byte by byte
MAP_LOAD_SKEWS = (1, 4, 16)


@functools.lru_cache(None)
def map_load_cases():
    cases = [_case('team_sim/map_load/%dx%d/batched' % (H, W), *_random(1500 + k, 3, 129, H, W, 0.1))
             for k, (H, W) in enumerate(MAP_LOAD_SHAPES)]
    cases += [_case('team_sim/map_load/16x20/shared/base+%d' % skew,
                    *_random(1510 + skew, 3, 129, 16, 20, 0.1, shared=True), grid_skew=skew) for skew in MAP_LOAD_SKEWS]
    assert [sc.load_paths(c, 64 + c['grid_skew']) for c in cases] == \
        [[16] * 3, [4] * 3, [1] * 3, [1] * 3, [4] * 3, [16] * 3]
    return cases


# ---- hand-built graph states (all stop, grow = 0) -------------------------------------------------------------------------
BROKEN_LINK = 700                                      # the widened link of the 1024-agent chain: agents 700 | 701


def _broken_chain():
    pos = lc._chain(1024, 3)
    pos[0, BROKEN_LINK + 1:, 1] += 1
    return pos


def _outlier_high():
    """1000 agents in a 40 x 40 box, agent 990 (word 15 of the agent set) far away."""
    pos = lc._scatter(31, 1, 1000, 40)
    pos[0, 990] = (120, 120)
    return pos


def _split_word():
    """Agents 0 .. 99 in one 10 x 10 box, 100 .. 159 in another 40 cells away: the components part inside word 1."""
    a = np.stack(np.unravel_index(np.random.default_rng(32).permutation(100), (10, 10)), 1)
    b = np.stack(np.unravel_index(np.random.default_rng(33).permutation(64)[:60], (8, 8)), 1) + 50
    return np.concatenate([a, b])[None]


def _packed_box_1024():
    return np.stack(np.unravel_index(np.random.default_rng(34).permutation(1024), (32, 32)), 1)[None]


def _radius5_padded():
    """The strict-`<` pairs of _radius5_state and 119 agents more than 5 away from them and from each other."""
    pad = [(40 + 6 * (k // 12), 6 * (k % 12)) for k in range(119)]
    return np.concatenate([sc._radius5_state(), np.array(pad)[None]], 1)


def _check_split(case, tr):
    S = tr['S'][0, 0]
    assert (tr['connected'] == 0).all() and not S[:100, 100:].any() and not S[100:, :100].any(), case['name']
    assert (S[:100, :100] != 0).any(1).all() and (S[100:, 100:] != 0).any(1).all(), case['name']


def _check_broken(case, tr):
    """The search from agent 0 reaches agents 0 .. BROKEN_LINK and nobody behind them (words 10 .. 15 stay unreached)."""
    S = tr['S'][0, 0]
    assert (tr['connected'] == 0).all() and BROKEN_LINK >= 64, case['name']
    assert not S[BROKEN_LINK, BROKEN_LINK + 1] and S[BROKEN_LINK - 1, BROKEN_LINK] and S[BROKEN_LINK + 1, BROKEN_LINK + 2]


@functools.lru_cache(None)
def graph_cases():
    return [
        _graph_case('team/chain129', lc._chain(129, 3), 3.5, 1, 3070, _check_graph(connected=1, degree=None)),
        _graph_case('team/chain1024', lc._chain(1024, 3), 3.5, 1, 3070, _check_graph(connected=1)),
        _graph_case('team/chain1024/broken_at_700', _broken_chain(), 3.5, 1, 3071, _check_broken),
        _graph_case('team/outlier990', _outlier_high(), 4.0, 128, 128, _check_graph(connected=0, isolated=990)),
        _graph_case('team/split_inside_word1', _split_word(), 3.0, 64, 64, _check_split),
        _graph_case('team/packed_box1024/degree1023', _packed_box_1024(), 50.0, 32, 32,
                    _check_graph(connected=1, degree=1023)),
        _graph_case('team/radius5/strict_less', _radius5_padded(), 5.0, 100, 100, _check_graph(connected=0, exact5=True)),
    ]


# ---- thin maps: a coordinate difference of up to 65 535 -------------------------------------------------------------------
# d2 = dx^2 + dy^2 reaches 65535^2 = 4 294 836 225: above 2^31, below 2^32.  A product kept in a signed word wraps to a
# negative number, which passes every `d2 <= T` test: an edge between agents a whole map apart.
THIN_SIDE = 65536
THIN_SHAPES = ((1, THIN_SIDE), (THIN_SIDE, 1))
THIN_SIZES = (2, 128, 129, 1024)                        # 2 and 128 take the one-wave kernels: the same statement


def _spread(N):
    """N cells spread evenly over 0 .. 65535, both ends occupied."""
    return np.round(np.linspace(0, THIN_SIDE - 1, N)).astype(np.int64)


def _thin_case(name, H, W, cells, radius, grow, check, seed):
    """One episode on an empty H x W map (one of them 1), the agents on `cells` along its long side, one step of random
    joint actions: every move across the map bumps its edge."""
    N = len(cells)
    assert len(set(cells.tolist())) == N and cells.min() >= 0 and cells.max() < THIN_SIDE
    pos = np.zeros((1, N, 2), np.int64)
    pos[0, :, 1 if H == 1 else 0] = cells
    actions = np.random.default_rng(seed).integers(0, 5, size=(1, 1, N))
    return _case('team_sim/thin/%dx%d/N%d/%s' % (H, W, N, name), np.zeros((H, W), np.uint8), pos, pos[:, ::-1], actions,
                 radius=radius, grow=grow, check=check)


def _d2(case):
    p = case['starts'][0].astype(np.int64)
    return ((p[:, None] - p[None]) ** 2).sum(-1)


def _check_wrapping_inputs(case):
    """Some pair has d2 above 2^31, and some pair has 2^31 - 2^17 < d2 mod 2^32: what a wrapped product gets wrong."""
    d2 = _d2(case)
    assert (d2 > 2 ** 31).any() and (d2 % 2 ** 32 > 2 ** 31 - 2 ** 17).any() and d2.max() < 2 ** 32, case['name']


def _check_spread(case, tr):
    _check_wrapping_inputs(case)
    assert not tr['S'][0].any() and tr['connected'][0, 0] == 0, case['name']
    across = (0, 2) if case['grids'].shape[0] == 1 else (1, 3)                 # the moves off the map's long side
    if np.isin(case['actions'][0, 0], across).any():
        assert tr['flags'][0, 0, 2] == 1, case['name']                         # ... bump its edge


def _check_pair(case, tr):
    N = case['starts'].shape[1]
    if N > 2:
        _check_wrapping_inputs(case)
    i, j = np.nonzero(tr['S'][0, 0])
    assert sorted(zip(i.tolist(), j.tolist())) == [(0, 1), (1, 0)], case['name']
    assert tr['connected'][0, 0] == int(N == 2), case['name']


def _check_ends(case, tr):
    _check_wrapping_inputs(case)
    h = case['starts'].shape[1] // 2
    S = tr['S'][0, 0]
    assert not S[:h, h:].any() and not S[h:, :h].any() and tr['connected'][0, 0] == 0, case['name']
    assert (S[:h, :h] != 0).any(1).all() and (S[h:, h:] != 0).any(1).all(), case['name']
    assert _d2(case)[:h, h:].min() > 2 ** 31, case['name']


def _check_grown(case, tr):
    """The oracle's fp64 sequence 2.0 / 1.1 * 1.1 * 1.1 ... up to the first radius above the widest gap."""
    cells = np.sort(case['starts'][0].max(-1))
    gap = int(np.diff(cells).max())
    r = 2.0 / 1.1
    steps = 0
    while True:
        r, steps = r * 1.1, steps + 1
        if np.sqrt(float(gap * gap)) < r:
            break
    assert tr['connected'][0, 0] == 1 and tr['radius'][0, 0] == r, (case['name'], tr['radius'][0, 0], r)
    assert cells[0] == 0 and cells[-1] == THIN_SIDE - 1, case['name']
    if len(cells) == 2:
        _check_wrapping_inputs(case)
        assert steps > 100 and r > THIN_SIDE - 1 and (r / 1.1) ** 2 > 2 ** 31, (steps, r)   # the threshold passed 2^31


HUGE_RADIUS = 1e10


def _check_all_pairs(case, tr):
    """The oracle's answer at a radius beyond every distance: every pair an edge, the radius as it was given."""
    _check_wrapping_inputs(case)
    N = case['starts'].shape[1]
    assert ((tr['S'][0, 0] != 0) == ~np.eye(N, dtype=bool)).all() and tr['connected'][0, 0] == 1, case['name']
    assert tr['radius'][0, 0] == HUGE_RADIUS, case['name']


@functools.lru_cache(None)
def thin_cases():
    cases = []
    for o, (H, W) in enumerate(THIN_SHAPES):
        for N in THIN_SIZES:
            cells = _spread(N)
            seed = 1600 + 10 * N + o
            cases.append(_thin_case('spread', H, W, cells, 2.0, 0, _check_spread, seed))
            pair = cells.copy()
            pair[1] = pair[0] + 1
            cases.append(_thin_case('spread_and_one_pair', H, W, pair, 2.0, 0, _check_pair, seed + 1))
            if N > 2:
                ends = np.concatenate([np.arange(N // 2), THIN_SIDE - (N - N // 2) + np.arange(N - N // 2)])
                cases.append(_thin_case('two_ends', H, W, ends, 2.0, 0, _check_ends, seed + 2))
        for N in (2, 129):
            cases.append(_thin_case('grow', H, W, _spread(N), 2.0, 1, _check_grown, 1690 + 10 * N + o))
    # a radius whose square (1e20) is beyond a 64-bit integer, grow = 0: dist2_bound decides it on the double.  One-wave
    # (128) and team (129) kernels; lists_cases() below sends both through the neighbour-list call as well.
    for N in (128, 129):
        cases.append(_thin_case('radius_1e10', 1, THIN_SIDE, _spread(N), HUGE_RADIUS, 0, _check_all_pairs, 1700 + N))
    return cases


def all_cases():
    """Small maps first, the thin maps last."""
    return non_square_cases() + fov_cases() + map_load_cases() + team_size_cases() + team_dense_cases() + graph_cases() + \
        thin_cases()


# ---- the neighbour-list call -----------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def lists_cases():
    """The thin-map states and the 1024-agent chain as cases of rollout_lists_cases.run_lists_case."""
    cases = [dict(name='lists/' + c['name'], pos=c['starts'], radius=c['radius'], grow=c['grow']) for c in thin_cases()]
    for c in cases:
        if c['name'].endswith('/spread') or c['name'].endswith('/two_ends'):
            c['connected'] = [0]
        if c['name'].endswith('/grow') or c['name'].endswith('/radius_1e10'):
            c['connected'] = [1]
    cases.append(dict(name='lists/team_sim/chain1024', pos=lc._chain(1024, 3), radius=3.5, grow=0, connected=[1]))
    cases.append(dict(name='lists/team_sim/chain1024/broken_at_700', pos=_broken_chain(), radius=3.5, grow=0, connected=[0]))
    return tuple(cases)


# ---- device only: the team launchers' LDS requests --------------------------------------------------------------------------
# Restated from the launchers of csrc/rollout_team_kernels.hip (round16 = up to a multiple of 16):
#   move     16 N + 272 + round16(2 H W) bytes: more than 64 KB from H W = 31 601 on at N = 129, from 24 441 on at N = 1024;
#            147 728 at N = 1024 on 256 x 256;
#   observe  round16(8 N) + round16(H W) + 23 232 bytes: more than 64 KB from H W = 41 265 on at N = 129, from 34 113 on at
#            N = 1024; 96 960 at N = 1024 on 256 x 256.
# Both kernels' limits are raised once to 160 KB.  (H, W, N, what the shape is there for), small maps before large ones.
def requests(H, W, N):
    """(move bytes, observe bytes) of the team launchers, restated."""
    up = lambda v: (v + 15) & ~15                                              # noqa: E731
    return 16 * N + 272 + up(2 * H * W), up(8 * N) + up(H * W) + 23232


LDS_SHAPES = (
    (104, 235, 1024, 'move at N = 1024, the last request of 64 KB: 24 440 cells'),
    (3, 8147, 1024, 'move at N = 1024, the first request above 64 KB: 24 441 cells'),
    (158, 200, 129, 'move at N = 129, the last request of 64 KB: 31 600 cells'),
    (13, 2431, 129, 'move at N = 129, above 64 KB: 31 603 cells'),
    (104, 328, 1024, 'observe at N = 1024, the last request of 64 KB: 34 112 cells'),
    (137, 249, 1024, 'observe at N = 1024, the first request above 64 KB: 34 113 cells'),
    (16, 2579, 129, 'observe at N = 129, the last request of 64 KB: 41 264 cells'),
    (45, 917, 129, 'observe at N = 129, the first request above 64 KB: 41 265 cells'),
    (256, 256, 129, 'the largest accepted map, 129 agents'), (256, 256, 1024, 'the largest accepted map, 1024 agents'),
    (1, 65536, 1024, 'the largest accepted map as one row'), (65536, 1, 1024, 'the largest accepted map as one column'),
)
UNSUPPORTED_SHAPES = ((257, 256, 129),)


@functools.lru_cache(None)
def lds_cases():
    """Agents and goals drawn over the whole map.  N = 129: two episodes, two steps; N = 1024: one episode, one step."""
    cases = []
    for k, (H, W, N, _) in enumerate(LDS_SHAPES):
        big = N == 1024
        cases.append(_case('team_lds/%dx%d/N%d' % (H, W, N), *_random(1700 + k, 1 if big else 2, N, H, W, 0.03,
                                                                        T=1 if big else 2), maxstep=[1] if big else [50, 2]))
    f = {s[:3]: requests(*s[:3]) for s in LDS_SHAPES}
    # each threshold has a map on either side: the last cell count at 64 KB and the first (or, where that count is a
    # prime, the third) above it
    assert f[(104, 235, 1024)][0] == 65536 and f[(3, 8147, 1024)][0] == 65552 and requests(1, 24441, 1024)[0] == 65552
    assert f[(158, 200, 129)][0] == 65536 and f[(13, 2431, 129)][0] == 65552 and requests(1, 31601, 129)[0] == 65552
    assert f[(104, 328, 1024)][1] == 65536 and f[(137, 249, 1024)][1] == 65552
    assert f[(16, 2579, 129)][1] == 65536 and f[(45, 917, 129)][1] == 65552
    assert f[(256, 256, 1024)] == (147728, 96960) and f[(256, 256, 129)] == (133408, 89808)
    assert f[(1, 65536, 1024)] == f[(65536, 1, 1024)] == (147728, 96960)
    assert max(v[0] for v in f.values()) == 147728 and max(v[1] for v in f.values()) == 96960
    cells = [s[0] * s[1] for s in LDS_SHAPES]
    assert cells == sorted(cells)
    assert any(s[0] > 4 * s[1] or s[1] > 4 * s[0] for s in LDS_SHAPES[:8])     # non-square shapes among the thresholds
    return cases


@functools.lru_cache(None)
def unsupported_cases():
    return [_case('team_lds/%dx%d/N%d/unsupported' % (H, W, N), *_random(1800 + k, 2, N, H, W, 0.03, T=1))
            for k, (H, W, N) in enumerate(UNSUPPORTED_SHAPES)]
