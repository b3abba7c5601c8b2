"""A training batch drawn from stored schedules (gnnpp_schedule_draw, include/gnnpp_schedule_draw.h): the statement, the
host-array runner and the hand-built cases, each defined once (the case_* functions) and run twice: by
tests/test_emu_schedule_draw.py on the host emulation and by tests/test_gpu_schedule_draw_cases.py on the MI355X, where
expert_team_lists_cases.DeviceRunner gives every host array, poison and sentinel margins included, a twin in device
memory for the length of a call.  A plain helper module, not a conftest.

The statement: row b of the batch is row index[b] (clamped into the set) of what the EXISTING calls write for the same
schedules -- obs, target and S of gnnpp_schedule_team_samples, and the block gnnpp_team_lists_gather makes of the set of
gnnpp_schedule_team_fill_lists -- and all zeros (cnt = 0) where the step's case is flagged.  Every comparison is an
equality of bytes.  Outputs start poisoned with 0xFF bytes and sit between sentinel margins, so a row the call skipped
cannot pass for one it wrote and a write outside an array shows."""
import ctypes

import numpy as np

import expert_cases as ec
import expert_team_lists_cases as lc
from expert_team_lists_cases import ERR_ARG, ERR_UNSUPPORTED, ScheduleStruct, guarded, margins_intact, roundup4  # noqa: F401

BAD_MOVE = 1                                  # GNNPP_SCHEDULE_BAD_MOVE


# ---- the existing calls on a schedule set: the yardstick ------------------------------------------------------------
class ScheduleSet:
    """gnnpp_schedule_team_plan on host arrays (lc.HostCall: radius and status are what the draw reads), and on demand
    the materialised forms of the same set: dense() = gnnpp_schedule_team_samples, capped() = the filled lists."""

    def __init__(self, lib, grids, goals, schedules, radius0=5.0, run=None):
        self.lib, self.run = lib, run
        self.h = lc.HostCall(lib, grids, goals, schedules, radius0, run).plan()
        self.T, self.N, self.C = self.h.T, self.h.N, self.h.C
        self.status = self.h.out['status']
        self.case_of = np.searchsorted(self.h.start, np.arange(self.T), side='right') - 1
        self._dense = self._capped = None

    def dense(self):
        if self._dense is None:
            self._dense = self.h.dense()
        return self._dense

    def capped(self):
        if self._capped is None:
            self._capped = lc.HostCall(self.lib, self.h.grid, self.h.goal,
                                       [self.h.pos[a:b] for a, b in zip(self.h.start[:-1], self.h.start[1:])],
                                       self.h.s.radius0, self.run).plan()
            self._capped.fill(max(4, roundup4(self._capped.out['step_deg'].max())))
        return self._capped

    def steps(self, index):
        return np.clip(np.asarray(index, np.int64), 0, self.T - 1)

    def flagged(self, index):
        return self.status[self.case_of[self.steps(index)]] != 0

    def want_rows(self, index, key):
        """Rows `index` of the dense call's output `key` ('obs', 'target', 'S'); zeros for the steps of a flagged case."""
        rows = self.dense()[key][self.steps(index)].copy()
        rows[self.flagged(index)] = 0
        return rows

    def want_block(self, index):
        """(raw, block) of gnnpp_team_lists_gather of the filled set: the yardstick where no pick is flagged."""
        f = self.capped()
        return lc.host_gather(self.lib, f.lists(), f.T, f.cap, index, self.N, run=self.run, buffers=list(f.raw.values()))


# ---- one gnnpp_schedule_draw call on poisoned host arrays ------------------------------------------------------------
class Draw:
    """picks: the steps to draw.  Outputs 0xFF-poisoned between sentinel margins.  kw: arguments of the C call to replace, by their names there;
    (a callable gets the Draw, for a pointer into its arrays); mutate(struct): changes to the gnnpp_schedules copy the
    call gets; s_misalign: bytes added to the S pointer."""

    def __init__(self, sset, picks, graph='dense', expect=0, s_misalign=0, mutate=None, **kw):
        lib, h = sset.lib, sset.h
        self.sset, self.graph = sset, graph
        self.index = np.ascontiguousarray(picks, np.int32)
        B, N = len(self.index), sset.N
        self.B = B
        self.raw, self.view = {}, {}
        sizes = {'obs': B * N * 363 * 4, 'target': B * N * 5 * 4}
        if graph in ('dense', 'both'):                       # ('both': for the refusal of a call that names two outputs)
            sizes['S'] = B * N * N * 4
        if graph in ('lists', 'both'):
            sizes['lists'] = lib.gnnpp_team_lists_bytes(B, N)
        for k, n in sizes.items():
            self.raw[k], self.view[k] = guarded(n, misalign=s_misalign if k == 'S' else 0)
        self.need = lib.gnnpp_schedule_draw_workspace_bytes(N, B)
        self.ws = np.full(max(self.need, 8) // 8 + 1, np.nan, np.float64)
        s = ScheduleStruct()
        ctypes.memmove(ctypes.byref(s), ctypes.byref(h.s), ctypes.sizeof(s))
        s.obs = s.S = s.S64 = s.target = s.growth = s.step_info = None       # outputs of the sample calls: ignored
        s.radius0 = 0.0
        if mutate:
            mutate(s)
        self.s = s
        ptr = lambda k: self.view[k].ctypes.data if k in self.view else None  # noqa: E731
        a = dict(s=ctypes.byref(s), index=self.index.ctypes.data, B=B, obs=ptr('obs'), target=ptr('target'), S=ptr('S'),
                 lists=ptr('lists'), lists_bytes=sizes.get('lists', 0), workspace=self.ws.ctypes.data,
                 workspace_bytes=self.need)
        a.update({k: v(self) if callable(v) else v for k, v in kw.items()})      # (a callable: from this call's arrays)
        buffers = [h.grid, h.goal, h.pos, h.start, h.out['radius'], h.out['status'], self.index, self.ws] + \
            list(self.raw.values())
        rc = (sset.run or lc.host_run)(lib.gnnpp_schedule_draw,
                                       (a['s'], a['index'], a['B'], a['obs'], a['target'], a['S'], a['lists'],
                                        a['lists_bytes'], a['workspace'], a['workspace_bytes'], None), buffers)
        assert rc == expect, (rc, expect)
        self.obs = self.view['obs'].view(np.float32).reshape(B, N, 3, 11, 11)
        self.target = self.view['target'].view(np.float32).reshape(B, N, 5)
        self.S = self.view['S'].view(np.float32).reshape(B, N, N) if 'S' in self.view else None
        self.block = self.view.get('lists')

    def margins_intact(self):
        return all(margins_intact(self.raw[k], self.view[k]) for k in self.raw)

    def untouched(self):
        return self.margins_intact() and all((v == 0xFF).all() for v in self.view.values()) and np.isnan(self.ws).all()

    def bytes(self):
        return b''.join(self.raw[k].tobytes() for k in sorted(self.raw))


def assert_batch(name, sset, index, graph='dense', **kw):
    """One draw equals the yardstick's rows; returns the Draw."""
    d = Draw(sset, index, graph, **kw)
    assert d.margins_intact(), name
    assert d.obs.tobytes() == sset.want_rows(index, 'obs').tobytes(), (name, 'obs')
    assert d.target.tobytes() == sset.want_rows(index, 'target').tobytes(), (name, 'target')
    if graph == 'dense':
        assert d.S.tobytes() == sset.want_rows(index, 'S').tobytes(), (name, 'S')
        return d
    bad = sset.flagged(index)
    got = lc.block_views(d.block, d.B, sset.N)
    if not bad.any():                                    # the whole block, the poison behind every column included
        raw, want = sset.want_block(index)
        assert d.block.tobytes() == want.tobytes(), (name, 'lists')
    else:
        good = np.nonzero(~bad)[0]
        assert (got[0][bad] == 0).all(), (name, 'cnt of a flagged pick')
        raw, want = sset.want_block(np.asarray(index)[good])
        lc.same_lists(name, tuple(v[good] for v in got), lc.block_views(want, len(good), sset.N))
    lc.check_lists(name, *got, lc.lists_of_dense(sset.want_rows(index, 'S')))
    return d


def shuffled(T, seed):
    return np.random.default_rng(seed).permutation(T)


# ---- the cases: lib is the bound library, run the runner (None: host arrays, the emulation) ---------------------------
GOLDEN_SMALL = [0, 2]                          # cases of tests/golden/expert_schedules.npz
GOLDEN_TEAM = [1]                              # case of tests/golden/expert_schedules_team.npz (130 agents)


def case_golden(lib, kind, ci, graph, run=None, most=None):
    """Every step of a reference-made case in a fixed shuffled order: the reference's own input / GSO / target rows.
    most: draw only that many of the shuffled steps (the emulation's time)."""
    m, g = (ec.load_golden() if kind == 'small' else lc.load_team_golden())[ci]
    sset = ScheduleSet(lib, g['grid'], g['goal'][None], [g['schedule']], run=run)
    index = shuffled(sset.T, 100 + ci)[:most]
    d = assert_batch('golden %s %d' % (kind, ci), sset, index, graph)
    assert np.array_equal(d.obs, g['input'][index].astype(np.float32))
    assert np.array_equal(d.target, g['target'][index].astype(np.float32))
    S32 = g['GSO'][index].astype(np.float32)
    if graph == 'dense':
        assert d.S.tobytes() == S32.tobytes()
    else:
        lc.check_lists('golden lists', *lc.block_views(d.block, d.B, sset.N), lc.lists_of_dense(S32))


RANDOM = [(2, 6, 3), (5, 9, 4), (7, 12, 4), (130, 60, 3)]


def random_set(lib, N, side, steps, run=None):
    """Three cases of different lengths on one map size, a map per case."""
    cases = [lc.random_schedule(N, side, steps + k, 3000 + 10 * N + k, density=0.1) for k in range(3)]
    cases[1] = (cases[1][0], cases[1][2][1], cases[1][2][:1])           # a case of ONE step (its goal: the next state)
    return ScheduleSet(lib, np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), [c[2] for c in cases],
                       run=run)


def random_picks(sset):
    a = [int(v) for v in sset.h.start]
    T = sset.T
    return {'B1': [a[1]], 'repeats': [2, 2, 0, 2, T - 1, T - 1], 'first_and_last': [a[0], a[1] - 1, a[2], a[3] - 1],
            'straddle': [a[1] - 1, a[1], a[2] - 1, a[2], a[1] - 1]}


def case_random(lib, N, side, steps, graph, run=None):
    sset = random_set(lib, N, side, steps, run)
    assert len(set(np.diff(sset.h.start).tolist())) > 1 and (sset.status == 0).all()
    for name, index in random_picks(sset).items():
        assert_batch('random %d %s' % (N, name), sset, index, graph)


FAR = np.array([[0, 0], [0, 1], [0, 2], [20, 0], [20, 1], [20, 2]])          # two clusters 20 rows apart
CHAIN = np.array([[5, 5 + 3 * k] for k in range(6)])                          # a chain, three cells between neighbours


def radius_set(lib, run=None):
    """Six agents, two cases on an empty 30 x 30 map: in the first the team stands in two clusters 20 rows apart, so the
    radius grows until they meet; in the second it stands in a chain that radius0 = 5 connects."""
    grid = np.zeros((30, 30), np.uint8)
    sset = ScheduleSet(lib, grid, np.stack([FAR, CHAIN]), [np.stack([FAR] * 2), np.stack([CHAIN] * 3)], run=run)
    growth = sset.h.out['growth']
    assert growth[0] > 0 and growth[1] == 0 and sset.h.out['radius'][0] > 20 > 5.0 == sset.h.out['radius'][1]
    return sset


def case_per_case_radius(lib, graph, run=None):
    sset = radius_set(lib, run)
    S = sset.dense()['S']
    # So that the test can fail: the clusters of the first case are 20 cells apart, so under radius0 = 5 (or the second
    # case's radius) its S has no entry between them -- the yardstick's has all nine; and the chain's ends are 15 cells
    # apart, so under the first case's radius (> 20) the second case's S would be full -- the yardstick's is a chain.
    between = np.linalg.norm(FAR[:3, None] - FAR[None, 3:], axis=-1)
    assert (between > 5.0).all() and (S[0][:3, 3:] != 0).all() and (S[1][:3, 3:] != 0).all()
    assert np.abs(CHAIN[0] - CHAIN[-1]).max() == 15 and S[2][0, 5] == 0 and (np.diag(S[2], 1) != 0).all()
    assert_batch('radius', sset, [0, 2, 1, 4, 3], graph)


def thin_set(lib, H, W, run=None):
    """ec.walk_call on a strip (the team spread over it, both end cells occupied, a map per case, the second turned by
    180 degrees) and a third case whose agents stand eight cells from their goals: outside the field of view."""
    side, N = max(H, W), 17
    cells = ec._spread(N, side)
    step = np.where(np.arange(N) < N / 2, 1, -1)
    sched = ec._on_strip(H, np.stack([cells + t * step for t in range(8)]))
    far = (np.zeros((H, W), np.uint8), ec._on_strip(H, cells + 8 * step), sched)
    assert np.abs(far[1] - sched[0]).max() == 8
    call = ec.walk_call(H, W, N, extra=[far])
    return ScheduleSet(lib, call['grids'], call['goals'], call['schedules'], call['radius0'], run=run)


THIN = [(1, 2048), (2048, 1)]


def case_thin_map(lib, H, W, graph, run=None):
    sset = thin_set(lib, H, W, run)
    assert (sset.status == 0).all()
    assert_batch('thin %dx%d' % (H, W), sset, shuffled(sset.T, 5), graph)


def case_pointer_alignment(lib, run=None):
    """N % 4 == 0: S four bytes off a 16-byte boundary takes the 4-byte stores and gives the same bytes."""
    grid, goal, sched = lc.random_schedule(8, 9, 4, 808, density=0.1)
    sset = ScheduleSet(lib, grid, goal[None], [sched], run=run)
    index = [1, 0, sset.T - 1]
    aligned = assert_batch('aligned', sset, index)
    off = assert_batch('misaligned', sset, index, s_misalign=4)
    assert off.view['S'].ctypes.data % 16 == 4 and aligned.view['S'].ctypes.data % 16 == 0
    assert off.S.tobytes() == aligned.S.tobytes()


def flagged_set(lib, N, side, cases, where, run=None):
    """`cases` copies of one random case, copy `where` with a diagonal move: GNNPP_SCHEDULE_BAD_MOVE."""
    grid, goal, sched = lc.random_schedule(N, side, 4, 77 + N, density=0.0)
    bad = sched.copy()
    free = next(d for d in ([1, 1], [1, -1], [-1, 1], [-1, -1])
                if 0 <= bad[0, 0, 0] + d[0] < side and 0 <= bad[0, 0, 1] + d[1] < side)
    bad[1, 0] = bad[0, 0] + free
    sset = ScheduleSet(lib, grid, np.stack([goal] * cases), [bad if c == where else sched for c in range(cases)], run=run)
    assert sset.status[where] & BAD_MOVE and (np.delete(sset.status, where) == 0).all()
    return sset


def case_flagged(lib, N, side, cases, where, graph, run=None):
    sset = flagged_set(lib, N, side, cases, where, run)
    a = [int(v) for v in sset.h.start]
    index = [a[where - 1], a[where], a[where] + 1, a[where + 1] - 1, a[where + 1], sset.T - 1, a[where]]
    assert sset.flagged(index).tolist() == [False, True, True, True, False, False, True]
    d = assert_batch('flagged', sset, index, graph)
    bad = sset.flagged(index)
    assert (d.obs[bad].view(np.uint32) == 0).all() and (d.target[bad].view(np.uint32) == 0).all()
    if graph == 'dense':
        assert (d.S[bad].view(np.uint32) == 0).all()
    alone = assert_batch('good ones alone', sset, np.asarray(index)[~bad], graph)
    assert d.obs[~bad].tobytes() == alone.obs.tobytes() and d.target[~bad].tobytes() == alone.target.tobytes()


def case_index_clamping(lib, graph, run=None):
    sset = random_set(lib, 5, 9, 4, run)
    T = sset.T
    d = assert_batch('clamped', sset, [-1, T + 5, 0, T - 1, -(1 << 31), (1 << 31) - 1], graph)
    assert d.obs[0].tobytes() == d.obs[2].tobytes() == d.obs[4].tobytes()
    assert d.obs[1].tobytes() == d.obs[3].tobytes() == d.obs[5].tobytes()


def case_determinism(lib, graph, run=None):
    sset = random_set(lib, 7, 12, 4, run)
    index = [3, 3, 0, sset.T - 1]
    a, b = Draw(sset, index, graph), Draw(sset, index, graph)
    assert a.margins_intact() and b.margins_intact() and a.bytes() == b.bytes()


def case_argument_errors(lib, run=None):
    """Every refusal leaves obs, target, S / lists and the workspace poisoned."""
    sset = random_set(lib, 5, 9, 4, run)
    index = [0, 1, 2]
    assert not Draw(sset, index).untouched()                                   # (the call these are variations of)

    def refused(expect=ERR_ARG, graph='dense', **kw):
        assert Draw(sset, index, graph, expect=expect, **kw).untouched(), kw

    for null in ('index', 'obs', 'target', 'workspace', 's'):
        refused(**{null: None})
        refused(graph='lists', **{null: None})
    refused(S=None)                                                            # neither graph output ...
    refused(graph='both')                                                      # ... and both
    refused(graph='lists', lists=None)
    for field in ('grid', 'goal', 'pos', 'case_start', 'radius', 'status'):
        refused(mutate=lambda s, f=field: setattr(s, f, None))
    for B in (0, -1):
        refused(B=B)
    for field, value in (('C', 0), ('T_total', 0), ('H', 0), ('W', -1), ('N', 0), ('N', 1025), ('C', sset.T + 1)):
        refused(mutate=lambda s, f=field, v=value: setattr(s, f, v))
    for k in ('obs', 'target', 'S'):                                           # two bytes off: not a float's alignment
        refused(**{k: lambda d, k=k: d.view[k].ctypes.data + 2})
    refused(index=lambda d: d.index.ctypes.data + 2)
    refused(workspace=lambda d: d.ws.ctypes.data + 4)
    refused(mutate=lambda s: setattr(s, 'radius', s.radius + 4))
    refused(workspace_bytes=lambda d: d.need - 1)
    refused(graph='lists', lists=lambda d: d.view['lists'].ctypes.data + 8)
    refused(graph='lists', lists_bytes=lambda d: d.view['lists'].size - 1)
    refused(expect=ERR_UNSUPPORTED, mutate=lambda s: setattr(s, 'N', 1))
    refused(expect=ERR_UNSUPPORTED, mutate=lambda s: setattr(s, 'H', 256) or setattr(s, 'W', 257))
    assert lib.gnnpp_schedule_draw_workspace_bytes(5, 3) == 128              # [B, N] doubles, rounded up to 16 bytes
    for N, B in ((0, 1), (1025, 1), (5, 0), (-1, -1)):
        assert lib.gnnpp_schedule_draw_workspace_bytes(N, B) == 0
    assert lib.gnnpp_version() == 330
