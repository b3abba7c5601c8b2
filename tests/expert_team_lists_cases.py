"""Capped neighbour lists from expert schedules (gnnpp_schedule_team_plan / _fill_lists / gnnpp_team_lists_gather): the
numpy restatement of "the lists of a dense S", the host-array runner and the hand-built cases, each defined once (the
case_* functions) and run twice: by tests/test_emu_expert_team_lists.py on the host emulation and by
tests/test_gpu_expert_team_lists_cases.py on the MI355X, where DeviceRunner gives every host array, poison and sentinel
margins included, a twin in device memory for the length of a call.  A plain helper module, not a conftest.

Every comparison is an equality: the work is integers, {0, 1} values and fp64 products in a fixed order.
Outputs start poisoned (0xFF bytes: count -1, index 65535, weight NaN), and the three lists arrays sit between sentinel
margins, so an element the call does not write cannot pass for one it wrote and a write outside an array shows."""
import ctypes
import json
import os

import numpy as np

from gnn_pathplanning_amd._native import ERR_ARG, ERR_UNSUPPORTED, ScheduleStruct  # noqa: F401 (the tests' names)

MARGIN = 64                                   # sentinel bytes on both sides of cnt / idx / val
SENTINEL = 0xA5


def roundup4(v):
    return (int(v) + 3) & ~3


def load_team_golden():
    """[(meta, dict of arrays)] of tests/golden/expert_schedules_team.npz (tools/gen_expert_golden_team.py)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'expert_schedules_team.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    keys = ('grid', 'goal', 'schedule', 'input', 'GSO', 'target')
    return [(m, {k: z['c%d_%s' % (ci, k)] for k in keys}) for ci, m in enumerate(meta)]


# ---- the statement -----------------------------------------------------------------------------------------------
def lists_of_dense(S32):
    """Per graph and column of S32 [graphs,N,N] float32: (ascending non-zero rows, their float32 weights)."""
    S32 = np.asarray(S32)
    assert S32.dtype == np.float32
    return [[(np.nonzero(S32[g, :, n])[0], S32[g, np.nonzero(S32[g, :, n])[0], n]) for n in range(S32.shape[1])]
            for g in range(S32.shape[0])]


def check_lists(name, cnt, idx, val, want, graphs=None, cap=None):
    """cnt [G,N] int32, idx [G,N,stride] uint16, val [G,N,stride] float32 are "the lists of a dense S" for want =
    lists_of_dense(S): cnt = the number of non-zeros, indices ascending, weights the fp32 values of S, zero padding up to
    roundup4(cnt).  graphs: (graph in the arrays, graph in want) pairs (default: all, in order).  cap: compare only
    the first `cap` entries of a column (a set filled below its need); cnt is the true degree all the same."""
    pairs = [(g, g) for g in range(len(want))] if graphs is None else graphs
    assert idx.dtype == np.uint16 and val.dtype == np.float32 and cnt.dtype == np.int32
    for g, gw in pairs:
        for n in range(len(want[gw])):
            rows, w = want[gw][n]
            k = len(rows)
            assert cnt[g, n] == k, (name, g, n, int(cnt[g, n]), k)
            k4 = roundup4(k)
            if cap is not None and k4 > cap:
                k = k4 = cap
            assert (idx[g, n, :k] == rows[:k]).all() and (idx[g, n, k:k4] == 0).all(), (name, g, n)
            assert val[g, n, :k].tobytes() == np.asarray(w[:k], np.float32).tobytes(), (name, g, n)
            assert val[g, n, k:k4].tobytes() == bytes(4 * (k4 - k)), (name, g, n)


def same_lists(name, a, b):
    """Two (cnt, idx, val) triples agree over cnt and the first roundup4(cnt) entries of every column."""
    (ca, ia, va), (cb, ib, vb) = a, b
    assert (ca == cb).all(), name
    w = min(ia.shape[2], ib.shape[2])
    assert ((ca + 3) & ~3).max() <= w, name
    live = np.arange(w)[None, None, :] < ((ca + 3) & ~3)[:, :, None]
    assert (ia[:, :, :w][live] == ib[:, :, :w][live]).all(), name
    assert va[:, :, :w][live].tobytes() == vb[:, :, :w][live].tobytes(), name


def block_views(block, graphs, N):
    """cnt, idx, val views of a standard lists block (uint8 numpy), restated from include/gnnpp.h."""
    Np = roundup4(N)
    up = lambda v: (v + 15) & ~15                                              # noqa: E731
    io = up(graphs * N * 4)
    vo = io + up(graphs * N * Np * 2)
    assert block.dtype == np.uint8 and block.size >= vo + up(graphs * N * Np * 4)
    return (block[:graphs * N * 4].view(np.int32).reshape(graphs, N),
            block[io:io + graphs * N * Np * 2].view(np.uint16).reshape(graphs, N, Np),
            block[vo:vo + graphs * N * Np * 4].view(np.float32).reshape(graphs, N, Np))


# ---- host arrays ----------------------------------------------------------------------------------------------------
def guarded(nbytes, fill=0xFF, misalign=0):
    """(raw uint8 array, view of nbytes bytes filled with `fill`, 16-byte aligned + misalign, between two sentinel
    margins of MARGIN bytes)."""
    raw = np.full(nbytes + 2 * MARGIN + 32, SENTINEL, np.uint8)
    off = MARGIN + (-(raw.ctypes.data + MARGIN) % 16) + misalign
    view = raw[off:off + nbytes]
    view[:] = fill
    assert (view.ctypes.data - misalign) % 16 == 0
    return raw, view


def margins_intact(raw, view):
    off = view.ctypes.data - raw.ctypes.data
    return bool((raw[:off] == SENTINEL).all() and (raw[off + view.size:] == SENTINEL).all())


def host_run(fn, args, buffers):
    """A call on the host arrays themselves (the emulated library)."""
    return fn(*args)


class DeviceRunner:
    """run(fn, args, buffers) for the library on the device: every array of `buffers` (each owns its memory) gets a twin
    in device memory with the same bytes -- poison and sentinel margins included -- and the same address modulo 16;
    every pointer among the arguments and in a gnnpp_schedules struct is moved to its twin; the call runs on the null
    stream; then every writable array takes its twin's bytes back.  A pointer into no buffer is an error: it must
    never reach the device."""

    def __init__(self, device):
        import torch
        self.torch, self.device = torch, torch.device(device)

    def __call__(self, fn, args, buffers):
        torch = self.torch
        regions = []
        for b in buffers:
            assert b.flags.c_contiguous
            flat = b.reshape(-1).view(np.uint8)
            twin = torch.empty(flat.size + 16, dtype=torch.uint8, device=self.device)
            shift = (flat.ctypes.data - twin.data_ptr()) % 16
            if flat.size:
                twin[shift:shift + flat.size].copy_(torch.from_numpy(flat.copy()))
            regions.append((flat.ctypes.data, flat, twin, shift))

        def moved(p):
            if p is None or p == 0:
                return None
            for base, flat, twin, shift in regions:
                if base <= p < base + max(flat.size, 1):
                    return twin.data_ptr() + shift + (p - base)
            raise AssertionError('pointer %#x lies in none of the buffers of the call' % p)

        def arg(a):
            s = getattr(a, '_obj', None)
            if isinstance(s, ctypes.Structure):
                t = type(s)()
                ctypes.memmove(ctypes.byref(t), ctypes.byref(s), ctypes.sizeof(s))
                for name, kind in s._fields_:
                    if kind is ctypes.c_void_p:
                        setattr(t, name, moved(getattr(s, name)))
                keep.append(t)
                return ctypes.byref(t)
            if isinstance(a, int) and a >= 1 << 32:              # an address (sizes and counts are far below)
                return moved(a)
            return a

        keep = []
        on_device = self.device.type == 'cuda'           # ('cpu': the twins are host memory, for the emulated library)
        if on_device:
            torch.cuda.synchronize()
        rc = fn(*[arg(a) for a in args])
        if on_device:
            torch.cuda.synchronize()
        for base, flat, twin, shift in regions:
            if flat.size and flat.flags.writeable:
                flat[:] = twin[shift:shift + flat.size].cpu().numpy()
        return rc


PLAN_OUTPUTS = ('target', 'radius', 'growth', 'status', 'step_info')


class HostCall:
    """The inputs of one call on host arrays and poisoned outputs; plan() / fill(cap) / dense() run the three entry
    points on them.  `ws` is the fp64 workspace (one spare element, poisoned)."""

    def __init__(self, lib, grids, goals, schedules, radius0=5.0, run=None):
        self.lib = lib
        self.run = run or host_run
        self.grid = np.ascontiguousarray(grids, dtype=np.uint8)
        self.goal = np.ascontiguousarray(goals, dtype=np.int32)
        self.C, self.N = self.goal.shape[:2]
        self.pos = np.ascontiguousarray(np.concatenate(schedules, 0), dtype=np.int32)
        self.start = np.ascontiguousarray(np.cumsum([0] + [len(s) for s in schedules]), dtype=np.int32)
        T, N, C = int(self.start[-1]), self.N, self.C
        self.T = T
        nan = np.nan
        self.out = {'obs': np.full((T, N, 3, 11, 11), nan, np.float32), 'target': np.full((T, N, 5), nan, np.float32),
                    'radius': np.full(C, nan, np.float64), 'growth': np.full(C, -1, np.int32),
                    'status': np.full(C, -1, np.int32), 'step_info': np.full(T, -1, np.int32),
                    'step_deg': np.full(T, -1, np.int32)}
        self.need = lib.gnnpp_schedule_team_workspace_bytes(N, T)
        self.ws = np.full(max(self.need, 8) // 8 + 1, nan, np.float64)
        s = ScheduleStruct()
        s.grid, s.grid_batched, s.goal, s.pos = (self.grid.ctypes.data, int(self.grid.ndim == 3), self.goal.ctypes.data,
                                                 self.pos.ctypes.data)
        s.case_start, s.C, s.N, s.H, s.W, s.T_total = self.start.ctypes.data, C, N, self.grid.shape[-2], self.grid.shape[-1], T
        s.radius0 = radius0
        s.obs, s.S, s.S64, s.target = self.out['obs'].ctypes.data, None, None, self.out['target'].ctypes.data
        s.radius, s.growth, s.status = (self.out[k].ctypes.data for k in ('radius', 'growth', 'status'))
        s.step_info = self.out['step_info'].ctypes.data
        self.s = s

    def plan(self, expect=0, ws_bytes=None, ws=True, step_deg=True):
        rc = self.run(self.lib.gnnpp_schedule_team_plan,
                      (ctypes.byref(self.s), self.ws.ctypes.data if ws else None,
                       self.need if ws_bytes is None else ws_bytes,
                       self.out['step_deg'].ctypes.data if step_deg else None, None), self.buffers())
        assert rc == expect, rc
        return self

    def alloc_lists(self, cap, misalign=(0, 0, 0)):
        T, N = self.T, self.N
        self.cap = cap
        self.raw = {}
        for k, size, dt, mis in (('cnt', 4, np.int32, misalign[0]), ('idx', 2 * cap, np.uint16, misalign[1]),
                                 ('val', 4 * cap, np.float32, misalign[2])):
            self.raw[k], view = guarded(T * N * size, misalign=mis)
            self.out[k] = view.view(dt).reshape((T, N) if k == 'cnt' else (T, N, cap))     # (mis: a multiple of 4)
        return self

    def fill(self, cap, expect=0, ws_bytes=None, ws=True, misalign=(0, 0, 0), null=None, pass_cap=None):
        """cap: what the arrays are sized for; pass_cap: what the call is told (default: cap)."""
        self.alloc_lists(cap, misalign)
        p = {k: (None if k == null else self.out[k].ctypes.data) for k in ('cnt', 'idx', 'val')}
        rc = self.run(self.lib.gnnpp_schedule_team_fill_lists,
                      (ctypes.byref(self.s), self.ws.ctypes.data if ws else None,
                       self.need if ws_bytes is None else ws_bytes, p['cnt'], p['idx'], p['val'],
                       cap if pass_cap is None else pass_cap, None), self.buffers())
        assert rc == expect, rc
        return self

    def buffers(self):
        """The arrays a call may read or write: inputs, outputs that own their memory, the workspace, and the three
        lists arrays with their margins."""
        own = [v for k, v in self.out.items() if k not in ('cnt', 'idx', 'val')]
        return [self.grid, self.goal, self.pos, self.start, self.ws] + own + list(getattr(self, 'raw', {}).values())

    def lists(self):
        return self.out['cnt'], self.out['idx'], self.out['val']

    def lists_untouched(self):
        return all((self.out[k].view(np.uint8) == 0xFF).all() and margins_intact(self.raw[k], self.out[k].view(np.uint8).reshape(-1))
                   for k in ('cnt', 'idx', 'val'))

    def margins_intact(self):
        return all(margins_intact(self.raw[k], self.out[k].view(np.uint8).reshape(-1)) for k in ('cnt', 'idx', 'val'))

    def dense(self):
        """gnnpp_schedule_team_samples on the same inputs: dict of its outputs (S fp32 included), poisoned first."""
        T, N, C = self.T, self.N, self.C
        out = {'obs': np.full((T, N, 3, 11, 11), np.nan, np.float32), 'target': np.full((T, N, 5), np.nan, np.float32),
               'radius': np.full(C, np.nan, np.float64), 'growth': np.full(C, -1, np.int32),
               'status': np.full(C, -1, np.int32), 'step_info': np.full(T, -1, np.int32)}
        raw, view = guarded(T * N * N * 4)
        out['S'] = view.view(np.float32).reshape(T, N, N)
        s = ScheduleStruct()
        ctypes.memmove(ctypes.byref(s), ctypes.byref(self.s), ctypes.sizeof(s))
        s.obs, s.S, s.target = out['obs'].ctypes.data, out['S'].ctypes.data, out['target'].ctypes.data
        s.radius, s.growth, s.status = (out[k].ctypes.data for k in ('radius', 'growth', 'status'))
        s.step_info = out['step_info'].ctypes.data
        ws = np.full(max(self.need, 8) // 8 + 1, np.nan, np.float64)
        assert self.run(self.lib.gnnpp_schedule_team_samples, (ctypes.byref(s), ws.ctypes.data, self.need, None),
                        [self.grid, self.goal, self.pos, self.start, ws, raw] +
                        [v for k, v in out.items() if k != 'S']) == 0
        out['ws'] = ws
        return out


def plan_and_fill(lib, grids, goals, schedules, radius0=5.0, extra=0, run=None):
    """plan, cap = roundup4(max step_deg) + extra, fill."""
    h = HostCall(lib, grids, goals, schedules, radius0, run).plan()
    return h.fill(max(4, roundup4(h.out['step_deg'].max())) + extra)


def host_gather(lib, capped, n_src, width, pick, nodes, expect=0, run=None, buffers=(), **kw):
    """gnnpp_team_lists_gather of host (cnt, idx, val) = capped, n_src graphs of `nodes` nodes at cap = width, into a
    fresh 0xFF-filled block: (raw, block uint8).  kw: arguments of the C call to replace, by their names there.
    buffers: the arrays that own capped's memory (for a runner that mirrors them on the device)."""
    cnt, idx, val = capped
    index = np.ascontiguousarray(pick, np.int32)
    B = len(index)
    nbytes = lib.gnnpp_team_lists_bytes(B, nodes)
    raw, block = guarded(nbytes)
    a = dict(cnt=cnt.ctypes.data, idx=idx.ctypes.data, val=val.ctypes.data, graphs_src=n_src, cap=width,
             index=index.ctypes.data, B=B, lists=block.ctypes.data, lists_bytes=nbytes, N=nodes)
    a.update(kw)
    rc = (run or host_run)(lib.gnnpp_team_lists_gather,
                           (a['cnt'], a['idx'], a['val'], a['graphs_src'], a['cap'], a['index'], a['B'], a['lists'],
                            a['lists_bytes'], a['N'], None), list(buffers) + [index, raw])
    assert rc == expect, rc
    return raw, block


# ---- the hand-built cases: lib is the bound library, run the runner (None: host arrays, the emulation) -------------------
def assert_plan_outputs_equal_dense(h, dense, obs=True):
    """target, radius, growth, status, step_info, the workspace (and obs) byte for byte what the dense call writes --
    NaN poison included: the same elements are left unwritten."""
    for k in PLAN_OUTPUTS + (('obs',) if obs else ()):
        assert h.out[k].tobytes() == dense[k].tobytes(), k
    assert h.ws.tobytes() == dense['ws'].tobytes()


def random_schedule(N, side, steps, seed, **kw):
    import expert_cases as ec
    rng = np.random.default_rng(seed)
    grid, goal, paths = ec.random_case(rng, N, side, side, max_steps=steps, **kw)
    return grid, goal, ec.schedule_of(paths, goal)


def want_gso(grid, goal, sched, radius0=5.0):
    import expert_cases as ec
    return ec.reference_samples(grid, goal, sched, radius0)['GSO'].astype(np.float32)


def chain7():
    """Seven agents waiting in a row, four cells apart: at most two neighbours each under radius 5."""
    pos = np.stack([np.zeros(7, np.int64), 4 * np.arange(7)], 1)
    return np.zeros((1, 30), np.uint8), pos, np.stack([pos, pos])


TINY_MAPS = [(2, 3), (5, 4), (7, 4), (130, 17)]


def case_tiny_map_where_everybody_neighbours_everybody(lib, N, side, run=None):
    """radius0 = 30 spans the whole map: degree N - 1 everywhere.  cap = roundup4(N - 1), which is roundup4(N) -- the
    standard block's stride -- unless N = 1 mod 4; at N = 5 the degree 4 IS cap: a column without padding."""
    grid, goal, sched = random_schedule(N, side, 3, 40 + N, density=0.0)
    h = plan_and_fill(lib, grid, goal[None], [sched], radius0=30.0, run=run)
    assert (h.out['step_deg'] == N - 1).all() and h.cap == roundup4(N - 1)
    assert h.cap == (roundup4(N) if N % 4 != 1 else N - 1)
    assert (h.out['cnt'] == N - 1).all()
    check_lists('full %d' % N, *h.lists(), lists_of_dense(want_gso(grid, goal, sched, 30.0)))
    assert h.margins_intact()
    assert_plan_outputs_equal_dense(h, h.dense())


def case_set_four_entries_wider_than_needed(lib, N, run=None):
    """The tail of every column stays poison (a chain of 7 at the standard stride 8; a random team of 130)."""
    grid, goal, sched = chain7() if N == 7 else random_schedule(N, 60, 3, 1000 + N, density=0.1)
    want = lists_of_dense(want_gso(grid, goal, sched))
    h = plan_and_fill(lib, grid, goal[None], [sched], run=run)
    assert h.cap + 4 <= roundup4(N)
    wide = plan_and_fill(lib, grid, goal[None], [sched], extra=4, run=run)
    assert wide.cap == h.cap + 4
    check_lists('wide %d' % N, *wide.lists(), want)
    assert (wide.out['idx'][:, :, h.cap:] == 0xFFFF).all()
    assert (wide.out['val'][:, :, h.cap:].view(np.uint32) == 0xFFFFFFFF).all()
    assert wide.margins_intact()
    same_lists('wide %d' % N, wide.lists(), h.lists())


def case_largest_degree_exactly_cap(lib, run=None):
    """129 agents on a 17 x 17 map that radius0 = 30 spans: degree 128 = cap, below the standard stride of 132; every
    column is full, no padding anywhere, and the last store of a column ends where the next column begins."""
    N = 129
    grid, goal, sched = random_schedule(N, 17, 2, 7, density=0.0)
    h = plan_and_fill(lib, grid, goal[None], [sched], radius0=30.0, run=run)
    assert h.cap == 128 and (h.out['cnt'] == 128).all() and h.cap < roundup4(N)
    check_lists('exact', *h.lists(), lists_of_dense(want_gso(grid, goal, sched, 30.0)))
    assert h.margins_intact()


def case_flagged_case_between_two_good_ones(lib, run=None):
    N = 130
    grid, goal, sched = random_schedule(N, 44, 3, 5, density=0.1)
    bad = sched.copy()
    bad[1, 70] = np.argwhere(grid != 0)[0]              # a state on an obstacle
    h = HostCall(lib, grid, np.stack([goal] * 3), [sched, bad, sched], run=run).plan()
    T = len(sched)
    assert h.out['status'][0] == 0 and h.out['status'][1] != 0 and h.out['status'][2] == 0
    assert (h.out['step_deg'][T:2 * T] == 0).all() and (h.out['step_deg'][:T] > 0).all()
    h.fill(max(4, roundup4(h.out['step_deg'].max())))
    want = lists_of_dense(want_gso(grid, goal, sched))
    check_lists('left', *h.lists(), want, graphs=[(t, t) for t in range(T)])
    check_lists('right', *h.lists(), want, graphs=[(2 * T + t, t) for t in range(T)])
    for k in ('cnt', 'idx', 'val'):                     # the flagged case's steps stay poison
        assert (h.out[k][T:2 * T].view(np.uint8) == 0xFF).all(), k
    assert np.isnan(h.out['obs'][T:2 * T]).all() and np.isnan(h.out['target'][T:2 * T]).all()
    assert h.margins_intact()
    assert_plan_outputs_equal_dense(h, h.dense())
    alone = plan_and_fill(lib, grid, goal[None], [sched], run=run)
    for k in ('cnt', 'idx', 'val', 'obs'):              # the neighbours are unaffected
        assert h.out[k][:T].tobytes() == alone.out[k].tobytes() == h.out[k][2 * T:].tobytes(), k


SHORT_CAPS = [(130, 60, 5.0), (7, 4, 30.0)]


def case_cap_four_below_the_need(lib, N, side, radius0, run=None):
    """cnt is the true degree, the first cap entries are right, nothing is written outside a column's cap entries."""
    grid, goal, sched = random_schedule(N, side, 3, 1000 + N, density=0.1 if N > 7 else 0.0)
    h = HostCall(lib, grid, goal[None], [sched], radius0, run).plan()
    need = roundup4(h.out['step_deg'].max())
    assert need >= 8
    h.fill(need - 4)
    assert (h.out['cnt'] > need - 4).any() and h.out['cnt'].max() == h.out['step_deg'].max()
    check_lists('short %d' % N, *h.lists(), lists_of_dense(want_gso(grid, goal, sched, radius0)), cap=need - 4)
    assert h.margins_intact()
    full = HostCall(lib, grid, goal[None], [sched], radius0, run).plan().fill(need)
    assert (h.out['cnt'] == full.out['cnt']).all()
    live = np.arange(need - 4)[None, None, :] < ((full.out['cnt'] + 3) & ~3)[:, :, None]
    assert (h.out['idx'][live] == full.out['idx'][:, :, :need - 4][live]).all()


# -- thin maps: the calls of tests/expert_cases.py on 1 x 65 536 and 65 536 x 1 through plan, fill and gather
def _thin_calls():
    import expert_cases as ec
    side = ec.THIN_SIDE
    return {'both_ends/1x65536': lambda: ec.both_ends_call(1, side), 'both_ends/65536x1': lambda: ec.both_ends_call(side, 1),
            'two_ends/1x65536/N129': lambda: ec.two_ends_call(1, side, 129),
            'two_ends/65536x1/N129': lambda: ec.two_ends_call(side, 1, 129),
            # radius0 * 1.1^3 = 64 513.57 spans the gap of 64 513 cells and no more: the halves meet in ONE pair, and the
            # largest degree is 512 = N / 2 (from radius0 = 5 the final radius of 68 903 makes every pair an edge: 1023)
            'two_ends/1x65536/N1024': lambda: ec.two_ends_call(1, side, 1024, radius0=48470.0),
            'spread/1x65536/N129': lambda: ec.spread_call(1, side, 129),
            'spread/65536x1/N129': lambda: ec.spread_call(side, 1, 129),
            'walk/1x65536/N129': lambda: ec.walk_call(1, side, 129), 'walk/65536x1/N129': lambda: ec.walk_call(side, 1, 129),
            'status_bits/1x65536/N129': ec.thin_status_bits_call}


THIN_CALLS = sorted(_thin_calls())
THIN_SHORT_CAPS = ['two_ends/1x65536/N1024', 'two_ends/65536x1/N129']     # needs of 512 and of 128 (every pair an edge)


def case_thin_map(lib, name, run=None, short=False):
    """step_deg = the largest degree of the restatement's graph; the lists are those of its S (float32); the margins keep
    their bytes; every other output is the dense call's; the gather into the standard block matches.  A flagged case of
    the call has step_deg 0 and keeps its poison.  short: the fill runs with cap four below the need."""
    import expert_cases as ec
    call = _thin_calls()[name]()
    wants = ec.call_wants(call)
    bounds = np.cumsum([0] + [len(s) for s in call['schedules']])
    h = HostCall(lib, call['grids'], call['goals'], call['schedules'], call['radius0'], run).plan()
    built, deg = [], np.zeros(h.T, np.int64)
    for c, want in enumerate(wants):
        a, b = int(bounds[c]), int(bounds[c + 1])
        if want is None:
            assert h.out['status'][c] != 0 and (h.out['step_deg'][a:b] == 0).all()
            continue
        assert h.out['status'][c] == 0 and h.out['radius'][c] == want['radius'] and h.out['growth'][c] == want['growth']
        deg[a:b] = (want['GSO'] != 0).sum(1).max(1)
        built += [(a + t, c, t) for t in range(b - a)]
    assert (h.out['step_deg'] == deg).all(), (h.out['step_deg'], deg)
    need = max(4, roundup4(deg.max()))
    if name == 'two_ends/1x65536/N1024':                # half the team each: a cap that is a multiple of 4 at N / 2
        assert deg.max() == 512 and deg.min() == 512 and need == 512 and wants[0]['growth'] == 3
        assert sorted((wants[0]['GSO'][0] != 0).sum(1).tolist()) == [511] * 1022 + [512] * 2
    cap = need - 4 if short else need
    assert cap >= 4
    h.fill(cap)
    for c, want in enumerate(wants):
        a, b = int(bounds[c]), int(bounds[c + 1])
        if want is None:
            for k in ('cnt', 'idx', 'val'):
                assert (h.out[k][a:b].view(np.uint8) == 0xFF).all(), k
            assert np.isnan(h.out['obs'][a:b]).all() and np.isnan(h.out['target'][a:b]).all()
            continue
        check_lists(name, *h.lists(), lists_of_dense(want['GSO'].astype(np.float32)),
                    graphs=[(a + t, t) for t in range(b - a)], cap=cap if short else None)
        assert np.array_equal(h.out['obs'][a:b], want['input']) and np.array_equal(h.out['target'][a:b], want['target'])
    assert h.margins_intact()
    if short:
        assert (h.out['cnt'] > cap).any() and h.out['cnt'].max() == deg.max()
        return
    dense = h.dense()
    assert_plan_outputs_equal_dense(h, dense)
    steps = [g for g, _, _ in built]
    index = steps[::-1][:3]                              # (a standard block at N = 1024 is 6 MB per graph)
    raw, block = host_gather(lib, h.lists(), h.T, h.cap, index, h.N, run=run, buffers=list(h.raw.values()))
    assert margins_intact(raw, block)
    S32 = np.stack([wants[c]['GSO'][t] for g, c, t in built[::-1][:3]]).astype(np.float32)
    assert S32.tobytes() == dense['S'][index].tobytes()
    check_lists('gather ' + name, *block_views(block, len(index), h.N), lists_of_dense(S32))


# -- gnnpp_team_lists_gather
def gather_pool(lib, run=None):
    """The capped set of the 5 steps of a 130-agent case and its dense S."""
    grid, goal, sched = random_schedule(130, 60, 5, 2030, density=0.1)
    h = plan_and_fill(lib, grid, goal[None], [sched], run=run)
    return h, h.dense()['S']


def lists_block_of_dense(lib, S, run=None):
    graphs, N = S.shape[:2]
    nbytes = lib.gnnpp_team_lists_bytes(graphs, N)
    raw, block = guarded(nbytes)
    S = np.ascontiguousarray(S)
    assert (run or host_run)(lib.gnnpp_team_lists_from_dense,
                             (S.ctypes.data, block.ctypes.data, nbytes, graphs, N, 0, None), [S, raw]) == 0
    return block


GATHERS = {'identity': [0, 1, 2, 3, 4], 'repeated': [2, 2, 0, 2], 'reversed': [4, 3, 2, 1, 0], 'B1': [3]}


def case_gather(lib, pool, index, run=None):
    h, S = pool
    N, B = h.N, len(index)
    lists_raw = list(h.raw.values())
    raw, block = host_gather(lib, h.lists(), h.T, h.cap, index, N, run=run, buffers=lists_raw)
    assert margins_intact(raw, block)
    got = block_views(block, B, N)
    want = lists_block_of_dense(lib, S[index], run)
    same_lists('gather', got, block_views(want, B, N))
    check_lists('gather', *got, lists_of_dense(S[index]))
    nbytes = lib.gnnpp_team_lists_bytes(B, N)                                  # symmetry: the lists of S^T are the same
    rawt, blockt = guarded(nbytes)
    assert (run or host_run)(lib.gnnpp_team_lists_transpose,
                             (block.ctypes.data, blockt.ctypes.data, nbytes, B, N, None), [raw, rawt]) == 0
    same_lists('transpose', got, block_views(blockt, B, N))
    # entries behind roundup4(cnt) are not copied
    cnt, idx, _ = got
    behind = np.arange(idx.shape[2])[None, None, :] >= ((cnt + 3) & ~3)[:, :, None]
    assert (idx[behind] == 0xFFFF).all()


def case_gather_clamps_an_index_out_of_range(lib, pool, run=None):
    """include/gnnpp.h: an index outside [0, graphs_src) is clamped into that range."""
    h, S = pool
    raw, block = host_gather(lib, h.lists(), h.T, h.cap, [-3, 5, 1 << 30, 1], h.N, run=run,
                             buffers=list(h.raw.values()))
    assert margins_intact(raw, block)
    check_lists('clamped', *block_views(block, 4, h.N), lists_of_dense(S[[0, 4, 4, 1]]))


def case_gather_from_a_set_at_the_standard_stride(lib, run=None):
    """cap == roundup4(N), N % 4 != 0: the three arrays are the regions of a standard block."""
    N = 7
    grid, goal, sched = random_schedule(N, 4, 3, 47, density=0.0)
    h = plan_and_fill(lib, grid, goal[None], [sched], radius0=30.0, run=run)
    assert h.cap == 8 == roundup4(N)
    raw, block = host_gather(lib, h.lists(), h.T, h.cap, np.arange(h.T), N, run=run, buffers=list(h.raw.values()))
    for a, b in zip(block_views(block, h.T, N), h.lists()):
        assert a.tobytes() == b.tobytes()
    assert margins_intact(raw, block)
