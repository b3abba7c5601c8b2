"""Capped neighbour lists from expert schedules (gnnpp_schedule_team_plan / _fill_lists / gnnpp_team_lists_gather): the
numpy restatement of "the lists of a dense S" and the host-array runner shared by tests/test_emu_expert_team_lists.py
(host emulation) and tests/test_gpu_expert_team_lists.py (MI355X).  A plain helper module, not a conftest.

Every comparison is an equality: the work is integers, {0, 1} values and fp64 products in a fixed order.
Outputs start poisoned (0xFF bytes: count -1, index 65535, weight NaN), and the three lists arrays sit between sentinel
margins, so an element the call does not write cannot pass for one it wrote and a write outside an array shows."""
import ctypes
import json
import os

import numpy as np

ERR_ARG, ERR_UNSUPPORTED = -1, -2
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


def bind(lib):
    """ctypes prototypes of the calls on a raw CDLL (the emulated library)."""
    from gnn_pathplanning_amd._native import ScheduleStruct
    vp, ci, cs = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    sp = ctypes.POINTER(ScheduleStruct)
    for name, args, res in (('gnnpp_schedule_team_workspace_bytes', [ci, ci], cs),
                            ('gnnpp_schedule_team_samples', [sp, vp, cs, vp], ci),
                            ('gnnpp_schedule_team_plan', [sp, vp, cs, vp, vp], ci),
                            ('gnnpp_schedule_team_fill_lists', [sp, vp, cs, vp, vp, vp, ci, vp], ci),
                            ('gnnpp_team_lists_gather', [vp, vp, vp, ci, ci, vp, ci, vp, cs, ci, vp], ci),
                            ('gnnpp_team_lists_bytes', [ci, ci], cs),
                            ('gnnpp_team_lists_from_dense', [vp, vp, cs, ci, ci, ci, vp], ci),
                            ('gnnpp_team_lists_transpose', [vp, vp, cs, ci, ci, vp], ci)):
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = res
    return lib


PLAN_OUTPUTS = ('target', 'radius', 'growth', 'status', 'step_info')


class HostCall:
    """The inputs of one call on host arrays and poisoned outputs; plan() / fill(cap) / dense() run the three entry
    points on them.  `ws` is the fp64 workspace (one spare element, poisoned)."""

    def __init__(self, lib, grids, goals, schedules, radius0=5.0):
        from gnn_pathplanning_amd._native import ScheduleStruct
        self.lib = lib
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
        rc = self.lib.gnnpp_schedule_team_plan(ctypes.byref(self.s), self.ws.ctypes.data if ws else None,
                                               self.need if ws_bytes is None else ws_bytes,
                                               self.out['step_deg'].ctypes.data if step_deg else None, None)
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
        rc = self.lib.gnnpp_schedule_team_fill_lists(ctypes.byref(self.s), self.ws.ctypes.data if ws else None,
                                                     self.need if ws_bytes is None else ws_bytes, p['cnt'], p['idx'],
                                                     p['val'], cap if pass_cap is None else pass_cap, None)
        assert rc == expect, rc
        return self

    def lists(self):
        return self.out['cnt'], self.out['idx'], self.out['val']

    def lists_untouched(self):
        return all((self.out[k].view(np.uint8) == 0xFF).all() and margins_intact(self.raw[k], self.out[k].view(np.uint8).reshape(-1))
                   for k in ('cnt', 'idx', 'val'))

    def margins_intact(self):
        return all(margins_intact(self.raw[k], self.out[k].view(np.uint8).reshape(-1)) for k in ('cnt', 'idx', 'val'))

    def dense(self):
        """gnnpp_schedule_team_samples on the same inputs: dict of its outputs (S fp32 included), poisoned first."""
        from gnn_pathplanning_amd._native import ScheduleStruct
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
        assert self.lib.gnnpp_schedule_team_samples(ctypes.byref(s), ws.ctypes.data, self.need, None) == 0
        out['ws'] = ws
        return out


def plan_and_fill(lib, grids, goals, schedules, radius0=5.0, extra=0):
    """plan, cap = roundup4(max step_deg) + extra, fill."""
    h = HostCall(lib, grids, goals, schedules, radius0).plan()
    return h.fill(max(4, roundup4(h.out['step_deg'].max())) + extra)


def host_gather(lib, capped, n_src, width, pick, nodes, expect=0, **kw):
    """gnnpp_team_lists_gather of host (cnt, idx, val) = capped, n_src graphs of `nodes` nodes at cap = width, into a
    fresh 0xFF-filled block: (raw, block uint8).  kw: arguments of the C call to replace, by their names there."""
    cnt, idx, val = capped
    index = np.ascontiguousarray(pick, np.int32)
    B = len(index)
    nbytes = lib.gnnpp_team_lists_bytes(B, nodes)
    raw, block = guarded(nbytes)
    a = dict(cnt=cnt.ctypes.data, idx=idx.ctypes.data, val=val.ctypes.data, graphs_src=n_src, cap=width,
             index=index.ctypes.data, B=B, lists=block.ctypes.data, lists_bytes=nbytes, N=nodes)
    a.update(kw)
    rc = lib.gnnpp_team_lists_gather(a['cnt'], a['idx'], a['val'], a['graphs_src'], a['cap'], a['index'], a['B'],
                                     a['lists'], a['lists_bytes'], a['N'], None)
    assert rc == expect, rc
    return raw, block
