"""CPU: the streamed rollout of large teams (csrc/rollout_team_stream_kernels.hip), compiled unmodified for the host emulation
and driven through the shared case tables (tests/rollout_team_stream_cases.py) behind the emulated large-team move kernel,
on the dense graph and on the neighbour lists: every per-case table equals the plain per-case rollout of the same scripts
exactly, the hand-derived case holds its written-out values, the seating order is the prefix rule, a freshly seated slot
holds the case's own step-0 state bit for bit (obs, S or its columns of the lists block, radius; connected = 1) and untouched
slots keep their bytes.  One mutant of the expectation shows that the hand-derived case can tell a wrong implementation."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rollout_team_stream_cases as tc                                              # noqa: E402
from test_emu_rollout_stream import _rollout                                        # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


def _lists_block(graphs, N):
    """(16-byte aligned uint8 view, its size)"""
    n = tc.lists_bytes(graphs, N)
    raw = np.zeros(n + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n], n


def plain_rollout(lib, tab):
    """The plain per-case rollout (B = C) of a table's scripts on the emulated gnnpp_rollout_* calls, with the step-0 state of
    every case on both graph forms; -> (read-backs for plain_expectation, {graph: dict(obs, S, radius)})."""
    C, N = tab['starts'].shape[:2]
    assert lib.gnnpp_team_lists_bytes(C, N) == tc.lists_bytes(C, N)
    r, a = _rollout(tab['grids'], tab['starts'], tab['goals'], tab['maxstep'], tab['commR'])
    r.grow = 1
    block, nbytes = _lists_block(C, N)
    assert lib.gnnpp_rollout_lists(ctypes.byref(r), block.ctypes.data, nbytes, None) == 0
    assert (a['connected'] == 1).all()
    radius_lists = a['radius'].copy()
    a['radius'][:] = tab['commR']
    a['connected'][:] = 0
    assert lib.gnnpp_rollout_observe(ctypes.byref(r), None) == 0 and lib.gnnpp_rollout_gso(ctypes.byref(r), None) == 0
    assert (a['connected'] == 1).all() and a['radius'].tobytes() == radius_lists.tobytes()
    fresh = {'dense': {'obs': a['obs'].copy(), 'S': a['S'].copy(), 'radius': a['radius'].copy()},
             'lists': {'obs': a['obs'].copy(), 'S': tc.lists_slots(block, C, N), 'radius': radius_lists}}
    frozen = []
    for t in range(int(tab['maxstep'].max())):
        acts = np.ascontiguousarray(tc.plain_actions(tab, t))
        frozen.append((a['done'] != 0) | (t + 1 > a['maxstep']))
        r.logits, r.actions, r.currentstep = None, acts.ctypes.data, t + 1
        assert lib.gnnpp_rollout_move(ctypes.byref(r), None) == 0
    assert (a['done'] != 0).all()
    return {'reached': a['reached'], 'start_step': a['start_step'], 'end_step': a['end_step'], 'pos': a['pos'],
            'stats': a['stats'], 'radius': radius_lists, 'frozen': np.stack(frozen)}, fresh


class EmuTeamEngine:
    """The engine of the shared driver over numpy arrays and the emulated library."""

    def __init__(self, lib, tab, graph):
        from gnn_pathplanning_amd._native import RolloutStreamStruct
        self.lib, self.tab, self.graph = lib, tab, graph
        C, N = tab['starts'].shape[:2]
        B = min(tab['slots'], C)
        self.B, self.C, self.N = B, C, N
        per_case = tc.batched(tab)
        self.q = {'grid': np.ascontiguousarray(tab['grids'], np.uint8), 'start': np.ascontiguousarray(tab['starts'], np.int32),
                  'goal': np.ascontiguousarray(tab['goals'], np.int32),
                  'maxstep': np.ascontiguousarray(tab['maxstep'], np.int32)}
        self.r, self.a = _rollout(self.q['grid'][:B] if per_case else self.q['grid'], self.q['start'][:B],
                                  self.q['goal'][:B], self.q['maxstep'][:B], tab['commR'])
        if not per_case:                                     # the one shared map IS the rollout's map
            self.a['grid'] = self.q['grid']
            self.r.grid = self.q['grid'].ctypes.data
        self.block, self.nbytes = (None, 0)
        if graph == 'lists':                                 # no dense S at all
            self.block, self.nbytes = _lists_block(B, N)
            self.r.S = None
            del self.a['S']
        i32 = np.int32
        self.s_arr = {'cursor': np.full(1, 77, i32), 'case': np.full(B, 77, i32), 't0': np.full(B, 77, i32),
                      'assign': np.full(B, 77, i32), 'reached': np.full((C, N), 77, i32),
                      'start_step': np.full((C, N), 77, i32), 'end_step': np.full((C, N), 77, i32),
                      'pos': np.full((C, N, 2), 77, i32), 'radius': np.full(C, 77.0), 'stats': np.full((C, 2), 77, i32),
                      'lived': np.full(C, 77, i32), 'slot': np.full(C, 77, i32), 'case_t0': np.full(C, 77, i32)}
        x, q, a = self.s_arr, self.q, self.a
        s = RolloutStreamStruct()
        s.case_grid, s.case_grid_batched = q['grid'].ctypes.data, int(per_case)
        s.case_start, s.case_goal, s.case_maxstep = q['start'].ctypes.data, q['goal'].ctypes.data, q['maxstep'].ctypes.data
        s.C, s.commR = C, tab['commR']
        s.cursor, s.slot_case, s.slot_t0, s.assign = (x[k].ctypes.data for k in ('cursor', 'case', 't0', 'assign'))
        s.slot_grid = a['grid'].ctypes.data if per_case else None
        s.goal, s.maxstep = a['goal'].ctypes.data, a['maxstep'].ctypes.data
        s.reached, s.start_step, s.end_step, s.pos = (x[k].ctypes.data for k in ('reached', 'start_step', 'end_step', 'pos'))
        s.radius, s.stats, s.lived, s.slot, s.t0 = (x[k].ctypes.data for k in ('radius', 'stats', 'lived', 'slot', 'case_t0'))
        self.s = s
        assert lib.gnnpp_rollout_team_stream_begin(ctypes.byref(self.r), ctypes.byref(s), None) == 0
        assert (a['done'] == 1).all() and (x['case'] == -1).all() and x['cursor'][0] == 0 and (x['lived'] == -1).all()
        assert (x['radius'] == -1.0).all() and (x['pos'] == -1).all() and (x['stats'] == -1).all()
        self.before_harvest = []                             # (case, r->stats row) as a harvest finds them

    def reseat(self, now):
        for b in np.flatnonzero((self.a['done'] != 0) & (self.s_arr['case'] >= 0)):
            self.before_harvest.append((int(self.s_arr['case'][b]), self.a['stats'][b].copy()))
        self.a['connected'][:] = -5
        lists = self.block.ctypes.data if self.block is not None else None
        assert self.lib.gnnpp_rollout_team_stream_reseat(ctypes.byref(self.r), ctypes.byref(self.s), now, lists, self.nbytes,
                                                         None) == 0
        seated = self.s_arr['assign'] >= 0
        assert (self.a['connected'][seated] == 1).all() and (self.a['connected'][~seated] == -5).all()

    def move(self, actions, step):
        acts = np.ascontiguousarray(actions, np.int32)
        self.r.logits, self.r.actions, self.r.currentstep = None, acts.ctypes.data, step
        assert self.lib.gnnpp_rollout_move(ctypes.byref(self.r), None) == 0

    def read(self, name):
        if name == 'S' and self.block is not None:
            return tc.lists_slots(self.block, self.B, self.N)
        return (self.s_arr[name] if name in ('case', 't0', 'assign', 'cursor') else self.a[name]).copy()

    def tables(self):
        x = self.s_arr
        return {'reached': x['reached'], 'start_step': x['start_step'], 'end_step': x['end_step'], 'pos': x['pos'],
                'radius': x['radius'], 'makespan': x['stats'][:, 0], 'flowtime': x['stats'][:, 1], 'lived': x['lived'],
                'slot': x['slot'], 't0': x['case_t0']}


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.load()


_plain, _runs = {}, {}


def _run(lib, name, graph):
    if name not in _plain:                                   # the reference: once per table, shared and left unchanged
        _plain[name] = plain_rollout(lib, tc.table(name))
    if (name, graph) not in _runs:
        tab = tc.table(name)
        plain, fresh = _plain[name]
        eng = EmuTeamEngine(lib, tab, graph)
        got, seats = tc.run_stream(eng, tab, fresh[graph])
        _runs[name, graph] = (tab, tc.plain_expectation(plain), got, seats, eng)
    return _runs[name, graph]


@pytest.mark.parametrize('graph', tc.GRAPHS)
@pytest.mark.parametrize('name', tc.TABLE_NAMES)
def test_emu_team_stream_table(emu, name, graph):
    tab, want, got, seats, _ = _run(emu, name, graph)
    tc.assert_tables(tab, got, want)
    tc.assert_seats(tab, seats, got)


def test_emu_team_stream_growth_table_grows(emu):
    """The commR = 1.0 table is what it claims: no case is connected at commR, every seat multiplied the radius often."""
    tab, want, got, _, _ = _run(emu, 'growth_n129_commR1', 'dense')
    assert (got['radius'] > 1.1 ** 4).all() and (got['t0'][2:] > 0).all()


def test_emu_team_stream_mutant_flowtime_from_stats(emu):
    """One-off mutant: makespan and flowtime taken from r->stats as the harvest finds them, instead of being recomputed from
    the relative records.  The hand-derived case (seated at t0 > 0) must tell: stats counts a missing start as GLOBAL step
    0, so every agent that only stays adds t0 to the flowtime."""
    tab, want, got, _, eng = _run(emu, 'hand_n129_20x20', 'dense')
    c = tab['named']['one_walker']
    mutant = {case: stats for (case, stats) in eng.before_harvest}
    assert sorted(mutant) == list(range(eng.C))
    t0 = int(got['t0'][c])
    assert t0 > 0 and got['flowtime'][c] == 131 and got['makespan'][c] == 3
    assert mutant[c][1] == 131 + 128 * t0 and mutant[c][0] == t0 + 3
