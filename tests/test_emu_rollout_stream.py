"""CPU: the streamed rollout's kernels (csrc/rollout_stream_kernels.hip), compiled unmodified for the host emulation,
driven through the shared case table (tests/rollout_stream_cases.py) behind the emulated move kernel: every per-case
table equals the plain per-case rollout of the same script exactly, the hand-derived cases hold their written-out values,
the seating order is the prefix rule, a freshly seated slot holds the case's own step-0 state bit for bit and untouched
slots keep their bytes.  Two one-off mutants of the tables show that the named cases can tell a wrong implementation."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rollout_stream_cases as sc                                                   # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


def _rollout(grids, starts, goals, maxstep, commR=sc.COMM_R):
    """A gnnpp_rollout over numpy arrays (B = the leading size of starts); -> (struct, arrays)."""
    from gnn_pathplanning_amd._native import RolloutStruct
    B, N = starts.shape[:2]
    a = {'grid': np.ascontiguousarray(grids, np.uint8).copy(), 'pos': np.ascontiguousarray(starts, np.int32).copy(),
         'goal': np.ascontiguousarray(goals, np.int32).copy(), 'maxstep': np.ascontiguousarray(maxstep, np.int32).copy(),
         'obs': np.zeros((B, N, 3, 11, 11), np.float32), 'S': np.zeros((B, N, N), np.float32),
         'radius': np.full(B, commR, np.float64), 'connected': np.zeros(B, np.int32),
         'reached': np.zeros((B, N), np.int32), 'start_step': np.full((B, N), -1, np.int32),
         'end_step': np.full((B, N), -1, np.int32), 'flags': np.zeros((B, 3), np.int32),
         'stats': np.zeros((B, 2), np.int32), 'done': np.zeros(B, np.int32), 'ccount': np.zeros(B, np.int32)}
    r = RolloutStruct()
    r.grid, r.grid_batched, r.goal, r.pos = a['grid'].ctypes.data, int(a['grid'].ndim == 3), a['goal'].ctypes.data, \
        a['pos'].ctypes.data
    r.B, r.N, r.H, r.W = B, N, a['grid'].shape[-2], a['grid'].shape[-1]
    r.obs, r.radius, r.S, r.connected = a['obs'].ctypes.data, a['radius'].ctypes.data, a['S'].ctypes.data, \
        a['connected'].ctypes.data
    r.reached, r.start_step, r.end_step = a['reached'].ctypes.data, a['start_step'].ctypes.data, a['end_step'].ctypes.data
    r.maxstep, r.flags, r.stats, r.done = a['maxstep'].ctypes.data, a['flags'].ctypes.data, a['stats'].ctypes.data, \
        a['done'].ctypes.data
    r.tie_mode, r.choice_count = 0, a['ccount'].ctypes.data
    return r, a


def plain_rollout(lib, tab):
    """The plain per-case rollout (B = C) of a table's scripts on the emulated gnnpp_rollout_* calls, with the step-0 state
    of every case; -> (read-backs for sc.plain_expectation, dict(obs, S, radius) of step 0)."""
    r, a = _rollout(tab['grids'], tab['starts'], tab['goals'], tab['maxstep'])
    r.grow = 1
    assert lib.gnnpp_rollout_observe(ctypes.byref(r), None) == 0 and lib.gnnpp_rollout_gso(ctypes.byref(r), None) == 0
    fresh = {'obs': a['obs'].copy(), 'S': a['S'].copy(), 'radius': a['radius'].copy()}
    frozen = []
    for t in range(int(tab['maxstep'].max())):
        acts = np.ascontiguousarray(sc.plain_actions(tab, t))
        frozen.append((a['done'] != 0) | (t + 1 > a['maxstep']))
        r.logits, r.actions, r.currentstep = None, acts.ctypes.data, t + 1
        assert lib.gnnpp_rollout_move(ctypes.byref(r), None) == 0
    assert (a['done'] != 0).all()
    return {'reached': a['reached'], 'start_step': a['start_step'], 'end_step': a['end_step'], 'pos': a['pos'],
            'stats': a['stats'], 'radius': fresh['radius'], 'frozen': np.stack(frozen)}, fresh


class EmuEngine:
    """The engine of sc.run_stream over numpy arrays and the emulated library."""

    def __init__(self, lib, tab):
        from gnn_pathplanning_amd._native import RolloutStreamStruct
        self.lib, self.tab = lib, tab
        C, N = tab['starts'].shape[:2]
        B = min(tab['slots'], C)
        self.B, self.C, self.N = B, C, N
        per_case = sc.batched(tab)
        self.q = {'grid': np.ascontiguousarray(tab['grids'], np.uint8), 'start': np.ascontiguousarray(tab['starts'], np.int32),
                  'goal': np.ascontiguousarray(tab['goals'], np.int32),
                  'maxstep': np.ascontiguousarray(tab['maxstep'], np.int32)}
        self.r, self.a = _rollout(self.q['grid'][:B] if per_case else self.q['grid'], self.q['start'][:B],
                                  self.q['goal'][:B], self.q['maxstep'][:B])
        if not per_case:                                     # the one shared map IS the rollout's map
            self.a['grid'] = self.q['grid']
            self.r.grid = self.q['grid'].ctypes.data
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
        s.C, s.commR = C, sc.COMM_R
        s.cursor, s.slot_case, s.slot_t0, s.assign = (x[k].ctypes.data for k in ('cursor', 'case', 't0', 'assign'))
        s.slot_grid = a['grid'].ctypes.data if per_case else None
        s.goal, s.maxstep = a['goal'].ctypes.data, a['maxstep'].ctypes.data
        s.reached, s.start_step, s.end_step, s.pos = (x[k].ctypes.data for k in ('reached', 'start_step', 'end_step', 'pos'))
        s.radius, s.stats, s.lived, s.slot, s.t0 = (x[k].ctypes.data for k in ('radius', 'stats', 'lived', 'slot', 'case_t0'))
        self.s = s
        assert lib.gnnpp_rollout_stream_begin(ctypes.byref(self.r), ctypes.byref(s), None) == 0
        assert (a['done'] == 1).all() and (x['case'] == -1).all() and x['cursor'][0] == 0 and (x['lived'] == -1).all()
        assert (x['radius'] == -1.0).all() and (x['pos'] == -1).all() and (x['stats'] == -1).all()
        self.before_harvest = []                             # (case, r->stats row, r->start_step row) as a harvest finds them

    def reseat(self, now):
        for b in np.flatnonzero((self.a['done'] != 0) & (self.s_arr['case'] >= 0)):
            self.before_harvest.append((int(self.s_arr['case'][b]), self.a['stats'][b].copy(), self.a['radius'][b]))
        assert self.lib.gnnpp_rollout_stream_reseat(ctypes.byref(self.r), ctypes.byref(self.s), now, None) == 0

    def move(self, actions, step):
        acts = np.ascontiguousarray(actions, np.int32)
        self.r.logits, self.r.actions, self.r.currentstep = None, acts.ctypes.data, step
        assert self.lib.gnnpp_rollout_move(ctypes.byref(self.r), None) == 0

    def read(self, name):
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


_runs = {}


def _run(lib, name):
    if name not in _runs:
        tab = sc.table(name)
        plain, fresh = plain_rollout(lib, tab)
        eng = EmuEngine(lib, tab)
        got, seats = sc.run_stream(eng, tab, fresh)
        _runs[name] = (tab, sc.plain_expectation(plain), got, seats, eng)
    return _runs[name]


@pytest.mark.parametrize('name', sc.TABLE_NAMES)
def test_emu_stream_table(emu, name):
    tab, want, got, seats, _ = _run(emu, name)
    sc.assert_tables(tab, got, want)
    sc.assert_seats(tab, seats, got)


def test_emu_stream_two_runs_give_the_same_bytes(emu):
    tab = sc.table('n4_6x6_every4')
    a, _ = sc.run_stream(EmuEngine(emu, tab), tab)
    b, _ = sc.run_stream(EmuEngine(emu, tab), tab)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_emu_stream_mutant_tables_read_from_stats(emu):
    """One-off mutant: makespan and flowtime taken from r->stats as the harvest finds them, instead of being recomputed
    from the relative records.  The named cases (seated at t0 > 0) must tell: stats counts a missing start as GLOBAL step 0."""
    tab, want, got, _, eng = _run(emu, 'hand_n2_6x6')
    mutant = {c: stats for (c, stats, _) in eng.before_harvest}
    assert sorted(mutant) == list(range(eng.C))
    wrong = [c for c in range(eng.C) if (mutant[c] != [want['makespan'][c], want['flowtime'][c]]).any()]
    for name in ('stays_on_goal', 'never_moved'):
        c = tab['named'][name]
        assert got['t0'][c] > 0 and c in wrong, (name, c, got['t0'][c], mutant[c])
    assert all(got['t0'][c] > 0 for c in wrong)             # (at t0 = 0 the two agree: a plain rollout)


def test_emu_stream_mutant_seat_without_radius_growth(emu):
    """One-off mutant: a seat that builds the graph at commR without the step-0 radius search (gnnpp_rollout_gso with
    grow = 0 on the case alone).  The named case must tell: its graph is not connected at commR and its radius differs."""
    tab, want, got, _, _ = _run(emu, 'growth_n3_24x24')
    c = tab['named']['needs_growth']
    r, a = _rollout(tab['grids'], tab['starts'][c:c + 1], tab['goals'][c:c + 1], tab['maxstep'][c:c + 1])
    r.grow = 0
    assert emu.gnnpp_rollout_gso(ctypes.byref(r), None) == 0
    assert a['connected'][0] == 0 and a['radius'][0] == sc.COMM_R
    assert got['radius'][c] == want['radius'][c] and got['radius'][c] > 2 * sc.COMM_R    # several multiplications by 1.1
    assert got['t0'][c] > 0
