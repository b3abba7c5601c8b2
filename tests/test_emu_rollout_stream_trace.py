"""CPU: the streamed rollout's recorder (csrc/rollout_stream_trace_kernels.hip), compiled unmodified for the host emulation,
behind the emulated move kernel, over the shared case table of streamed rollouts.  Every case's tables equal, exactly, the
trace of the PLAIN per-case rollout (B = C) of the same scripts recorded by gnnpp_rollout_trace_begin / _record; two named
cases hold values written out by hand; a numpy restatement of the rule agrees with the kernel and, with one fault switched
on, is told apart by the named cases (a wrong row index, a missing comparison with the seat); two runs give the same bytes;
empty slots and cases that never got a move leave the tables as begin left them; the words behind every array stay."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rollout_stream_cases as sc                                                   # noqa: E402
import rollout_stream_trace_cases as stc                                            # noqa: E402
from test_emu_rollout_stream import EmuEngine, _rollout                              # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')

POISON = np.int32(0x5a5a5a5a)


class HostStreamTrace:
    """A gnnpp_rollout_stream_trace over numpy buffers LARGER than the trace: a row of poison behind path and action and a
    poisoned word behind every other array; everything starts as poison, so begin must set all of it."""

    def __init__(self, B, C, N, T_cap):
        from gnn_pathplanning_amd._native import RolloutStreamTraceStruct
        self.B, self.C, self.N, self.T_cap = B, C, N, T_cap
        self.sizes = {'path': C * (T_cap + 1) * N * 2, 'action': C * T_cap * N, 'moves': C * N, 'shielded': C * N,
                      'steps': C, 'seen_done': B}
        self.buf = {k: np.full(n + (2 * N if k in ('path', 'action') else 1), 0x5a if k == 'action' else POISON,
                               np.int8 if k == 'action' else np.int32) for k, n in self.sizes.items()}
        s = RolloutStreamTraceStruct()
        for k in self.sizes:
            setattr(s, k, self.buf[k].ctypes.data)
        s.T_cap = T_cap
        self.s = s

    def arrays(self):
        C, N, T = self.C, self.N, self.T_cap
        shape = {'path': (C, T + 1, N, 2), 'action': (C, T, N), 'moves': (C, N), 'shielded': (C, N), 'steps': (C,),
                 'seen_done': (self.B,)}
        return {k: self.buf[k][:n].reshape(shape[k]) for k, n in self.sizes.items()}

    def poison_intact(self):
        return all((self.buf[k][n:] == (0x5a if k == 'action' else POISON)).all() for k, n in self.sizes.items())


class TracedEngine(EmuEngine):
    """EmuEngine whose move() calls gnnpp_rollout_move and then the streamed record, and keeps a log of what each move
    left for stc.model."""

    def __init__(self, lib, tab):
        super().__init__(lib, tab)
        self.tr = HostStreamTrace(self.B, self.C, self.N, stc.t_cap(tab))
        assert lib.gnnpp_rollout_stream_trace_begin(ctypes.byref(self.r), ctypes.byref(self.s), ctypes.byref(self.tr.s),
                                                    None) == 0
        got = self.tr.arrays()
        assert (got['path'] == 0).all() and (got['action'] == -1).all() and (got['steps'] == -1).all()
        assert not got['moves'].any() and not got['shielded'].any() and not got['seen_done'].any()
        assert self.tr.poison_intact()
        self.log = []

    def record(self):
        return self.lib.gnnpp_rollout_stream_trace_record(ctypes.byref(self.r), ctypes.byref(self.s),
                                                          ctypes.byref(self.tr.s), None)

    def move(self, actions, step):
        super().move(actions, step)
        empty = self.s_arr['case'] < 0
        before = {k: v.copy() for k, v in self.tr.arrays().items()} if empty.all() else None
        seen_before = self.tr.arrays()['seen_done'].copy()
        assert self.record() == 0
        assert (self.tr.arrays()['seen_done'][empty] == seen_before[empty]).all(), 'an empty slot wrote its seen_done'
        if before is not None:
            assert all(v.tobytes() == before[k].tobytes() for k, v in self.tr.arrays().items())
        self.log.append({'t': step, 'case': self.s_arr['case'].copy(), 't0': self.s_arr['t0'].copy(),
                         'maxstep': self.a['maxstep'].copy(), 'actions': np.array(actions, np.int32),
                         'pos': self.a['pos'].copy(), 'done': self.a['done'].copy()})


def plain_trace(lib, tab):
    """The plain per-case rollout (B = C) of a table's scripts, recorded by the EXISTING recorder on the emulation."""
    from gnn_pathplanning_amd._native import RolloutTraceStruct
    r, a = _rollout(tab['grids'], tab['starts'], tab['goals'], tab['maxstep'])
    C, N = tab['starts'].shape[:2]
    T = stc.t_cap(tab)
    out = {'path': np.zeros((C, T + 1, N, 2), np.int32), 'action': np.zeros((C, T, N), np.int8),
           'moves': np.zeros((C, N), np.int32), 'shielded': np.zeros((C, N), np.int32), 'steps': np.zeros(C, np.int32),
           'seen_done': np.zeros(C, np.int32)}
    s = RolloutTraceStruct()
    for k, v in out.items():
        setattr(s, k, v.ctypes.data)
    s.T_cap = T
    assert lib.gnnpp_rollout_trace_begin(ctypes.byref(r), ctypes.byref(s), None) == 0
    for t in range(T):
        acts = np.ascontiguousarray(sc.plain_actions(tab, t))
        r.logits, r.actions, r.currentstep = None, acts.ctypes.data, t + 1
        assert lib.gnnpp_rollout_move(ctypes.byref(r), None) == 0
        assert lib.gnnpp_rollout_trace_record(ctypes.byref(r), ctypes.byref(s), None) == 0
    assert (a['done'] != 0).all()
    return out


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.load()


_runs = {}


def _run(lib, name):
    if name not in _runs:
        tab = sc.table(name)
        eng = TracedEngine(lib, tab)
        tables, _ = sc.run_stream(eng, tab)
        _runs[name] = (tab, plain_trace(lib, tab), {k: v.copy() for k, v in eng.tr.arrays().items()}, tables, eng)
    return _runs[name]


@pytest.mark.parametrize('name', sc.TABLE_NAMES)
def test_emu_stream_trace_table(emu, name):
    tab, want, got, tables, eng = _run(emu, name)
    stc.assert_case_traces(tab, got, want, lived=tables['lived'])
    assert eng.tr.poison_intact()
    # the numpy restatement of the rule, fed with what each move left, agrees with the kernel in every word
    mine = stc.model(tab, eng.log, eng.B)
    for k in stc.KEYS + ('seen_done',):
        assert np.array_equal(mine[k], got[k]), (name, k)


def test_emu_stream_trace_hand_values(emu):
    """steps, moves, shielded, every row of path and every asked action of the two named cases, written out by hand; both
    are seated at t0 > 0, into slots that held a case before."""
    tab, _, got, tables, _ = _run(emu, 'hand_n2_6x6')
    for key in ('stays_on_goal', 'never_moved'):
        c = tab['named'][key]
        assert tables['t0'][c] > 0
        stc.assert_hand(got, c, key)


def test_emu_stream_trace_mutant_rows_by_global_step(emu):
    """One-off mutant: rows indexed by the global step t instead of t - t0.  Every named case of the hand table is seated
    at t0 > 0 and must tell; a case seated at 0 cannot."""
    tab, _, got, tables, eng = _run(emu, 'hand_n2_6x6')
    wrong = stc.model(tab, eng.log, eng.B, mutant='global_rows')
    named = [c for c in tab['named'].values() if tables['t0'][c] > 0]
    assert len(named) == len(tab['named']) >= 2              # such cases exist in the table
    for c in named:
        assert stc.tells(wrong, got, c), c
        assert wrong['steps'][c] != got['steps'][c]
    assert not any(stc.tells(wrong, got, c) for c in range(eng.C) if tables['t0'][c] == 0)


@pytest.mark.parametrize('name', ['n4_6x6_every4', 'corridor_n2_1x5', 'n65_16x16_shared_every4'])
def test_emu_stream_trace_mutant_no_rewind(emu, name):
    """One-off mutant: frozen decided by seen_done[b] != 0 && seen_done[b] < t, with no comparison to t0 -- the word a
    previous tenant left then freezes the next one for good.  With reseat_every = 4, every case seated into a slot whose
    previous tenant ended must tell, whether that tenant ended several moves before the seat or (n4_6x6_every4 holds such
    a pair) in the move right before it."""
    tab, _, got, tables, eng = _run(emu, name)
    assert tab['reseat_every'] == 4
    wrong = stc.model(tab, eng.log, eng.B, mutant='no_t0')
    later = stc.successors(tables['slot'], tables['t0'], tables['lived'])
    assert later and all(gap >= 0 for _, _, gap in later)
    for c, _, gap in later:
        assert stc.tells(wrong, got, c) and wrong['steps'][c] == -1, (name, c, gap)
    assert not any(stc.tells(wrong, got, c) for c in range(eng.C) if tables['t0'][c] == 0)
    assert any(gap > 0 for _, _, gap in later)
    if name == 'n4_6x6_every4':
        assert any(gap == 0 for _, _, gap in later), later      # the boundary: ended in move t', seated at now = t'


def test_emu_stream_trace_boundary_every_step(emu):
    """reseat_every = 1: every reseated case follows a tenant that ended in the move right before the seat (the record
    behind that move stored seen_done = t0), and is recorded from its first step."""
    tab, want, got, tables, eng = _run(emu, 'hand_n2_6x6')
    later = stc.successors(tables['slot'], tables['t0'], tables['lived'])
    assert later and all(gap == 0 for _, _, gap in later)
    wrong = stc.model(tab, eng.log, eng.B, mutant='no_t0')
    assert all(wrong['steps'][c] == -1 and got['steps'][c] >= 1 for c, _, _ in later)


def test_emu_stream_trace_two_runs_give_the_same_bytes(emu):
    tab = sc.table('n4_6x6_every4')
    runs = []
    for _ in range(2):
        eng = TracedEngine(emu, tab)
        sc.run_stream(eng, tab)
        runs.append(eng.tr)
    for k in runs[0].buf:
        assert runs[0].buf[k].tobytes() == runs[1].buf[k].tobytes(), k


def test_emu_stream_trace_drained_queue_leaves_the_tables(emu):
    """Once the queue is drained and every slot is empty, further moves and records change no byte (seen_done included);
    while the stream ran, TracedEngine.move checked the same for every slot that was already empty."""
    tab = sc.table('c2_lt_slots')
    eng = TracedEngine(emu, tab)
    sc.run_stream(eng, tab)
    assert (eng.s_arr['case'] == -1).all()
    before = {k: v.copy() for k, v in eng.tr.buf.items()}
    now = len(eng.log)
    for t in (now + 1, now + 2):
        eng.move(np.zeros((eng.B, eng.N), np.int32), t)
    assert all(eng.tr.buf[k].tobytes() == before[k].tobytes() for k in before)


def test_emu_stream_trace_seated_but_never_moved(emu):
    """A reseat in the middle of a stream (what results() does) seats cases that then never get a move: they read
    steps = -1 and their rows are what begin left."""
    tab = sc.table('n4_6x6_every4')
    eng = TracedEngine(emu, tab)
    eng.reseat(0)
    for now in range(2):
        eng.move(sc.script_actions(tab, eng.read('case'), eng.read('t0'), now), now + 1)
    held = set(eng.read('case').tolist())
    eng.reseat(2)                                            # off the period of 4, like results()
    fresh = sorted(set(eng.read('case').tolist()) - held)
    assert fresh and all(c >= eng.B for c in fresh)
    got = eng.tr.arrays()
    for c in fresh:
        assert got['steps'][c] == -1 and not got['path'][c].any() and (got['action'][c] == -1).all()
        assert not got['moves'][c].any() and not got['shielded'][c].any()
    seated = sorted(held | set(fresh))
    assert (got['steps'][[c for c in range(eng.C) if c not in seated]] == -1).all()
    assert (got['steps'][sorted(held)] == 2).all() and eng.tr.poison_intact()


def test_emu_stream_trace_guards_its_rows(emu):
    """A trace shorter than a case's limit (Python refuses it; the kernel guards its own memory): steps beyond T_cap write
    nothing, and nothing lands behind the arrays."""
    tab = sc.table('hand_n2_6x6')
    eng = TracedEngine(emu, tab)
    short = HostStreamTrace(eng.B, eng.C, eng.N, 2)
    assert emu.gnnpp_rollout_stream_trace_begin(ctypes.byref(eng.r), ctypes.byref(eng.s), ctypes.byref(short.s), None) == 0
    eng.tr = short
    sc.run_stream(eng, tab)
    got = short.arrays()
    assert got['steps'].max() == 2 and short.poison_intact()
    full = _run(emu, 'hand_n2_6x6')[2]
    assert np.array_equal(got['path'], full['path'][:, :3]) and np.array_equal(got['action'], full['action'][:, :2])
