"""GPU (-m gpu): the shared case table of streamed rollouts (tests/rollout_stream_cases.py) through
rollout.RolloutStream(trace=True).move() on the device, with the assertions of the emulated run
(tests/test_emu_rollout_stream_trace.py): every case's steps, moves, shielded, rows 0 .. steps of path and rows
0 .. steps - 1 of action equal, exactly, the trace of the plain per-case rollout of the same scripts
(BatchedRollout(record=True) with B = C), the rows beyond are 0 / -1, the hand-derived values hold, and the per-case
result tables are what the untraced stream's tests pin."""
import numpy as np
import pytest
import torch

import rollout_stream_cases as sc
import rollout_stream_trace_cases as stc
from test_gpu_rollout_stream_cases import GpuEngine, plain_rollout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


def host(trace):
    torch.cuda.synchronize(trace.device)
    return {k: getattr(trace, k).cpu().numpy() for k in stc.KEYS + ('seen_done',)}


def plain_trace(tab, dev):
    from gnn_pathplanning_amd.rollout import BatchedRollout
    env = BatchedRollout(tab['grids'], tab['starts'], tab['goals'], tab['maxstep'], dev, commR=sc.COMM_R, record=True)
    assert env.trace.T_cap == stc.t_cap(tab)
    for t in range(stc.t_cap(tab)):
        env.move(actions=torch.from_numpy(sc.plain_actions(tab, t)).to(dev))
    assert env.results()['done'].all()
    return host(env.trace)


class TracedGpuEngine(GpuEngine):
    def __init__(self, tab, dev):
        from gnn_pathplanning_amd.rollout import RolloutStream, StreamTrace
        self.st = RolloutStream(tab['grids'], tab['starts'], tab['goals'], tab['maxstep'], dev, slots=tab['slots'],
                                commR=sc.COMM_R, reseat_every=tab['reseat_every'], trace=True)
        self.B, self.C, self.N = self.st.slots, self.st.C, self.st.N
        self.dev = dev
        tr = self.st.trace
        assert isinstance(tr, StreamTrace) and (tr.B, tr.N, tr.T_cap) == (self.C, self.N, stc.t_cap(tab))
        assert tr.grid is self.st.grid and tr.goal is self.st.goal and tr.grid_batched == int(sc.batched(tab))
        got = host(tr)                                        # begin: everything set
        assert not got['path'].any() and (got['action'] == -1).all() and (got['steps'] == -1).all()
        assert not got['moves'].any() and not got['shielded'].any() and not got['seen_done'].any()


@pytest.mark.parametrize('name', sc.TABLE_NAMES)
def test_gpu_stream_trace_table(dev, name):
    tab = sc.table(name)
    want = plain_trace(tab, dev)
    eng = TracedGpuEngine(tab, dev)
    tables, seats = sc.run_stream(eng, tab)
    got = host(eng.st.trace)
    stc.assert_case_traces(tab, got, want, lived=tables['lived'])
    # recording changes nothing: the per-case result tables and the seating are the untraced stream's
    plain, _ = plain_rollout(tab, dev)
    sc.assert_tables(tab, tables, sc.plain_expectation(plain))
    sc.assert_seats(tab, seats, tables)
    for c in (0, eng.C - 1):
        assert np.array_equal(eng.st.trace.schedule(c), got['path'][c, :int(got['steps'][c]) + 1].astype(np.int64))


def test_gpu_stream_trace_two_runs_give_the_same_bytes(dev):
    tab = sc.table('n4_6x6_every4')
    runs = []
    for _ in range(2):
        eng = TracedGpuEngine(tab, dev)
        sc.run_stream(eng, tab)
        runs.append(host(eng.st.trace))
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k


def test_gpu_stream_trace_seated_but_never_moved(dev):
    """results() in the middle of a stream seats cases that then never get a move: they read steps = -1, their rows are
    what begin left, and audit() refuses by name while such a case exists."""
    from gnn_pathplanning_amd._native import GnnppError
    tab = sc.table('n4_6x6_every4')
    eng = TracedGpuEngine(tab, dev)
    st = eng.st
    st.reseat()
    for now in range(2):                                     # (reseat_every = 4: these moves do not reseat)
        st.move(actions=torch.from_numpy(sc.script_actions(tab, st.case.cpu().numpy(), st.t0.cpu().numpy(), now)).to(dev))
    held = set(st.case.cpu().tolist())
    st.results()
    fresh = sorted(set(st.case.cpu().tolist()) - held)
    assert fresh and all(c >= eng.B for c in fresh)
    got = host(st.trace)
    for c in fresh:
        assert got['steps'][c] == -1 and not got['path'][c].any() and (got['action'][c] == -1).all()
    assert (got['steps'][sorted(held)] == 2).all()
    with pytest.raises(GnnppError, match='no recorded move'):
        st.trace.audit()
