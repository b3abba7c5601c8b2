"""GPU (-m gpu): rollout.RolloutStream(trace=...) with a policy in the loop.  A randomly initialised DecentralPlannerNet
(K = 3, eval) drives 24 casegen cases through a 4-slot traced stream on each of the rollout's three routes (the one-launch
burst at N = 10, move_and_observe at N = 20, move + gso_observe at N = 40).  The yardstick is what existed before:
BatchedRollout(record=True).run over chunks of 4 of the same cases.  Every comparison is exact equality of integers."""
import os

import numpy as np
import pytest
import torch

import rollout_stream_trace_cases as stc
from test_gpu_rollout_stream import CASES, PER_CASE, SLOTS, _cases, _net

pytestmark = pytest.mark.gpu

AUDIT_KEYS = ('status', 'arrival', 'makespan', 'flowtime', 'counts', 'first')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


def host(trace):
    torch.cuda.synchronize(trace.device)
    return {k: getattr(trace, k).cpu().numpy() for k in stc.KEYS}


_shared = {}


def _setup(N, W, dev):
    """Cases, limits, planner, and the chunked RECORDED baseline (rollouts, results, traces), computed once per team size."""
    if N not in _shared:
        from gnn_pathplanning_amd.rollout import BatchedRollout
        cases, maxstep = _cases(N, W, dev)
        net = _net(N, dev)
        envs, results = [], []
        with torch.no_grad():
            for lo in range(0, CASES, SLOTS):
                # (a rollout moves its agents in the tensor it is given when that is already an int32 device tensor: a copy)
                env = BatchedRollout(cases.grid[lo:lo + SLOTS], cases.start[lo:lo + SLOTS].clone(), cases.goal[lo:lo + SLOTS],
                                     maxstep[lo:lo + SLOTS], dev, record=True)
                results.append(env.run(net))
                envs.append(env)
        _shared[N] = (cases, maxstep, net, envs, results, [host(e.trace) for e in envs])
    return _shared[N]


_streams = {}


def _traced(N, W, dev, every=1):
    if (N, every) not in _streams:
        from gnn_pathplanning_amd.rollout import RolloutStream
        cases, maxstep, net = _setup(N, W, dev)[:3]
        with torch.no_grad():
            stream = RolloutStream(cases.grid, cases.start, cases.goal, maxstep, dev, slots=SLOTS, reseat_every=every,
                                   trace=True)
            got = stream.run(net)
        _streams[(N, every)] = (stream, got)
    return _streams[(N, every)]


@pytest.mark.parametrize('N,W,every', [(10, 20, 1), (10, 20, 4), (20, 20, 1), (40, 24, 1)])
def test_traced_stream_equals_chunked_recorded_rollouts(dev, N, W, every):
    """Per case: steps, moves, shielded, rows 0 .. steps of path, rows 0 .. steps - 1 of action.  every = 4 at N = 10 runs the
    traced burst with nsteps > 1."""
    cases, maxstep, net, envs, results, traces = _setup(N, W, dev)
    stream, got = _traced(N, W, dev, every)
    assert got['done'].all() and (got['t0'][SLOTS:] > 0).all()
    assert stream.trace.T_cap == int(maxstep.max()) and stream.trace.B == CASES
    tr = host(stream.trace)
    assert np.array_equal(tr['steps'], got['lived'].numpy()) and (tr['steps'] >= 1).all()
    for c in range(CASES):
        want, b = traces[c // SLOTS], c % SLOTS
        s = int(want['steps'][b])
        assert int(tr['steps'][c]) == s, (N, c)
        assert np.array_equal(tr['path'][c, :s + 1], want['path'][b, :s + 1]), (N, c)
        assert np.array_equal(tr['action'][c, :s], want['action'][b, :s]) and (tr['action'][c, :s] >= 0).all(), (N, c)
        assert np.array_equal(tr['moves'][c], want['moves'][b]) and np.array_equal(tr['shielded'][c], want['shielded'][b])
        assert not tr['path'][c, s + 1:].any() and (tr['action'][c, s:] == -1).all(), (N, c)
    assert tr['moves'].sum() > 0
    if N == 10:
        assert stream.env._logits is not None               # the one-launch step ran


@pytest.mark.parametrize('N,W', [(10, 20), (20, 20), (40, 24)])
def test_recording_changes_nothing(dev, N, W):
    """results() of the traced stream equal the untraced stream's in every per-case key, and the seating."""
    from gnn_pathplanning_amd.rollout import RolloutStream
    cases, maxstep, net = _setup(N, W, dev)[:3]
    _, got = _traced(N, W, dev)
    with torch.no_grad():
        plain = RolloutStream(cases.grid, cases.start, cases.goal, maxstep, dev, slots=SLOTS)
        assert plain.trace is None and plain.env._stream_trace is None
        want = plain.run(net)
    for k in PER_CASE + ('slot', 't0', 'lived'):
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (N, k)
    assert got['steps'] == want['steps'] and got['occupancy'] == want['occupancy']


@pytest.mark.parametrize('N,W', [(10, 20), (40, 24)])
def test_audit_agrees_with_the_chunks(dev, N, W):
    cases, maxstep, net, envs, results, traces = _setup(N, W, dev)
    stream, _ = _traced(N, W, dev)
    a = stream.trace.audit()
    torch.cuda.synchronize(dev)
    for i, env in enumerate(envs):
        b = env.trace.audit()
        torch.cuda.synchronize(dev)
        for k in AUDIT_KEYS:
            assert torch.equal(getattr(a, k)[i * SLOTS:(i + 1) * SLOTS], getattr(b, k)), (N, i, k)


def test_prediction_files_equal_the_chunks(dev, tmp_path):
    """write_prediction_cases on the stream writes, per case, the two files it writes for the chunked recorded rollouts, and
    expert.read_solution reads a pair back to trace.schedule(c) -- up to the makespan the file states, from which the
    reference's loader takes its length (as tests/test_gpu_rollout_trace.py explains); the rows behind it are in the file
    and compared through the chunk's file."""
    from gnn_pathplanning_amd import expert
    cases, maxstep, net, envs, results, traces = _setup(10, 20, dev)
    stream, got = _traced(10, 20, dev)
    mine = expert.write_prediction_cases(str(tmp_path / 'stream'), stream, results=got)
    assert [w[0] for w in mine] == list(range(CASES))
    full = 0
    for i, env in enumerate(envs):
        theirs = expert.write_prediction_cases(str(tmp_path / 'chunks'), env, ids=range(i * SLOTS, (i + 1) * SLOTS),
                                               results=results[i])
        for (b, inp_b, pred_b) in theirs:
            c, inp, pred = mine[i * SLOTS + b]
            assert c == i * SLOTS + b
            assert os.path.relpath(inp, str(tmp_path / 'stream')) == os.path.relpath(inp_b, str(tmp_path / 'chunks'))
            assert os.path.relpath(pred, str(tmp_path / 'stream')) == os.path.relpath(pred_b, str(tmp_path / 'chunks'))
            assert open(inp).read() == open(inp_b).read() and open(pred).read() == open(pred_b).read(), c
            assert open(pred).read() == stream.trace.prediction_yaml(c)
            sched = stream.trace.schedule(c)
            assert sched.dtype == np.int64 and np.array_equal(sched, env.trace.schedule(b))
            grid, goal, read = expert.read_solution(inp, pred)
            assert np.array_equal(grid, cases.grid[c].cpu().numpy()) and np.array_equal(goal, cases.goal[c].cpu().numpy())
            rows = int(got['makespan'][c]) + 1
            assert read.shape[0] == rows <= sched.shape[0] and np.array_equal(read, sched[:rows])
            full += int(rows == sched.shape[0])
    assert full >= 1                                          # a case whose files read back to ALL of trace.schedule(c)


def test_hashed_twice_gives_the_same_bytes(dev):
    from gnn_pathplanning_amd.rollout import RolloutStream
    cases, maxstep, net = _setup(10, 20, dev)[:3]
    runs = []
    with torch.no_grad():
        for _ in range(2):
            st = RolloutStream(cases.grid, cases.start, cases.goal, maxstep, dev, slots=SLOTS, tie_mode='hashed', seed=7,
                               reseat_every=4, trace=True)
            res = st.run(net)
            assert res['done'].all()
            tr = host(st.trace)
            tr['seen_done'] = st.trace.seen_done.cpu().numpy()
            runs.append(tr)
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    assert (runs[0]['steps'] >= 1).all()


def test_refusals_are_named(dev):
    from gnn_pathplanning_amd._native import GnnppError
    from gnn_pathplanning_amd.rollout import RolloutStream
    grid = np.zeros((16, 16), np.uint8)
    starts = np.stack([np.stack([np.arange(4), np.zeros(4, int)], 1)] * 3)
    goals = starts[:, ::-1].copy()
    with pytest.raises(GnnppError, match=r'trace=4 is below .*max\(maxstep\) = 7'):
        RolloutStream(grid, starts, goals, [5, 7, 3], dev, slots=2, trace=4)
    with pytest.raises(GnnppError, match='record'):
        RolloutStream(grid, starts, goals, 5, dev, slots=2, record=True)
    with pytest.raises(GnnppError, match='record'):
        RolloutStream(grid, starts, goals, 5, dev, slots=2, record=True, trace=True)
    assert RolloutStream(grid, starts, goals, [5, 7, 3], dev, slots=2, trace=9).trace.T_cap == 9
    assert RolloutStream(grid, starts, goals, [5, 7, 3], dev, slots=2, trace=True).trace.T_cap == 7
    assert RolloutStream(grid, starts, goals, [5, 7, 3], dev, slots=2).trace is None


def test_reseat_move_record_in_a_hip_graph_equals_eager(dev):
    """Two identical traced streams take the same scripted steps; then one reseats, moves and records eagerly, the other
    replays ONE captured graph of the same three calls (tests/test_gpu_rollout_stream.py::test_reseat_in_a_hip_graph_equals_
    eager, with the move and its record behind the reseat)."""
    from gnn_pathplanning_amd.rollout import RolloutStream
    cases = _setup(10, 20, dev)[0]
    limits = torch.tensor([1, 3, 2, 5] * (CASES // 4), dtype=torch.int32)
    rng = np.random.default_rng(3)
    acts = [torch.from_numpy(rng.integers(0, 5, size=(SLOTS, 10)).astype(np.int32)).to(dev) for _ in range(4)]
    streams = [RolloutStream(cases.grid, cases.start, cases.goal, limits, dev, slots=SLOTS, reseat_every=8, trace=True)
               for _ in range(2)]
    for st in streams:
        for a in acts[:3]:                                   # (reseat_every = 8: the first move seats, the others only move)
            st.move(actions=a)
        torch.cuda.synchronize(dev)
        assert int((st.env.done != 0).sum()) >= 2 and st.t == 3
    eager, graphed = streams
    eager.reseat()
    eager.move(actions=acts[3])
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            graphed.reseat()
            graphed.move(actions=acts[3])
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    assert int(graphed.cursor[0]) == SLOTS and int(graphed.trace.steps.max()) == 3            # captured, not yet run
    graph.replay()
    torch.cuda.synchronize(dev)
    assert eager.t == graphed.t == 4 and int(eager.cursor[0]) > SLOTS
    fresh = eager.case[eager.t0 == 3].cpu().tolist()
    assert len(fresh) >= 2 and (eager.trace.steps[fresh] == 1).all()      # seated in the graph, recorded at their row 1
    for name in ('path', 'action', 'moves', 'shielded', 'steps', 'seen_done'):
        assert getattr(eager.trace, name).cpu().numpy().tobytes() == getattr(graphed.trace, name).cpu().numpy().tobytes(), name
    for name in ('cursor', 'case', 't0', 'assign', 'reached', 'start_step', 'end_step', 'pos', 'radius', 'stats', 'lived',
                 'case_slot', 'case_t0'):
        assert getattr(eager, name).cpu().numpy().tobytes() == getattr(graphed, name).cpu().numpy().tobytes(), name
    for name in ('pos', 'goal', 'maxstep', 'obs', 'S', 'radius', 'reached', 'start_step', 'end_step', 'flags', 'stats', 'done'):
        assert getattr(eager.env, name).cpu().numpy().tobytes() == getattr(graphed.env, name).cpu().numpy().tobytes(), name
