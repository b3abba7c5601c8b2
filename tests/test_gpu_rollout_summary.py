"""GPU (-m gpu): gnnpp_rollout_summary and metrics.summarise on the MI355X.  The shared table of shapes against the float64
numpy restatement (integers and histogram exactly, doubles within the measured bound) and the reference's fixture;
summarise() on a scripted BatchedRollout (3 cases x 2 agents, traced and audited, targets from mapf.distances), on a
RolloutStream (5 cases x 2 agents in 2 slots, one case unfinished, traced) and on a TeamRolloutStream (3 cases x 129 agents in
2 slots, targets from a Solutions with one unsolved case), each against the same numbers computed from results() on the
host; one call captured in a HIP graph and replayed twice; two calls give equal tensors; merge of two device summaries."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rollout_summary_cases as rc                                                  # noqa: E402

pytestmark = pytest.mark.gpu

STAY, LEFT, RIGHT = 4, 1, 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'metrics_summary.npz')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


class DeviceCall:
    """One entry's tables on the device and a poisoned record with 16 guard bytes behind it; launch() enqueues the call."""

    def __init__(self, x, dev, poison=0x5a):
        from gnn_pathplanning_amd import _native
        self.x, self.dev, self.poison = x, dev, poison
        self.lib = _native.lib()
        self.nbytes = self.lib.gnnpp_rollout_summary_out_bytes(x['N'], x['G'])
        assert self.nbytes == x['G'] * 192 + x['G'] * (x['N'] + 1) * 4
        self.keep = {}

        def ptr(a):
            t = self.keep.setdefault(id(a), torch.from_numpy(np.ascontiguousarray(a)).to(dev))
            return t.data_ptr()
        self.s = rc.fill_struct(_native.RolloutSummaryIn(), x, ptr)
        self.out = torch.full((self.nbytes + 16,), poison, dtype=torch.uint8, device=dev)
        assert self.out.data_ptr() % 8 == 0

    def launch(self):
        from gnn_pathplanning_amd import _native
        rcode = self.lib.gnnpp_rollout_summary(ctypes.byref(self.s), self.out.data_ptr(), _native.stream_ptr(self.dev))
        assert rcode == 0, rcode

    def read(self):
        torch.cuda.synchronize(self.dev)
        buf = self.out.cpu().numpy()
        assert (buf[self.nbytes:] == self.poison).all(), 'a write behind the record'
        return tuple(v.copy() for v in rc.out_views(buf[:self.nbytes], self.x['N'], self.x['G']))


def run_device(x, dev, poison=0x5a):
    call = DeviceCall(x, dev, poison)
    call.launch()
    return call.read()


@pytest.mark.parametrize('C,N,G', rc.SHAPES)
def test_gpu_summary_table(dev, C, N, G):
    worst = 0.0
    for with_valid, degenerate in rc.VARIANTS:
        x = rc.inputs(C, N, G, with_valid, degenerate)
        worst = max(worst, rc.check(run_device(x, dev), rc.restate(x), (C, N, G, with_valid, degenerate)))
    print('largest relative difference from numpy float64 at C=%d N=%d G=%d: %.3g' % (C, N, G, worst))


@pytest.mark.parametrize('C,N,G', rc.HIST_SHAPES)
def test_gpu_summary_histogram_paths(dev, C, N, G):
    for with_valid in (True, False):
        x = rc.inputs(C, N, G, with_valid, 'one')
        rc.check(run_device(x, dev), rc.restate(x), (C, N, G, with_valid))


def golden_entry():
    z = np.load(GOLDEN)
    return z, {'C': int(z['reached'].shape[0]), 'N': int(z['reached'].shape[1]), 'G': 1, 'reached': z['reached'],
               'stats': z['stats'], 'targets': z['targets'], 'target_stride': 2, 'valid': None, 'group': None,
               'shielded': z['shielded'], 'audit_ok': z['audit_ok']}


def test_gpu_summary_meets_the_reference_fixture(dev):
    from gnn_pathplanning_amd.metrics import Summary
    z, x = golden_entry()
    got = run_device(x, dev)
    rc.check(got, rc.restate(x), 'fixture')
    res = Summary(*got).host()
    for k in ('rateReachGoal', 'avg_rate_deltaMP', 'std_rate_deltaMP', 'avg_rate_deltaFT', 'std_rate_deltaFT',
              'rateFailedReachGoalSH', 'ratefindOptimalSolution', 'rateCollsionFreeSol', 'rateCollisionPredictedinLoop'):
        assert rc.rel_diff([res[k]], [float(z[k])]) <= rc.TOL, (k, res[k], float(z[k]))
    assert res['list_numAgentReachGoal'] == z['hist_numAgentReachGoal'].tolist()


def test_gpu_summary_is_deterministic_and_capturable(dev):
    """Two calls give torch.equal records; a captured call replayed twice gives the same bytes as the eager one."""
    x = rc.inputs(600, 3, 3, True, 'one')
    a, b = DeviceCall(x, dev), DeviceCall(x, dev, poison=0xa5)
    a.launch()
    b.launch()
    torch.cuda.synchronize(dev)
    assert torch.equal(a.out[:a.nbytes], b.out[:b.nbytes])
    g = DeviceCall(x, dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            g.launch()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    assert bool((g.out == 0x5a).all())                       # captured, not yet run
    for _ in range(2):
        g.out.fill_(0x33)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(g.out[:g.nbytes], a.out[:a.nbytes]) and bool((g.out[g.nbytes:] == 0x33).all())


def entry_from_results(res, targets, N, shielded=None, audit_ok=None, valid=None):
    """The kernel's inputs as the HOST sees them in results(): the restatement of these is what summarise() must give."""
    done = res['done'].numpy()
    if valid is not None:
        done = done & valid
    C = len(done)
    return {'C': C, 'N': N, 'G': 1, 'reached': res['reached'].numpy().astype(np.int32),
            'stats': np.stack([res['makespan'].numpy(), res['flowtime'].numpy()], 1).astype(np.int32),
            'targets': np.ascontiguousarray(targets, np.int32), 'target_stride': 2, 'valid': done.astype(np.int32),
            'group': None, 'shielded': shielded, 'audit_ok': audit_ok}


def test_summarise_a_scripted_batched_rollout(dev):
    """3 cases x 2 agents on an empty 6 x 6 map, 4 scripted steps, recorded.  Case 0: both agents start on their goals (the
    expert's costs are 0: degenerate).  Case 1: agent 0 walks three cells to its goal.  Case 2: agent 0 asks to walk off the
    map at every step, is shielded every time and never arrives."""
    from gnn_pathplanning_amd import mapf, metrics
    from gnn_pathplanning_amd.rollout import BatchedRollout
    grid = np.zeros((6, 6), np.uint8)
    starts = np.array([[[1, 1], [4, 4]], [[2, 0], [4, 4]], [[0, 0], [4, 4]]], np.int32)
    goals = np.array([[[1, 1], [4, 4]], [[2, 3], [4, 4]], [[0, 2], [4, 4]]], np.int32)
    script = torch.tensor([[STAY, STAY], [RIGHT, STAY], [LEFT, STAY]], dtype=torch.int32, device=dev)
    arrived = script.clone()
    arrived[1, 0] = STAY                                      # (asking to move on the goal would count as shielded)
    env = BatchedRollout(grid, starts, goals, 4, dev, record=True)
    for step in range(4):
        env.move(actions=script if step < 3 else arrived)
    dist = mapf.distances(grid, starts, goals, dev)
    audit = env.trace.audit()
    s = metrics.summarise(env, dist, audit=audit)
    again = metrics.summarise(env, dist, audit=(audit.status == 0).to(torch.int32))
    res = env.results()
    assert res['success'].tolist() == [True, True, False]
    targets = np.stack([dist.lower_makespan.cpu().numpy(), dist.lower_flowtime.cpu().numpy()], 1)
    assert targets.tolist() == [[0, 0], [3, 3], [2, 2]]
    x = entry_from_results(res, targets, 2, shielded=env.trace.shielded.cpu().numpy(),
                           audit_ok=(audit.status == 0).cpu().numpy().astype(np.int32))
    x['valid'] = None                                         # a fixed batch: every episode counts
    rc.check(s._read(), rc.restate(x), 'batched')
    assert torch.equal(s.i64, again.i64) and torch.equal(s.hist, again.hist)
    assert s.f64.cpu().numpy().tobytes() == again.f64.cpu().numpy().tobytes()
    h = s.host()
    assert h['n'] == 3 and h['n_reach_all'] == 2 and h['n_degenerate'] == 1 and h['n_fail_shielded'] == 1
    assert h['list_numAgentReachGoal'] == [0, 1, 2] and h['rateReachGoal'] == 2 / 3
    assert h['rateCollisionPredictedinLoop'] == 1 / 3 and h['rateFailedReachGoalSH'] == 1 / 3


def _drive(stream, script, unfinished):
    """Scripted moves (case c asks for script[c] at every step) until all but `unfinished` cases have ended."""
    C = stream.C
    table = torch.cat([script, torch.full((1,) + tuple(script.shape[1:]), STAY, dtype=torch.int32, device=script.device)])
    for _ in range(40):
        stream.reseat()
        stream.move(actions=table[stream.case.long()])       # (an empty slot holds case -1: the last row, STAY)
        res = stream.results()
        if int(res['done'].sum()) >= C - unfinished:
            return res
    raise AssertionError('the scripted stream did not get there')


def test_summarise_a_stream_with_one_case_unfinished(dev):
    """5 cases x 2 agents through 2 slots, traced.  Cases 0 and 2 start on their goals, cases 1 and 4 walk into the map's
    edge until their limits (3 and 9 steps), case 3 walks three cells to its goal; the last one still runs when the
    summary is taken."""
    from gnn_pathplanning_amd import metrics
    from gnn_pathplanning_amd.rollout import RolloutStream
    grid = np.zeros((6, 6), np.uint8)
    on, wall, walk = [[1, 1], [4, 4]], [[0, 0], [4, 4]], [[2, 0], [4, 4]]
    starts = np.array([on, wall, on, walk, wall], np.int32)
    goals = np.array([on, [[0, 2], [4, 4]], on, [[2, 3], [4, 4]], [[0, 2], [4, 4]]], np.int32)
    script = torch.tensor([[STAY, STAY], [LEFT, STAY], [STAY, STAY], [RIGHT, STAY], [LEFT, STAY]], dtype=torch.int32,
                          device=dev)
    stream = RolloutStream(grid, starts, goals, [9, 3, 9, 9, 9], dev, slots=2, trace=True)
    _drive(stream, script, unfinished=1)
    targets = torch.tensor([[1, 1], [2, 2], [0, 0], [3, 3], [2, 2]], dtype=torch.int32, device=dev)
    group = torch.tensor([0, 1, 0, 1, 1], dtype=torch.int32, device=dev)
    s = metrics.summarise(stream, targets)
    by_group = metrics.summarise(stream, targets, group=group, groups=2)
    res = stream.results()
    assert int(res['done'].sum()) == 4 and not bool(res['done'][4])
    x = entry_from_results(res, targets.cpu().numpy(), 2, shielded=stream.trace.shielded.cpu().numpy())
    rc.check(s._read(), rc.restate(x), 'stream')
    rc.check(by_group._read(), rc.restate(dict(x, G=2, group=group.cpu().numpy())), 'stream, two groups')
    h = s.host()
    assert h['n'] == 4 and h['n_reach_all'] == 3 and h['n_degenerate'] == 1 and h['n_fail_shielded'] == 1
    assert by_group.per_group(0)['n'] == 2 and by_group.per_group(1)['n'] == 2 and by_group.host()['n'] == 4
    # merge of two device summaries: the two groups, summarised one by one, against the summary of all
    parts = [metrics.summarise(stream, targets, group=(group != g).to(torch.int32), groups=1) for g in (0, 1)]
    for g, p in enumerate(parts):                             # (group ids 1 fall outside the one group: n_bad_group)
        assert p.host()['n'] == 2 and p.host()['n_bad_group'] == 2
    merged = metrics.Summary.merge(parts)
    want = [a.copy() for a in s._read()]
    want[0][0, rc.I_BAD_GROUP] = 4
    rc.check(merged._read(), tuple(want), 'merge of two device summaries')


def test_summarise_a_team_stream(dev):
    """3 cases x 129 agents on an empty 16 x 16 map through 2 slots.  In cases 0 and 2 every agent starts on its goal; in
    case 1 agent 0's goal is elsewhere and it never moves (limit 3).  The targets are a Solutions whose case 2 is
    unsolved: it takes no part."""
    from gnn_pathplanning_amd import mapf, metrics
    from gnn_pathplanning_amd.rollout import TeamRolloutStream
    N = 129
    grid = np.zeros((16, 16), np.uint8)
    cells = np.stack([np.arange(N) // 16, np.arange(N) % 16], 1).astype(np.int32)
    starts = np.stack([cells] * 3)
    goals = starts.copy()
    goals[1, 0] = [15, 15]
    script = torch.full((3, N), STAY, dtype=torch.int32, device=dev)
    stream = TeamRolloutStream(grid, starts, goals, 3, dev, slots=2)
    _drive(stream, script, unfinished=0)
    i32 = dict(dtype=torch.int32, device=dev)
    sol = mapf.Solutions(status=torch.tensor([0, 0, mapf.NO_PATH], **i32), makespan=torch.tensor([1, 2, -1], **i32),
                         flowtime=torch.tensor([N, 2 * N, -1], **i32), arrival=torch.zeros(3, N, **i32))
    s = metrics.summarise(stream, sol)
    res = stream.results()
    assert res['done'].all() and res['success'].tolist() == [True, False, True]
    x = entry_from_results(res, [[1, N], [2, 2 * N], [-1, -1]], N, valid=np.array([True, True, False]))
    rc.check(s._read(), rc.restate(x), 'team stream')
    h = s.host()
    assert h['n'] == 2 and h['n_reach_all'] == 1 and h['min_reached'] == N - 1 and h['max_reached'] == N
    assert h['list_numAgentReachGoal'][N - 1:] == [1, 1] and sum(h['list_numAgentReachGoal']) == 2
    assert np.isnan(h['rateFailedReachGoalSH']) and np.isnan(h['rateCollsionFreeSol'])     # no trace, no audit
