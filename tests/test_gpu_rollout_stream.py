"""GPU (-m gpu): rollout.RolloutStream with a policy in the loop.  A randomly initialised DecentralPlannerNet (K = 3, eval)
drives casegen cases through a 4-slot stream on each of the rollout's three routes (the one-launch step at N = 10,
move_and_observe at N = 20, move + gso_observe at N = 40); the baseline is BatchedRollout.run over chunks of the same batch
size, so both run the same kernel variant, and every per-case key must be identical.  Also: occupancy, the hand-over to
expert.solve_failures, 'hashed' twice, the refused modes by name, and one reseat captured in a HIP graph."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SLOTS, CASES = 4, 24
PER_CASE = ('reached', 'success', 'makespan', 'flowtime', 'end_step', 'start_step', 'positions', 'radius', 'done')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


def _net(N, dev):
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from oracle import policy_oracle as orc

    class Cfg:
        num_agents, nGraphFilterTaps, device = N, 3, dev
    net = DecentralPlannerNet(Cfg()).to(dev).eval()
    net.load_state_dict(orc.init_state_dict(3, seed=N))
    return net


def _cases(N, W, dev, C=CASES, rate=2.0):
    from gnn_pathplanning_amd import casegen, mapf
    cases = casegen.generate(C, N, W, W, dev, density=0.1, seed=100 + N)
    assert bool(cases.ok.all())
    lower = mapf.distances(cases.grid, cases.start, cases.goal, dev).lower_makespan
    return cases, mapf.maxstep_from_distances(lower, rate)


_shared = {}


def _both(N, W, dev):
    """The stream's results and the chunked baseline's, computed once per team size."""
    if N not in _shared:
        from gnn_pathplanning_amd.rollout import BatchedRollout, RolloutStream
        cases, maxstep = _cases(N, W, dev)
        net = _net(N, dev)
        with torch.no_grad():
            stream = RolloutStream(cases.grid, cases.start, cases.goal, maxstep, dev, slots=SLOTS)
            got = stream.run(net)
            chunks = []
            for lo in range(0, CASES, SLOTS):
                env = BatchedRollout(cases.grid[lo:lo + SLOTS], cases.start[lo:lo + SLOTS], cases.goal[lo:lo + SLOTS],
                                     maxstep[lo:lo + SLOTS], dev)
                chunks.append(env.run(net))
        _shared[N] = (cases, maxstep, net, stream, got, chunks)
    return _shared[N]


@pytest.mark.parametrize('N,W', [(10, 20), (20, 20), (40, 24)])
def test_stream_equals_chunked_rollouts(dev, N, W):
    cases, maxstep, net, stream, got, chunks = _both(N, W, dev)
    assert got['done'].all() and (got['t0'][SLOTS:] > 0).all()
    for k in PER_CASE:
        want = torch.cat([c[k] for c in chunks], 0)
        assert got[k].dtype == want.dtype and torch.equal(got[k], want), (N, k)
    # occupancy: live slot-steps over all slot-steps; the chunked figure from the chunks' own results -- an episode lives
    # until the call after its last arrival, or its limit
    lived = torch.minimum(torch.cat([c['end_step'] for c in chunks], 0).max(dim=1).values + 1, maxstep.cpu())
    assert torch.equal(got['lived'], lived.to(got['lived'].dtype))
    chunked = float(lived.sum()) / sum(SLOTS * c['steps'] for c in chunks)
    assert got['occupancy'] == pytest.approx(float(lived.sum()) / (SLOTS * got['steps']))
    print('N = %d: occupancy stream %.3f (%d steps), chunked %.3f (%d steps)'
          % (N, got['occupancy'], got['steps'], chunked, sum(c['steps'] for c in chunks)))
    assert got['occupancy'] >= chunked


def test_solve_failures_takes_the_stream(dev):
    from gnn_pathplanning_amd import expert
    cases, maxstep, net, stream, got, chunks = _both(10, 20, dev)
    failed = np.nonzero(~got['success'].numpy())[0]
    sol = expert.solve_failures(stream, results=got)
    if len(failed) == 0:
        assert sol is None
        return
    assert (sol.episodes == failed).all()
    torch.cuda.synchronize(dev)
    # planned from the FINAL positions of those cases: row 0 of every schedule
    assert torch.equal(sol.schedules[:, 0].cpu(), got['positions'][failed].to(sol.schedules.dtype))
    assert stream.pos.shape == (CASES, 10, 2) and stream.goal.shape == (CASES, 10, 2) and stream.B == CASES


def test_hashed_is_deterministic(dev):
    from gnn_pathplanning_amd.rollout import RolloutStream
    cases, maxstep, net, _, _, _ = _both(10, 20, dev)
    runs = []
    with torch.no_grad():
        for _ in range(2):
            runs.append(RolloutStream(cases.grid, cases.start, cases.goal, maxstep, dev, slots=SLOTS, tie_mode='hashed',
                                      seed=7, reseat_every=4).run(net))
    for k in PER_CASE + ('slot', 't0', 'lived'):
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert runs[0]['occupancy'] == runs[1]['occupancy'] and runs[0]['done'].all()


def test_refused_modes_are_named(dev):
    from gnn_pathplanning_amd._native import GnnppError
    from gnn_pathplanning_amd.rollout import RolloutStream
    grid = np.zeros((16, 16), np.uint8)
    starts = np.stack([np.stack([np.arange(4), np.zeros(4, int)], 1)] * 3)
    goals = starts[:, ::-1].copy()
    for kw, word in (({'tie_mode': 'replay'}, 'replay'), ({'tie_mode': 'mt19937'}, 'mt19937'), ({'record': True}, 'record'),
                     ({'graph': 'lists'}, 'lists')):
        with pytest.raises(GnnppError, match=word):
            RolloutStream(grid, starts, goals, 5, dev, slots=2, **kw)
    many = np.stack([np.stack([np.arange(129) // 16, np.arange(129) % 16], 1)] * 2)
    with pytest.raises(GnnppError, match='N > 128'):
        RolloutStream(grid, many, many, 5, dev, slots=2)


def test_reseat_in_a_hip_graph_equals_eager(dev):
    """Two identical streams take the same scripted steps; one reseats eagerly, the other replays a captured reseat."""
    from gnn_pathplanning_amd.rollout import RolloutStream
    cases, _, _, _, _, _ = _both(10, 20, dev)
    limits = torch.tensor([1, 3, 2, 5] * (CASES // 4), dtype=torch.int32)
    rng = np.random.default_rng(3)
    acts = [torch.from_numpy(rng.integers(0, 5, size=(SLOTS, 10)).astype(np.int32)).to(dev) for _ in range(3)]
    streams = [RolloutStream(cases.grid, cases.start, cases.goal, limits, dev, slots=SLOTS, reseat_every=8)
               for _ in range(2)]
    for st in streams:
        for a in acts:                                       # (reseat_every = 8: the first move seats, the others only move)
            st.move(actions=a)
        torch.cuda.synchronize(dev)
        assert int((st.env.done != 0).sum()) >= 2 and st.t == 3
    eager, graphed = streams
    eager.reseat()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            graphed.reseat()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    assert int(graphed.cursor[0]) == SLOTS and int((graphed.lived >= 0).sum()) == 0      # captured, not yet run
    graph.replay()
    torch.cuda.synchronize(dev)
    assert int(eager.cursor[0]) > SLOTS and int((eager.assign >= 0).sum()) >= 2
    for name in ('cursor', 'case', 't0', 'assign', 'reached', 'start_step', 'end_step', 'pos', 'radius', 'stats', 'lived',
                 'case_slot', 'case_t0'):
        assert getattr(eager, name).cpu().numpy().tobytes() == getattr(graphed, name).cpu().numpy().tobytes(), name
    for name in ('grid', 'pos', 'goal', 'maxstep', 'obs', 'S', 'radius', 'connected', 'reached', 'start_step', 'end_step',
                 'flags', 'stats', 'done'):
        assert getattr(eager.env, name).cpu().numpy().tobytes() == getattr(graphed.env, name).cpu().numpy().tobytes(), name
