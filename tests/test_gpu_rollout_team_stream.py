"""GPU (-m gpu): rollout.TeamRolloutStream with a policy in the loop.  A randomly initialised DecentralPlannerNet
(largeGraphFilter='lists', K = 3, eval) drives casegen cases of 129 agents through a 2-slot stream on the dense graph and on
the neighbour lists; the baseline is BatchedRollout.run over chunks of the same batch size and graph form, and every per-case
key must be identical.  Also: 'hashed' twice, the hand-over to expert.solve_failures, the refusals by name, one reseat
captured in a HIP graph, and one scripted reseat at N = 1024 on 64 x 64 (the full-width harvest fold and LDS request)."""
import numpy as np
import pytest
import torch

import rollout_team_stream_cases as tc

pytestmark = pytest.mark.gpu

N, W, SLOTS, CASES = 129, 24, 2, 6
PER_CASE = ('reached', 'success', 'makespan', 'flowtime', 'end_step', 'start_step', 'positions', 'radius', 'done')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


def _net(dev, n=N):
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from oracle import policy_oracle as orc

    class Cfg:
        num_agents, nGraphFilterTaps, device, largeGraphFilter = n, 3, dev, 'lists'
    net = DecentralPlannerNet(Cfg()).to(dev).eval()
    sd = orc.init_state_dict(3, seed=23)
    # a head whose arg-max differs from agent to agent, so that the teams move and collide
    sd['actionsMLP.0.weight'] = torch.randn(5, 128, generator=torch.Generator().manual_seed(5))
    sd['actionsMLP.0.bias'] = torch.zeros(5)
    net.load_state_dict(sd)
    return net


_shared = {}


def _cases(dev):
    if 'cases' not in _shared:
        from gnn_pathplanning_amd import casegen, mapf
        cases = casegen.generate(CASES, N, W, W, dev, density=0.1, seed=100 + N)
        assert bool(cases.ok.all())
        lower = mapf.distances(cases.grid, cases.start, cases.goal, dev).lower_makespan
        limits = torch.clamp(mapf.maxstep_from_distances(lower, 1.0), max=24)
        limits[1], limits[4] = 5, 9                          # mixed lengths: slots come free at different steps
        _shared['cases'] = (cases, limits, _net(dev))
    return _shared['cases']


def _both(dev, graph):
    """The stream's results and the chunked baseline's, computed once per graph form."""
    if graph not in _shared:
        from gnn_pathplanning_amd.rollout import BatchedRollout, TeamRolloutStream
        cases, maxstep, net = _cases(dev)
        with torch.no_grad():
            stream = TeamRolloutStream(cases.grid, cases.start, cases.goal, maxstep, dev, slots=SLOTS, graph=graph)
            got = stream.run(net)
            chunks = []
            for lo in range(0, CASES, SLOTS):
                # (a rollout moves its agents in the tensor it is given: a copy of the starts)
                env = BatchedRollout(cases.grid[lo:lo + SLOTS], cases.start[lo:lo + SLOTS].clone(), cases.goal[lo:lo + SLOTS],
                                     maxstep[lo:lo + SLOTS], dev, graph=graph)
                chunks.append(env.run(net))
        _shared[graph] = (stream, got, chunks)
    return _shared[graph]


@pytest.mark.parametrize('graph', tc.GRAPHS)
def test_team_stream_equals_chunked_rollouts(dev, graph):
    cases, maxstep, net = _cases(dev)
    stream, got, chunks = _both(dev, graph)
    assert (stream.env.S is None) == (graph == 'lists')
    assert got['done'].all() and (got['t0'][SLOTS:] > 0).all()
    for k in PER_CASE:
        want = torch.cat([c[k] for c in chunks], 0)
        assert got[k].dtype == want.dtype and torch.equal(got[k], want), (graph, k)
    lived = torch.minimum(torch.cat([c['end_step'] for c in chunks], 0).max(dim=1).values + 1, maxstep.cpu())
    assert torch.equal(got['lived'], lived.to(got['lived'].dtype))
    chunked = float(lived.sum()) / sum(SLOTS * c['steps'] for c in chunks)
    assert got['occupancy'] == pytest.approx(float(lived.sum()) / (SLOTS * got['steps']))
    print('%s: occupancy stream %.3f (%d steps), chunked %.3f (%d steps)'
          % (graph, got['occupancy'], got['steps'], chunked, sum(c['steps'] for c in chunks)))
    assert got['occupancy'] >= chunked
    moved = int((got['positions'] != cases.start.cpu()).any(-1).sum())
    assert moved > CASES * N // 10                            # (the planner does move the teams)


def test_team_stream_dense_equals_lists(dev):
    a, b = _both(dev, 'dense')[1], _both(dev, 'lists')[1]
    for k in PER_CASE + ('slot', 't0', 'lived'):
        assert torch.equal(a[k], b[k]), k


def test_solve_failures_takes_the_team_stream(dev):
    from gnn_pathplanning_amd import expert, mapf
    stream, got, _ = _both(dev, 'dense')
    failed = np.nonzero(~got['success'].numpy())[0]
    assert len(failed) > 0                                    # (a random planner under a limit of the lower bound)
    sol = expert.solve_failures(stream, results=got)
    assert (sol.episodes == failed).all()
    # planned from the FINAL positions of those cases, their goals and their maps: the same call made by hand
    idx = torch.as_tensor(failed, device=dev)
    assert torch.equal(stream.pos.cpu(), got['positions'])
    want = mapf.solve_team(stream.grid.index_select(0, idx), stream.pos.index_select(0, idx),
                           stream.goal.index_select(0, idx), dev)
    torch.cuda.synchronize(dev)
    assert torch.equal(sol.status, want.status) and torch.equal(sol.schedules, want.schedules)
    solved = (sol.status == 0).cpu()
    assert torch.equal(sol.schedules[:, 0].cpu()[solved], got['positions'][failed].to(sol.schedules.dtype)[solved])
    assert stream.pos.shape == (CASES, N, 2) and stream.goal.shape == (CASES, N, 2) and stream.B == CASES


def test_hashed_is_deterministic(dev):
    from gnn_pathplanning_amd.rollout import TeamRolloutStream
    cases, maxstep, net = _cases(dev)
    runs = []
    with torch.no_grad():
        for _ in range(2):
            runs.append(TeamRolloutStream(cases.grid, cases.start, cases.goal, maxstep, dev, slots=SLOTS, tie_mode='hashed',
                                          seed=7, reseat_every=4, graph='lists').run(net))
    for k in PER_CASE + ('slot', 't0', 'lived'):
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert runs[0]['occupancy'] == runs[1]['occupancy'] and runs[0]['done'].all()


def test_refused_modes_are_named(dev):
    from gnn_pathplanning_amd._native import GnnppError
    from gnn_pathplanning_amd.rollout import TeamRolloutStream
    grid = np.zeros((16, 16), np.uint8)
    many = np.stack([np.stack([np.arange(129) // 16, np.arange(129) % 16], 1)] * 3)
    for kw, word in (({'tie_mode': 'replay'}, 'replay'), ({'tie_mode': 'mt19937'}, 'mt19937'), ({'record': True}, 'record'),
                     ({'trace': True}, 'trace'), ({'graph': 'sparse'}, 'sparse')):
        with pytest.raises(GnnppError, match=word):
            TeamRolloutStream(grid, many, many, 5, dev, slots=2, **kw)
    with pytest.raises(GnnppError, match='N <= 128.*RolloutStream'):
        TeamRolloutStream(grid, many[:, :128], many[:, :128], 5, dev, slots=2)
    big = np.zeros((2, 1025, 2), np.int64)
    with pytest.raises(GnnppError, match='N > 1024'):
        TeamRolloutStream(np.zeros((40, 40), np.uint8), big, big, 5, dev, slots=2)
    with pytest.raises(GnnppError, match='65536 cells'):
        TeamRolloutStream(np.zeros((257, 256), np.uint8), many, many, 5, dev, slots=2)
    # graph='lists': the planner is checked before anything is enqueued
    st = TeamRolloutStream(grid, many, many, 5, dev, slots=2, graph='lists')

    class NoLists:
        training = False
    with pytest.raises(GnnppError, match='forward_logits_lists'):
        st.steps(NoLists(), 1)
    torch.cuda.synchronize(dev)
    assert st.t == 0 and int(st.cursor[0]) == 0 and bool((st.case == -1).all())


def _scripted(dev, graph, cases, limits, slots, n, seed):
    """Two identical streams after three scripted moves (reseat_every = 8: the first move seats, the others only move)."""
    from gnn_pathplanning_amd.rollout import TeamRolloutStream
    rng = np.random.default_rng(seed)
    acts = [torch.from_numpy(rng.integers(0, 5, size=(slots, n)).astype(np.int32)).to(dev) for _ in range(3)]
    streams = [TeamRolloutStream(cases[0], cases[1], cases[2], limits, dev, slots=slots, reseat_every=8, graph=graph)
               for _ in range(2)]
    for st in streams:
        if graph == 'lists':
            st.env.lists.zero_()                              # (what lies behind a list is nobody's: make it comparable)
        for a in acts:
            st.move(actions=a)
    torch.cuda.synchronize(dev)
    return streams, acts


ENV_STATE = ('grid', 'pos', 'goal', 'maxstep', 'obs', 'S', 'lists', 'radius', 'connected', 'reached', 'start_step', 'end_step',
             'flags', 'stats', 'done')
STREAM_STATE = ('cursor', 'case', 't0', 'assign', 'reached', 'start_step', 'end_step', 'pos', 'radius', 'stats', 'lived',
                'case_slot', 'case_t0')


@pytest.mark.parametrize('graph', tc.GRAPHS)
def test_reseat_in_a_hip_graph_equals_eager(dev, graph):
    """Two identical streams take the same scripted steps; one reseats eagerly, the other replays a captured reseat."""
    cases, _, _ = _cases(dev)
    limits = torch.tensor([1, 3, 2, 5, 2, 2], dtype=torch.int32)
    (eager, graphed), _ = _scripted(dev, graph, (cases.grid, cases.start, cases.goal), limits, SLOTS, N, 3)
    assert int((eager.env.done != 0).sum()) >= 1 and eager.t == 3
    eager.reseat()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    cuda_graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(cuda_graph, stream=side):
            graphed.reseat()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    assert int(graphed.cursor[0]) == SLOTS and int((graphed.lived >= 0).sum()) == 0      # captured, not yet run
    cuda_graph.replay()
    torch.cuda.synchronize(dev)
    assert int(eager.cursor[0]) > SLOTS and int((eager.assign >= 0).sum()) >= 1
    for name in STREAM_STATE:
        assert getattr(eager, name).cpu().numpy().tobytes() == getattr(graphed, name).cpu().numpy().tobytes(), name
    for name in ENV_STATE:
        a, b = getattr(eager.env, name), getattr(graphed.env, name)
        if a is None:
            assert b is None and name in ('S', 'lists')
            continue
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), name


@pytest.mark.parametrize('graph', tc.GRAPHS)
def test_one_reseat_at_1024_agents(dev, graph):
    """N = 1024 on 64 x 64, 2 slots, 3 cases, scripted: after three moves slot 0 (limit 1) is harvested and takes case 2.  The
    harvested row is the plain rollout of case 0 alone, the seated slot is case 2's own step 0, slot 1 keeps its bytes."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    from rollout_team_cases import make_instances
    n, w = 1024, 64
    grids, starts, goals = make_instances(np.random.default_rng(64), 3, n, w, w, 0.05)
    limits = torch.tensor([1, 9, 9], dtype=torch.int32)
    (st, _), acts = _scripted(dev, graph, (grids, starts, goals), limits, 2, n, 11)
    before = {k: getattr(st.env, k).clone() for k in ENV_STATE if getattr(st.env, k) is not None}
    st.reseat()
    torch.cuda.synchronize(dev)
    assert st.assign.tolist() == [2, -1] and st.case.tolist() == [2, 1] and st.t0.tolist() == [3, 0]
    assert int(st.cursor[0]) == 3
    # the harvest: case 0 alone, one move
    plain = BatchedRollout(grids[:1], starts[:1], goals[:1], 1, dev)
    plain.observe()
    plain.gso(0)
    plain.move(actions=acts[0][:1])
    want = plain.results()
    assert want['done'].all()
    assert torch.equal(st.reached[0].cpu(), want['reached'][0].to(torch.int32))
    assert torch.equal(st.start_step[0].cpu(), want['start_step'][0]) and torch.equal(st.end_step[0].cpu(), want['end_step'][0])
    assert torch.equal(st.pos[0].cpu(), want['positions'][0]) and float(st.radius[0]) == float(want['radius'][0])
    assert st.stats[0].tolist() == [int(want['makespan'][0]), int(want['flowtime'][0])]
    assert st.lived[:2].tolist() == [1, -1] and st.case_slot[0].item() == 0 and st.case_t0[0].item() == 0
    # the seat: case 2 alone at its step 0
    fresh = BatchedRollout(grids[2:], starts[2:], goals[2:], 9, dev, graph=graph)
    fresh.observe()
    fresh.gso(0)
    torch.cuda.synchronize(dev)
    e = st.env
    assert e.obs[0].cpu().numpy().tobytes() == fresh.obs[0].cpu().numpy().tobytes()
    assert float(e.radius[0]) == float(fresh.radius[0]) and int(e.connected[0]) == int(fresh.connected[0]) == 1
    if graph == 'dense':
        assert e.S[0].cpu().numpy().tobytes() == fresh.S[0].cpu().numpy().tobytes()
    else:
        assert tc.lists_slots(e.lists.cpu().numpy(), 2, n)[0].tobytes() == \
            tc.lists_slots(fresh.lists.cpu().numpy(), 1, n)[0].tobytes()
    assert torch.equal(e.pos[0].cpu(), torch.as_tensor(starts[2])) and torch.equal(e.goal[0].cpu(), torch.as_tensor(goals[2]))
    assert torch.equal(e.grid[0].cpu(), torch.as_tensor(grids[2])) and e.maxstep.tolist() == [12, 9]
    assert e.done.tolist() == [0, 0] and int(e.reached[0].sum()) == 0
    # slot 1 was live: untouched
    for k, v in before.items():
        if k == 'lists':
            assert tc.lists_slots(e.lists.cpu().numpy(), 2, n)[1].tobytes() == tc.lists_slots(v.cpu().numpy(), 2, n)[1].tobytes()
        else:
            assert getattr(e, k)[1].cpu().numpy().tobytes() == v[1].cpu().numpy().tobytes(), k
