"""MI355X: gnnpp_mapf_solve through gnn_pathplanning_amd/mapf.py against the sequential numpy restatement of the
contract (tests/mapf_cases.py): equality of every output of every case, solved or not; every solved schedule replayed
through the device simulator (BatchedRollout.move, tie_mode 'lowest'); identical bytes across calls, a side stream and a
captured graph; and the whole loop rollout -> solve_failures -> samples_from_solutions -> SamplePool -> train_step."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mapf_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OUTS = ('schedules', 'arrival', 'makespan', 'flowtime', 'status', 'failing', 'restart')


@pytest.fixture(scope='module')
def mapf():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from gnn_pathplanning_amd import _native, mapf as m
    _native.lib()
    return m


def assert_equal_to_yardstick(sol, cases, T, orders=None):
    host = {k: getattr(sol, k).cpu().numpy() for k in OUTS}
    for c, (g, s, gl) in enumerate(cases):
        want = mc.solve_case(g, s, gl, T, None if orders is None else list(orders[c]))
        for k in ('status', 'restart', 'makespan', 'flowtime', 'failing'):
            assert int(host[k][c]) == want[k], (c, k, int(host[k][c]), want[k])
        assert np.array_equal(host['arrival'][c], want['arrival']), c
        assert np.array_equal(host['schedules'][c], want['schedule']), c
    return host


def replay_on_device(cases, sol):
    """Every solved case's schedule through BatchedRollout.move (tie_mode 'lowest'): positions equal the schedule at
    every step, no move or predict collision flag."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    ids = np.nonzero(sol.status.cpu().numpy() == 0)[0]
    assert len(ids)
    sched = [sol.schedule(int(c)) for c in ids]
    T = max(len(s) for s in sched)
    full = np.stack([np.concatenate([s, np.repeat(s[-1:], T - len(s), 0)]) for s in sched])      # [S,T,N,2]
    grids = np.stack([cases[c][0] for c in ids])
    acts = np.stack([mc.actions_of(f) for f in full])                                        # [S,T-1,N]
    ro = BatchedRollout(grids, full[:, 0], np.stack([cases[c][2] for c in ids]), 10 ** 6, DEV, tie_mode='lowest')
    for t in range(T - 1):
        flags = ro.move(actions=torch.from_numpy(np.ascontiguousarray(acts[:, t])).to(DEV))
        assert int(flags[:, 1:].abs().sum()) == 0, 'collision flag at step %d' % (t + 1)
        assert np.array_equal(ro.pos.cpu().numpy(), full[:, t + 1]), 'positions differ after step %d' % (t + 1)
    for k, c in enumerate(ids):
        g, s, gl = cases[c]
        mc.check_plans(g, s, gl, sched[k], sol.arrival[c].cpu().numpy())


@pytest.mark.parametrize('N,side,count', [(10, 20, 200), (20, 20, 100), (40, 28, 40), (64, 40, 20), (128, 64, 4)])
def test_equal_to_yardstick(mapf, N, side, count):
    rng = np.random.default_rng(100 * N + side)
    cases = mc.random_cases(rng, count, N, side, density=0.1)
    T = mc.default_horizon(side, side)
    sol = mapf.solve(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]),
                     np.stack([c[2] for c in cases]), DEV)
    host = assert_equal_to_yardstick(sol, cases, T)
    print('N=%d %dx%d: %d/%d solved' % (N, side, side, int((host['status'] == 0).sum()), count))
    replay_on_device(cases, sol)


@pytest.mark.parametrize('R', [1, 4])
def test_given_orders(mapf, R):
    rng = np.random.default_rng(7 + R)
    N, side, count = 20, 20, 60
    cases = mc.random_cases(rng, count, N, side, density=0.1)
    orders = np.stack([np.stack([rng.permutation(N) for _ in range(R)]) for _ in range(count)])
    orders[0, -1] = orders[0, 0]                        # a repeated order: a tie, kept by the lower index
    T = mc.default_horizon(side, side)
    sol = mapf.solve(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]),
                     np.stack([c[2] for c in cases]), DEV, priorities=orders)
    host = assert_equal_to_yardstick(sol, cases, T, orders)
    if R > 1:
        assert len(set(host['restart'].tolist())) > 1
    replay_on_device(cases, sol)


def test_default_restarts_are_seeded_permutations(mapf):
    rng = np.random.default_rng(3)
    cases = mc.random_cases(rng, 30, 20, 20, density=0.1)
    args = (np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases]), DEV)
    sol = mapf.solve(*args, restarts=4, seed=11)
    perm = np.argsort(np.random.default_rng(11).random((30, 3, 20)), axis=-1)
    orders = np.concatenate([np.broadcast_to(np.arange(20), (30, 1, 20)), perm], 1)
    assert_equal_to_yardstick(sol, cases, mc.default_horizon(20, 20), orders)


def _inputs(mapf, count=64, N=10, side=20, seed=0):
    rng = np.random.default_rng(seed)
    cases = mc.random_cases(rng, count, N, side, density=0.1)
    dev = torch.device(DEV)
    grid = torch.from_numpy(np.stack([c[0] for c in cases])).to(dev)
    start = torch.from_numpy(np.stack([c[1] for c in cases])).to(torch.int32).to(dev)
    goal = torch.from_numpy(np.stack([c[2] for c in cases])).to(torch.int32).to(dev)
    order = torch.from_numpy(np.stack([np.stack([np.arange(N), rng.permutation(N)]) for _ in cases])).to(torch.int32)
    return grid, start, goal, order.to(dev)


def _fresh(mapf, grid, start, order, T):
    out = mapf.empty_solutions(int(start.shape[0]), int(start.shape[1]), int(grid.shape[-2]), T, DEV, int(order.shape[1]))
    for k in OUTS:
        getattr(out, k).fill_(-7)
    return out


def test_identical_bytes_side_stream_and_graph(mapf):
    grid, start, goal, order = _inputs(mapf)
    T = 160
    runs = []
    for _ in range(2):
        out = _fresh(mapf, grid, start, order, T)
        mapf.enqueue_solve(grid, start, goal, order, out)
        torch.cuda.synchronize()
        runs.append(out)
    side_out = _fresh(mapf, grid, start, order, T)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mapf.enqueue_solve(grid, start, goal, order, side_out)
    side.synchronize()
    graphed = _fresh(mapf, grid, start, order, T)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mapf.enqueue_solve(grid, start, goal, order, graphed)
    torch.cuda.synchronize()
    assert (graphed.status == -7).all()                 # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    for other in (runs[1], side_out, graphed):
        for k in OUTS:
            assert torch.equal(getattr(runs[0], k), getattr(other, k)), k
    assert (runs[0].status == 0).any()
    graphed.schedules.fill_(-7)                         # a replay runs again on the same buffers
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.schedules, runs[0].schedules)


def test_rollout_failures_to_train_step(mapf):
    """A seeded rollout of an untrained policy -> solve_failures -> samples_from_solutions -> SamplePool -> train_step."""
    from gnn_pathplanning_amd import expert
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from gnn_pathplanning_amd.rollout import BatchedRollout
    from gnn_pathplanning_amd.training import train_step
    from oracle import policy_oracle as orc
    dev = torch.device(DEV)
    N, side, B = 10, 20, 16
    rng = np.random.default_rng(2024)
    cases = mc.random_cases(rng, B, N, side, density=0.1)
    grids = np.stack([c[0] for c in cases])
    goals = np.stack([c[2] for c in cases])

    class Cfg:
        num_agents, nGraphFilterTaps, device = N, 3, dev

    def model():
        net = DecentralPlannerNet(Cfg()).to(dev)
        net.load_state_dict(orc.init_state_dict(3, seed=7))
        return net

    ro = BatchedRollout(grids, np.stack([c[1] for c in cases]), goals, 24, dev, commR=6.0)
    res = ro.run(model().eval())
    sol = expert.solve_failures(ro, results=res)
    assert sol is not None and len(sol) == int((~res['success']).sum())
    fail = sol.episodes
    pos = res['positions'].numpy()
    # the yardstick on the CPU solves the same cases the same way (at least one of them)
    host = assert_equal_to_yardstick(sol, [(grids[b], pos[b], goals[b]) for b in fail], mc.default_horizon(side, side))
    assert (host['status'] == 0).any()
    samples, ids = expert.samples_from_solutions(sol, grids[fail], goals[fail])
    assert len(ids) == int((host['status'] == 0).sum())
    assert len(samples) == sum(int(host['makespan'][c]) + 1 for c in ids)
    for k, c in enumerate(ids):                         # each case's targets: the schedule's own moves
        a, b = samples.bounds[k], samples.bounds[k + 1]
        sched = sol.schedule(int(c))
        want = np.zeros((b - a, N, 5), np.float32)
        acts = np.concatenate([mc.actions_of(sched), np.full((1, N), 4)], 0)
        want[np.arange(b - a)[:, None], np.arange(N)[None], acts] = 1
        assert np.array_equal(samples.target[a:b].cpu().numpy(), want)
    pool = expert.SamplePool()
    pool.append(samples)
    batch = pool.draw(16, torch.Generator(device=dev).manual_seed(3))
    net = model().train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    loss = train_step(net, opt, *batch).item()
    assert np.isfinite(loss)
