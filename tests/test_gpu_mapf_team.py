"""MI355X: gnnpp_mapf_team_solve through mapf.solve_team against the sequential numpy restatement of the contract
(tests/mapf_cases.py) at the sizes the large-team simulator runs: equality of every output, the validator and the
reference simulator on the 130- and 160-agent cases, the 512-agent schedule replayed through the large-team simulator
kernels (BatchedRollout.move), default restarts, identical bytes across calls / slot counts / a side stream / a captured
graph, both entry points on a case both accept, and expert.solve_failures on a rollout of 160 agents."""
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


def stacked(cases):
    return np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])


def assert_equal_to_yardstick(sol, cases, T, orders=None):
    host = {k: getattr(sol, k).cpu().numpy() for k in OUTS}
    wants = []
    for c, (g, s, gl) in enumerate(cases):
        want = mc.solve_case(g, s, gl, T, None if orders is None else list(orders[c]))
        for k in ('status', 'restart', 'makespan', 'flowtime', 'failing'):
            assert int(host[k][c]) == want[k], (c, k, int(host[k][c]), want[k])
        assert np.array_equal(host['arrival'][c], want['arrival']), c
        assert np.array_equal(host['schedules'][c], want['schedule']), c
        wants.append(want)
    return host, wants


def solve_and_compare(mapf, seed, count, N, H, W, **kw):
    cases = mc.random_cases(np.random.default_rng(seed), count, N, H, W, density=0.1)
    T = mc.default_horizon(H, W)
    sol = mapf.solve_team(*stacked(cases), DEV, **kw)
    assert sol.schedules.shape == (count, T + 1, N, 2)
    host, wants = assert_equal_to_yardstick(sol, cases, T)
    print('seed %d, %d agents on %d x %d: status %s makespan %s flowtime %s' % (
        seed, N, H, W, host['status'].tolist(), host['makespan'].tolist(), host['flowtime'].tolist()))
    return cases, sol, host, wants


def test_rows_of_two_words(mapf):
    """3 cases of 20 agents on 8 x 65."""
    _, _, host, _ = solve_and_compare(mapf, 1, 3, 20, 8, 65)
    assert host['status'].tolist() == [0, 0, 0] and host['makespan'].tolist() == [42, 56, 57]


@pytest.mark.parametrize('seed,N,side,makespans', [(2, 130, 40, [72, 56]), (3, 160, 64, [96, 106])])
def test_teams_beyond_128_agents_checked_by_validator_and_simulator(mapf, seed, N, side, makespans):
    cases, sol, host, _ = solve_and_compare(mapf, seed, 2, N, side, side)
    assert host['status'].tolist() == [0, 0] and host['makespan'].tolist() == makespans
    for c, (g, s, gl) in enumerate(cases):
        sched = sol.schedule(c)
        assert len(sched) == makespans[c] + 1
        mc.check_plans(g, s, gl, sched, host['arrival'][c])
        mc.replay_through_simulator(g, gl, sched)


def test_256_agents_on_100x100(mapf):
    _, _, host, _ = solve_and_compare(mapf, 4, 1, 256, 100, 100)
    assert (host['status'][0], host['makespan'][0], host['flowtime'][0]) == (0, 167, 19250)


def test_512_agents_replayed_through_the_large_team_simulator(mapf):
    """The large-team solver and the large-team simulator kernels agree: every step of the device schedule through
    BatchedRollout.move reproduces the schedule's positions and flags no collision."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    cases, sol, host, _ = solve_and_compare(mapf, 5, 1, 512, 100, 100)
    assert (host['status'][0], host['makespan'][0], host['flowtime'][0]) == (0, 163, 38525)
    g, s, gl = cases[0]
    sched = sol.schedule(0)
    acts = mc.actions_of(sched)
    ro = BatchedRollout(g[None], sched[:1], gl[None], 10 ** 6, DEV, tie_mode='lowest')
    for t in range(len(sched) - 1):
        flags = ro.move(actions=torch.from_numpy(np.ascontiguousarray(acts[t][None])).to(DEV))
        assert int(flags[:, 1:].abs().sum()) == 0, 'collision flag at step %d' % (t + 1)
        assert np.array_equal(ro.pos.cpu().numpy()[0], sched[t + 1]), 'positions differ after step %d' % (t + 1)
    assert np.array_equal(ro.pos.cpu().numpy()[0], gl)


def test_largest_map(mapf):
    """130 agents on 256 x 256, T_max = 2048: a 100.7 MB slot."""
    _, sol, host, _ = solve_and_compare(mapf, 7, 1, 130, 256, 256)
    assert (host['status'][0], host['makespan'][0]) == (0, 388)
    assert sol.workspace.numel() == mapf.team_workspace_bytes(1, 1, 256, 256, 2048)


def test_default_restarts_are_seeded_permutations(mapf):
    cases = mc.random_cases(np.random.default_rng(3), 3, 140, 48, 70, density=0.1)
    T = mc.default_horizon(48, 70)
    sol = mapf.solve_team(*stacked(cases), DEV, restarts=4, seed=11)
    perm = np.argsort(np.random.default_rng(11).random((3, 3, 140)), axis=-1)
    orders = np.concatenate([np.broadcast_to(np.arange(140), (3, 1, 140)), perm], 1)
    host, _ = assert_equal_to_yardstick(sol, cases, T, orders)
    print('restarts chosen:', host['restart'].tolist(), 'status', host['status'].tolist())
    # fewer slots than items (12 items, 5 slots): the same bytes
    capped = mapf.solve_team(*stacked(cases), DEV, restarts=4, seed=11,
                             workspace_bytes=mapf.team_workspace_min_bytes(3, 4, 48, 70, T) +
                             4 * mapf.team_slot_bytes(48, 70, T))
    assert capped.workspace.numel() < sol.workspace.numel()
    for k in OUTS:
        assert torch.equal(getattr(sol, k), getattr(capped, k)), k


def test_same_bytes_as_the_one_wave_call(mapf):
    """Sizes both entry points accept: 20 cases of 64 agents on 40 x 40 (two restarts), 4 of 128 agents on 64 x 64."""
    for seed, count, N, side, R in ((6440, 20, 64, 40, 2), (12864, 4, 128, 64, 1)):
        cases = mc.random_cases(np.random.default_rng(seed), count, N, side, density=0.1)
        a = mapf.solve(*stacked(cases), DEV, restarts=R, seed=2)
        b = mapf.solve_team(*stacked(cases), DEV, restarts=R, seed=2)
        for k in OUTS:
            assert torch.equal(getattr(a, k), getattr(b, k)), (N, k)
        assert (a.status == 0).any()


def _inputs(N=140, H=20, W=70, count=12, seed=0):
    rng = np.random.default_rng(seed)
    cases = mc.random_cases(rng, count, N, H, W, density=0.1)
    dev = torch.device(DEV)
    grid = torch.from_numpy(np.stack([c[0] for c in cases])).to(dev)
    start = torch.from_numpy(np.stack([c[1] for c in cases])).to(torch.int32).to(dev)
    goal = torch.from_numpy(np.stack([c[2] for c in cases])).to(torch.int32).to(dev)
    order = torch.from_numpy(np.stack([np.stack([np.arange(N), rng.permutation(N)]) for _ in cases])).to(torch.int32)
    return grid, start, goal, order.to(dev)


def _fresh(mapf, grid, start, order, T, **kw):
    out = mapf.empty_solutions(int(start.shape[0]), int(start.shape[1]), int(grid.shape[-2]), T, DEV, int(order.shape[1]),
                               W=int(grid.shape[-1]), team=True, **kw)
    for k in OUTS:
        getattr(out, k).fill_(-7)
    out.workspace.fill_(0x5a)
    return out


def test_identical_bytes_side_stream_and_graph(mapf):
    grid, start, goal, order = _inputs()
    T = 200
    runs = []
    for _ in range(2):
        out = _fresh(mapf, grid, start, order, T)
        mapf.enqueue_solve_team(grid, start, goal, order, out)
        torch.cuda.synchronize()
        runs.append(out)
    one_slot = _fresh(mapf, grid, start, order, T, workspace_bytes=mapf.team_workspace_min_bytes(12, 2, 20, 70, T))
    mapf.enqueue_solve_team(grid, start, goal, order, one_slot)
    side_out = _fresh(mapf, grid, start, order, T)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mapf.enqueue_solve_team(grid, start, goal, order, side_out)
    side.synchronize()
    graphed = _fresh(mapf, grid, start, order, T)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mapf.enqueue_solve_team(grid, start, goal, order, graphed)
    torch.cuda.synchronize()
    assert (graphed.status == -7).all()                 # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    for other in (runs[1], one_slot, side_out, graphed):
        for k in OUTS:
            assert torch.equal(getattr(runs[0], k), getattr(other, k)), k
    assert (runs[0].status == 0).any() and not (runs[0].schedules == -7).any()
    graphed.schedules.fill_(-7)                         # a replay runs again on the same buffers
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.schedules, runs[0].schedules)


def test_workspace_smaller_than_one_slot_is_refused(mapf):
    from gnn_pathplanning_amd import _native
    grid, start, goal, order = _inputs(count=2)
    out = _fresh(mapf, grid, start, order, 50)
    least = mapf.team_workspace_min_bytes(2, 2, 20, 70, 50)
    out.workspace = out.workspace[:least - 1]
    with pytest.raises(_native.GnnppError, match='gnnpp_mapf_team_solve'):
        mapf.enqueue_solve_team(grid, start, goal, order, out)
    torch.cuda.synchronize()
    assert (out.status == -7).all() and (out.schedules == -7).all()
    with pytest.raises(_native.GnnppError, match='holds no slot'):
        mapf.empty_solutions(2, 140, 20, 50, DEV, 2, W=70, team=True, workspace_bytes=least - 1)


@pytest.mark.parametrize('steps', [0, 3])
def test_solve_failures_of_a_160_agent_rollout(mapf, steps):
    """expert.solve_failures on a BatchedRollout of 160 agents on 64 x 64 (the large-team simulator), stepped zero or
    a few times with random actions: the rollout's current positions are the starts."""
    from gnn_pathplanning_amd import expert
    from gnn_pathplanning_amd.rollout import BatchedRollout
    rng = np.random.default_rng(31)
    cases = mc.random_cases(rng, 2, 160, 64, density=0.1)
    grids, starts, goals = stacked(cases)
    ro = BatchedRollout(grids, starts, goals, 10 ** 6, DEV, tie_mode='lowest')
    for _ in range(steps):
        ro.move(actions=torch.from_numpy(rng.integers(0, 5, (2, 160))).to(DEV))
    res = ro.results()
    assert not res['success'].any()
    pos = res['positions'].numpy()
    assert (steps == 0) == np.array_equal(pos, starts)
    sol = expert.solve_failures(ro, results=res)
    assert sol.episodes.tolist() == [0, 1] and len(sol) == 2
    T = mc.default_horizon(64, 64)
    host, wants = assert_equal_to_yardstick(sol, [(grids[b], pos[b], goals[b]) for b in range(2)], T)
    assert np.array_equal(host['schedules'][:, 0], pos)
    assert (host['status'] == 0).any()


@pytest.mark.parametrize('seed', [10, 11, 12, 13, 14, 15])
def test_1024_agents_on_128x128(mapf, seed):
    _, _, host, _ = solve_and_compare(mapf, seed, 1, 1024, 128, 128)
    assert host['status'][0] == 0 and 207 <= host['makespan'][0] <= 230 and 103500 <= host['flowtime'][0] <= 111500


def test_1024_agents_without_a_path(mapf):
    _, _, host, _ = solve_and_compare(mapf, 6, 1, 1024, 128, 128)
    assert (host['status'][0], host['failing'][0]) == (mc.NO_PATH, 334)
