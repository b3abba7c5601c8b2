"""CPU: the yardstick of the MAPF solver (tests/mapf_cases.py) checked by independent means -- a plain (cell, t)
breadth-first search confirms every arrival is the minimum and every failure genuine, the validator and the reference
simulator (oracle.rollout_oracle.move_step) accept every solved schedule -- and the host side of mapf.py: argument
checks, no CPU fallback, and the solution file round trip through expert.read_solution."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expert_cases as ec  # noqa: E402
import mapf_cases as mc  # noqa: E402
from gnn_pathplanning_amd import _native, expert, mapf  # noqa: E402


def check_against_bfs(grid, starts, goals, T, order=None):
    """Replan every agent with the plain search, given the earlier agents' actual (padded) paths."""
    N = len(starts)
    order = list(range(N)) if order is None else list(order)
    st, arrival, paths, failing = mc.plan_order(grid, starts, goals, order, T)
    earlier = []
    for i in order:
        a = mc.bfs_arrival(grid, starts[i], goals[i], earlier, T)
        if i == failing:
            assert a is None, 'agent %d has a path (arrival %d) the restatement missed' % (i, a)
            return st
        assert a == arrival[i], 'agent %d: restatement %d, search %s' % (i, arrival[i], a)
        p = paths[i]
        earlier.append(np.concatenate([p, np.repeat(p[-1:], T + 1 - len(p), 0)]))
    return st


@pytest.mark.parametrize('N,side,count,density', [(10, 20, 12, 0.1), (6, 9, 20, 0.25), (12, 8, 12, 0.2)])
def test_yardstick_against_plain_search_and_simulator(N, side, count, density):
    rng = np.random.default_rng(N * side)
    statuses = []
    for grid, starts, goals in mc.random_cases(rng, count, N, side, density=density):
        T = mc.default_horizon(side, side) if side > 10 else 16
        order = rng.permutation(N)
        statuses.append(check_against_bfs(grid, starts, goals, T, order))
        want = mc.solve_case(grid, starts, goals, T, [order])
        if want['status'] == 0:
            sched = want['schedule'][:want['makespan'] + 1]
            mc.check_plans(grid, starts, goals, sched, want['arrival'])
            mc.replay_through_simulator(grid, goals, sched)
    assert 0 in statuses
    if side < 10:
        assert mc.NO_PATH in statuses                   # the dense small maps exercise genuine failures too


def test_edge_cases_against_plain_search():
    grid = np.array([[1, 1, 0, 1, 1], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], np.uint8)
    assert check_against_bfs(grid, np.array([[1, 0], [1, 2]]), np.array([[1, 4], [1, 2]]), 12) == 0
    grid = np.zeros((2, 2), np.uint8)
    assert check_against_bfs(grid, np.array([[0, 0], [0, 1]]), np.array([[0, 1], [0, 0]]), 8) == 0
    grid = np.array([[0, 0, 0], [1, 0, 1]], np.uint8)
    assert check_against_bfs(grid, np.array([[1, 1], [0, 0]]), np.array([[0, 1], [0, 2]]), 10) == mc.NO_PATH


def test_validator_rejects_conflicts():
    grid = np.zeros((3, 3), np.uint8)
    starts, goals = np.array([[0, 0], [0, 1]]), np.array([[0, 1], [0, 0]])
    swap = np.array([[[0, 0], [0, 1]], [[0, 1], [0, 0]]])
    with pytest.raises(AssertionError, match='swap'):
        mc.check_plans(grid, starts, goals, swap, [1, 1])
    with pytest.raises(AssertionError):
        mc.replay_through_simulator(grid, goals, swap)
    clash = np.array([[[0, 0], [0, 2]], [[0, 1], [0, 1]]])
    with pytest.raises(AssertionError, match='vertex'):
        mc.check_plans(grid, clash[0], np.array([[0, 1], [0, 1]]), clash, [1, 1])


def _host_solutions(cases, T):
    """A Solutions of CPU tensors holding the yardstick's answer (only the host-side methods are exercised)."""
    wants = [mc.solve_case(g, s, gl, T) for g, s, gl in cases]

    def t(key):
        return torch.tensor(np.array([w[key] for w in wants]), dtype=torch.int32)
    return mapf.Solutions(schedules=t('schedule'), arrival=t('arrival'), makespan=t('makespan'),
                          flowtime=t('flowtime'), status=t('status'), failing=t('failing'), restart=t('restart')), wants


def test_solution_yaml_round_trip():
    rng = np.random.default_rng(4)
    cases = mc.random_cases(rng, 4, 10, 20)
    T = mc.default_horizon(20, 20)
    sol, wants = _host_solutions(cases, T)
    for c, (grid, starts, goals) in enumerate(cases):
        assert wants[c]['status'] == 0
        text = sol.solution_yaml(c)
        paths = sol.paths(c)
        assert text == ec.solution_yaml([[tuple(p) for p in path] for path in paths])
        g, gl, sched = expert.read_solution(expert.failure_case_yaml(grid, starts, goals), text)
        assert np.array_equal(g, grid) and np.array_equal(gl, goals)
        assert np.array_equal(sched, sol.schedule(c)) and sched.dtype == np.int64
        assert len(sched) == wants[c]['makespan'] + 1
        assert 'cost: %d' % wants[c]['flowtime'] in text


def test_unsolved_case_is_reported_not_raised_until_asked():
    grid = np.zeros((6, 6), np.uint8)
    grid[3:6, 3] = 1
    grid[3, 3:6] = 1
    sol, _ = _host_solutions([(grid, np.array([[0, 0], [5, 5]]), np.array([[1, 1], [0, 3]]))], 30)
    assert sol.solved().tolist() == [False]
    with pytest.raises(_native.GnnppError, match='no path for agent 1'):
        sol.schedule(0)


def test_no_cpu_fallback():
    grid, starts, goals = mc.random_cases(np.random.default_rng(1), 1, 3, 8)[0]
    with pytest.raises(_native.GnnppError, match='HIP device'):
        mapf.solve(grid, starts[None], goals[None], 'cpu')
    T = 8
    out = mapf.Solutions(**{k: torch.zeros(s, dtype=torch.int32) for k, s in (
        ('schedules', (1, T + 1, 3, 2)), ('arrival', (1, 3)), ('makespan', (1,)), ('flowtime', (1,)), ('status', (1,)),
        ('failing', (1,)), ('restart', (1,)))}, workspace=torch.zeros(1 << 16, dtype=torch.uint8))
    args = [torch.from_numpy(a).to(torch.int32) for a in (starts[None], goals[None])]
    with pytest.raises(_native.GnnppError, match='no CPU fallback'):
        mapf.enqueue_solve(torch.from_numpy(grid), args[0], args[1], None, out)


def test_argument_checks():
    """Refused on the host, before anything reaches the device."""
    grid, starts, goals = mc.random_cases(np.random.default_rng(1), 1, 3, 8)[0]
    bad = [dict(grids=grid, starts=starts, goals=goals),                                 # not [C,N,2]
           dict(grids=grid, starts=starts[None], goals=goals[None, :2]),
           dict(grids=np.stack([grid] * 2), starts=starts[None], goals=goals[None]),     # a map per case: 2 != 1
           dict(grids=np.zeros((65, 8), np.uint8), starts=starts[None], goals=goals[None]),
           dict(grids=grid, starts=np.zeros((1, 129, 2)), goals=np.zeros((1, 129, 2))),
           dict(grids=grid, starts=starts[None], goals=goals[None], max_steps=1025),
           dict(grids=grid, starts=starts[None], goals=goals[None], max_steps=-1),
           dict(grids=grid, starts=starts[None], goals=goals[None], restarts=0),
           dict(grids=grid, starts=starts[None], goals=goals[None], priorities=np.zeros((1, 2, 4)))]
    for kw in bad:
        with pytest.raises(_native.GnnppError):
            mapf.solve(device='cuda:0', **kw)
