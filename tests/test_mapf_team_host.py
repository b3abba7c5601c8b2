"""CPU, no library: the host side of mapf.solve_team -- argument checks refused before anything reaches the device, no
CPU fallback, the rule by which expert.solve_failures picks the solver, the plain error of samples_from_solutions for
large teams, and the solution file round trip of a team-sized case (yardstick answers: tests/mapf_cases.py)."""
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


def test_limits_match_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gnnpp.h')).read()

    def macro(name):
        return int(text.split('#define ' + name)[1].split()[0])
    assert mapf.MAX_TEAM == macro('GNNPP_ROLLOUT_MAX_TEAM') == 1024
    assert mapf.MAX_TEAM_SIDE == macro('GNNPP_MAPF_TEAM_MAX_SIDE') == 256
    assert mapf.MAX_TEAM_STEPS == macro('GNNPP_MAPF_TEAM_MAX_STEPS') == 2048
    assert mapf.MAX_TEAM_SIDE ** 2 <= macro('GNNPP_ROLLOUT_TEAM_MAX_CELLS')
    assert mapf.MAX_TEAM_STEPS == mc.default_horizon(mapf.MAX_TEAM_SIDE, mapf.MAX_TEAM_SIDE)
    assert (mapf.MAX_AGENTS, mapf.MAX_SIDE, mapf.MAX_STEPS) == (128, 64, 1024)          # solve() keeps its own
    assert mapf.team_slot_bytes(128, 128, 1024) == 1025 * 6 * 128 * 2 * 8
    assert mapf.team_slot_bytes(256, 256, 2048) == 2049 * 6 * 256 * 4 * 8
    assert mapf.team_slot_bytes(8, 65, 0) == 6 * 8 * 2 * 8


def test_no_cpu_fallback():
    grid, starts, goals = mc.random_cases(np.random.default_rng(1), 1, 3, 8)[0]
    with pytest.raises(_native.GnnppError, match='HIP device'):
        mapf.solve_team(grid, starts[None], goals[None], 'cpu')
    T = 8
    out = mapf.Solutions(**{k: torch.zeros(s, dtype=torch.int32) for k, s in (
        ('schedules', (1, T + 1, 3, 2)), ('arrival', (1, 3)), ('makespan', (1,)), ('flowtime', (1,)), ('status', (1,)),
        ('failing', (1,)), ('restart', (1,)))}, workspace=torch.zeros(1 << 16, dtype=torch.uint8))
    args = [torch.from_numpy(a).to(torch.int32) for a in (starts[None], goals[None])]
    with pytest.raises(_native.GnnppError, match='no CPU fallback'):
        mapf.enqueue_solve_team(torch.from_numpy(grid), args[0], args[1], None, out)


def test_argument_checks():
    """Refused on the host, before anything reaches the device (no library is loaded: the device does not exist here)."""
    grid, starts, goals = mc.random_cases(np.random.default_rng(1), 1, 3, 8)[0]
    bad = [(dict(grids=grid, starts=starts, goals=goals), r'\[C,N,2\]'),
           (dict(grids=grid, starts=starts[None], goals=goals[None, :2]), r'\[C,N,2\]'),
           (dict(grids=np.stack([grid] * 2), starts=starts[None], goals=goals[None]), 'one map per case'),
           (dict(grids=np.zeros((257, 8), np.uint8), starts=starts[None], goals=goals[None]), 'at most 256 x 256'),
           (dict(grids=np.zeros((8, 257), np.uint8), starts=starts[None], goals=goals[None]), 'at most 256 x 256'),
           (dict(grids=grid, starts=np.zeros((1, 1025, 2)), goals=np.zeros((1, 1025, 2))), '1 to 1024 agents'),
           (dict(grids=grid, starts=np.zeros((1, 0, 2)), goals=np.zeros((1, 0, 2))), '1 to 1024 agents'),
           (dict(grids=grid, starts=starts[None], goals=goals[None], max_steps=2049), r'0 \.\. 2048'),
           (dict(grids=grid, starts=starts[None], goals=goals[None], max_steps=-1), r'0 \.\. 2048'),
           (dict(grids=grid, starts=starts[None], goals=goals[None], restarts=0), 'restarts'),
           (dict(grids=grid, starts=starts[None], goals=goals[None], priorities=np.zeros((1, 2, 4))), 'priorities')]
    for kw, match in bad:
        with pytest.raises(_native.GnnppError, match=match):
            mapf.solve_team(device='cuda:0', **kw)


def test_default_orders_are_shared_with_solve():
    """Restart 0 the index order, the others argsort of default_rng(seed).random: what tests/test_gpu_mapf.py pins for
    solve()."""
    got = mapf.default_orders(30, 20, 4, 11)
    perm = np.argsort(np.random.default_rng(11).random((30, 3, 20)), axis=-1)
    want = np.concatenate([np.broadcast_to(np.arange(20), (30, 1, 20)), perm], 1)
    assert np.array_equal(got, want)


class _StubRollout:
    """What solve_failures reads of a BatchedRollout."""

    def __init__(self, B, N, H, W, batched=True):
        self.device = torch.device('cpu')
        self.B, self.N, self.grid_batched = B, N, int(batched)
        self.grid = torch.zeros((B, H, W) if batched else (H, W), dtype=torch.uint8)
        self.pos = torch.arange(B * N * 2, dtype=torch.int32).reshape(B, N, 2)
        self.goal = self.pos + 1


@pytest.mark.parametrize('N,H,W,batched,team', [
    (128, 64, 64, True, False), (10, 20, 20, False, False), (129, 64, 64, True, True), (10, 65, 20, True, True),
    (10, 20, 65, False, True), (1024, 128, 128, True, True), (128, 64, 65, True, True)])
def test_solve_failures_picks_the_solver_by_size(monkeypatch, N, H, W, batched, team):
    calls = []

    def fake(name):
        def f(grid, starts, goals, device, **kw):
            calls.append((name, grid, starts, goals, kw))
            return mapf.Solutions(status=torch.zeros(len(starts), dtype=torch.int32))
        return f
    monkeypatch.setattr(mapf, 'solve', fake('solve'))
    monkeypatch.setattr(mapf, 'solve_team', fake('solve_team'))
    ro = _StubRollout(3, N, H, W, batched)
    sol = expert.solve_failures(ro, results={'success': np.array([True, False, False])}, restarts=2, seed=5)
    assert len(calls) == 1
    name, grid, starts, goals, kw = calls[0]
    assert name == ('solve_team' if team else 'solve')
    assert kw == dict(restarts=2, seed=5)
    assert sol.episodes.tolist() == [1, 2]
    assert torch.equal(starts, ro.pos[1:]) and torch.equal(goals, ro.goal[1:])
    assert tuple(grid.shape) == ((2, H, W) if batched else (H, W))
    calls.clear()
    assert expert.solve_failures(ro, results={'success': np.array([True, True, True])}) is None and not calls


def _host_solutions(cases, T):
    wants = [mc.solve_case(g, s, gl, T) for g, s, gl in cases]

    def t(key):
        return torch.tensor(np.array([w[key] for w in wants]), dtype=torch.int32)
    return mapf.Solutions(schedules=t('schedule'), arrival=t('arrival'), makespan=t('makespan'),
                          flowtime=t('flowtime'), status=t('status'), failing=t('failing'), restart=t('restart')), wants


def test_solution_yaml_round_trip_of_a_team_case():
    """140 agents on 70 x 70: beyond both limits of the one-wave solver."""
    cases = mc.random_cases(np.random.default_rng(9), 1, 140, 70, density=0.1)
    T = mc.default_horizon(70, 70)
    sol, wants = _host_solutions(cases, T)
    grid, starts, goals = cases[0]
    assert wants[0]['status'] == 0 and wants[0]['schedule'].max() >= 64
    text = sol.solution_yaml(0)
    assert text == ec.solution_yaml([[tuple(p) for p in path] for path in sol.paths(0)])
    g, gl, sched = expert.read_solution(expert.failure_case_yaml(grid, starts, goals), text)
    assert np.array_equal(g, grid) and np.array_equal(gl, goals)
    assert np.array_equal(sched, sol.schedule(0)) and sched.dtype == np.int64
    assert len(sched) == wants[0]['makespan'] + 1 and sched.shape[1] == 140
    assert 'cost: %d' % wants[0]['flowtime'] in text
    with pytest.raises(_native.GnnppError, match='at most 128 agents'):
        expert.samples_from_solutions(sol, grid, goals[None])
