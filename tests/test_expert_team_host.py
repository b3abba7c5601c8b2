"""CPU: the host side of expert.samples_from_schedules_team -- no CPU fallback, shape and team-size errors refused
before anything reaches the device, the size of a call's outputs, and the routing of samples_from_solutions (team=False
keeps the plain error for large teams, team=True reaches the team call)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mapf_cases as mc  # noqa: E402
from gnn_pathplanning_amd import _native, expert, mapf  # noqa: E402


def test_limits_match_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gnnpp.h')).read()
    assert expert.MAX_TEAM == int(text.split('#define GNNPP_ROLLOUT_MAX_TEAM')[1].split()[0]) == 1024
    assert expert.MAX_AGENTS == 128                     # samples_from_schedules keeps its own
    for name in ('gnnpp_schedule_team_workspace_bytes', 'gnnpp_schedule_team_samples'):
        assert name in _native.EXPORTS and name + '(' in text


def test_no_cpu_fallback():
    grid = np.zeros((20, 20), np.uint8)
    goal = np.zeros((1, 140, 2), np.int32)
    with pytest.raises(_native.GnnppError, match='no CPU fallback'):
        expert.samples_from_schedules_team(grid, goal, [np.zeros((2, 140, 2), np.int32)], 'cpu')
    T, N = 2, 140
    out = expert.ScheduleSamples(
        input=torch.zeros(T, N, 3, 11, 11), GSO=torch.zeros(T, N, N), GSO64=None, target=torch.zeros(T, N, 5),
        radius=torch.zeros(1, dtype=torch.float64), growth=torch.zeros(1, dtype=torch.int32),
        status=torch.zeros(1, dtype=torch.int32), step_growth=torch.zeros(T, dtype=torch.int32),
        workspace=torch.zeros(T * N * 8, dtype=torch.uint8))
    with pytest.raises(_native.GnnppError, match='no CPU fallback'):
        expert.enqueue_schedule_team_samples(torch.from_numpy(grid), torch.from_numpy(goal),
                                             torch.zeros(T, N, 2, dtype=torch.int32),
                                             torch.tensor([0, T], dtype=torch.int32), out)


def test_argument_checks():
    """Refused on the host, before anything reaches the device (the device does not exist here)."""
    grid = np.zeros((20, 20), np.uint8)

    def sched(T, N):
        return np.zeros((T, N, 2), np.int32)
    bad = [(dict(grids=grid, goals=np.zeros((140, 2)), schedules=[sched(2, 140)]), r'\[C,N,2\]'),
           (dict(grids=grid, goals=np.zeros((2, 140, 2)), schedules=[sched(2, 140)]), r'\[C,N,2\]'),
           (dict(grids=grid, goals=np.zeros((0, 140, 2)), schedules=[]), r'\[C,N,2\]'),
           (dict(grids=np.stack([grid] * 2), goals=np.zeros((1, 140, 2)), schedules=[sched(2, 140)]), r'\[H,W\] or \[C,H,W\]'),
           (dict(grids=grid, goals=np.zeros((1, 1025, 2)), schedules=[sched(2, 1025)]), r'2 to 1024 agents \(got 1025\)'),
           (dict(grids=grid, goals=np.zeros((1, 1, 2)), schedules=[sched(2, 1)]), r'2 to 1024 agents \(got 1\)'),
           (dict(grids=grid, goals=np.zeros((2, 140, 2)), schedules=[sched(2, 140), sched(2, 139)]), r'schedule 1 must be'),
           (dict(grids=grid, goals=np.zeros((1, 140, 2)), schedules=[sched(0, 140)]), r'schedule 0 must be')]
    for kw, match in bad:
        with pytest.raises(_native.GnnppError, match=match):
            expert.samples_from_schedules_team(device='cuda:0', **kw)
    with pytest.raises(_native.GnnppError, match=r'2 to 128 agents \(got 140\)'):         # the one-wave call: unchanged
        expert.samples_from_schedules(grid, np.zeros((1, 140, 2)), [sched(2, 140)], 'cuda:0')


def test_team_output_bytes():
    for T, N in ((1, 2), (3, 1024), (2100, 1024), (7, 130)):
        tensors = T * N * 3 * 11 * 11 * 4 + T * N * N * 4 + T * N * 5 * 4
        assert expert.team_output_bytes(T, N) == tensors == T * N * (1452 + 4 * N + 20)
        assert expert.team_output_bytes(T, N, keep_fp64_gso=True) == tensors + T * N * N * 8
    assert round(expert.team_output_bytes(1, 1024) / 1e6, 1) == 5.7
    assert expert.team_output_bytes(2100, 1024) > 2 ** 33          # (an int, not a 32-bit count)


def _host_solutions(cases, T):
    wants = [mc.solve_case(g, s, gl, T) for g, s, gl in cases]

    def t(key):
        return torch.tensor(np.array([w[key] for w in wants]), dtype=torch.int32)
    return mapf.Solutions(schedules=t('schedule'), arrival=t('arrival'), makespan=t('makespan'),
                          flowtime=t('flowtime'), status=t('status'), failing=t('failing'), restart=t('restart')), wants


def test_samples_from_solutions_routes_by_the_team_flag(monkeypatch):
    """140 agents on 70 x 70, two cases of which the second is made unsolvable by a horizon of its own."""
    cases = mc.random_cases(np.random.default_rng(9), 2, 140, 70, density=0.1)
    T = mc.default_horizon(70, 70)
    sol, wants = _host_solutions(cases, T)
    assert wants[0]['status'] == 0
    sol.status[1] = 1                                   # case 1 counts as unsolved
    grids = np.stack([g for g, _, _ in cases])
    goals = np.stack([gl for _, _, gl in cases])
    calls = []

    def fake(name):
        def f(g, gl, sched, dev, commR=5.0, keep_fp64_gso=False):
            calls.append((name, g, gl, sched, dev, commR))
            return name
        return f
    monkeypatch.setattr(expert, 'samples_from_schedules', fake('one-wave'))
    monkeypatch.setattr(expert, 'samples_from_schedules_team', fake('team'))
    with pytest.raises(_native.GnnppError, match=r'at most 128 agents.*team=True'):
        expert.samples_from_solutions(sol, grids, goals)
    assert not calls
    got, ids = expert.samples_from_solutions(sol, grids, goals, commR=6.0, team=True)
    assert got == 'team' and ids.tolist() == [0] and len(calls) == 1
    name, g, gl, sched, dev, commR = calls[0]
    assert commR == 6.0 and dev == torch.device('cpu')
    assert np.array_equal(g.numpy(), grids[:1]) and np.array_equal(gl.numpy(), goals[:1])
    assert len(sched) == 1 and np.array_equal(sched[0].numpy(), sol.schedule(0))
    assert len(sched[0]) == wants[0]['makespan'] + 1
    # small teams: the default keeps the one-wave call, team=True takes the team call for them too
    small = mc.random_cases(np.random.default_rng(2), 1, 5, 12)
    ssol, _ = _host_solutions(small, 30)
    calls.clear()
    assert expert.samples_from_solutions(ssol, small[0][0], small[0][2][None])[0] == 'one-wave'
    assert expert.samples_from_solutions(ssol, small[0][0], small[0][2][None], team=True)[0] == 'team'
    assert [c[0] for c in calls] == ['one-wave', 'team']
