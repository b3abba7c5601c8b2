"""MI355X: every hand-built and seeded case of tests/mapf_cases.py (ONE_WAVE, TEAM, BOTH -- the ones tests/test_emu_mapf.py
and tests/test_emu_mapf_team.py run under the host emulation, which executes the work-items of a workgroup one at a
time) through gnnpp_mapf_solve and gnnpp_mapf_team_solve on the device: real waves, barriers, LDS and ballots.  Every
output of every case equals the sequential numpy restatement's, bit for bit.  The outputs start out as -7, so an element
a kernel never writes cannot pass; where the emulation test poisons the workspace it is full of 0x5a bytes here too.
Every solved hand-built case also goes through the validator and the reference simulator."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mapf_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEYS = ('schedule', 'arrival', 'makespan', 'flowtime', 'status', 'failing', 'restart')


@pytest.fixture(scope='module')
def mapf():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from gnn_pathplanning_amd import _native, mapf as m
    _native.lib()
    return m


def device_call(mapf, case, team, shared=False, workspace_bytes=None, poison_ws=None):
    """One enqueue_solve / enqueue_solve_team call on poisoned outputs; host arrays of every output.  shared: the map
    of case 0 passed once, for the whole call.  workspace_bytes: what the team call's workspace holds."""
    dev = torch.device(DEV)
    grid = case['grid'][0] if shared else case['grid']
    g = torch.from_numpy(np.ascontiguousarray(grid, dtype=np.uint8)).to(dev)
    start = torch.from_numpy(np.ascontiguousarray(case['starts'], dtype=np.int32)).to(dev)
    goal = torch.from_numpy(np.ascontiguousarray(case['goals'], dtype=np.int32)).to(dev)
    order = None
    if case['orders'] is not None:
        order = torch.from_numpy(np.ascontiguousarray(case['orders'], dtype=np.int32)).to(dev)
    C, N = start.shape[:2]
    H, W = grid.shape[-2:]
    R = 1 if order is None else int(order.shape[1])
    if team:
        out = mapf.empty_solutions(C, N, H, case['T'], dev, R, W=W, team=True, workspace_bytes=workspace_bytes)
    else:
        out = mapf.empty_solutions(C, N, H, case['T'], dev, R)
    for k in KEYS:
        getattr(out, 'schedules' if k == 'schedule' else k).fill_(mc.POISON)
    out.workspace.fill_(0x5a if (case['poison_ws'] if poison_ws is None else poison_ws) else 0)
    (mapf.enqueue_solve_team if team else mapf.enqueue_solve)(g, start, goal, order, out)
    torch.cuda.synchronize()
    host = {k: getattr(out, 'schedules' if k == 'schedule' else k).cpu().numpy() for k in KEYS}
    host['workspace_bytes'] = out.workspace.numel()
    return host


def run_case(mapf, case, team, **kw):
    out = device_call(mapf, case, team, **kw)
    mc.assert_outputs_equal(out, mc.wants_of(case))
    if case['structured']:
        mc.check_solved_plans(case, out)
    return out


def assert_same_bytes(a, b):
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize('name', sorted(mc.ONE_WAVE))
def test_one_wave_case(mapf, name):
    """gnnpp_mapf_solve: an agent on its goal steps aside and returns, target conflict, swap is no shortcut, a walled-in
    agent stops the plan, bad cases flag only themselves, bit 63 of a row and lane 63 of the wave, non-square maps,
    restart ties and the corridor only the reversed order solves."""
    run_case(mapf, mc.ONE_WAVE[name](), team=False)


@pytest.mark.parametrize('name', sorted(mc.TEAM))
def test_team_case(mapf, name):
    """gnnpp_mapf_team_solve: rows of two and three words (W = 65, 128, 129), the corridor crossing the word boundary
    both ways, the swap refused across columns 63 / 64, more than one wave of rows with one door between rows 63 and
    64, 70 x 130 with 140 agents, restarts, crowded and bad cases, T = 0 and N = 1."""
    run_case(mapf, mc.TEAM[name](), team=True)


@pytest.mark.parametrize('team', [False, True])
def test_batched_grid_next_to_shared_grid(mapf, team):
    case = (mc.TEAM if team else mc.ONE_WAVE)['batched_grid_next_to_shared_grid']()
    assert_same_bytes(run_case(mapf, case, team, shared=True), run_case(mapf, case, team))


@pytest.mark.parametrize('name', sorted(mc.BOTH))
def test_same_bytes_from_both_entry_points(mapf, name):
    case = mc.BOTH[name]()
    a = run_case(mapf, case, team=False, poison_ws=False)
    b = run_case(mapf, case, team=True, poison_ws=True)
    assert_same_bytes(a, b)


def test_outputs_do_not_depend_on_the_slot_count(mapf):
    """Ten work items with a slot each, with the one-slot workspace, and with three slots and 100 spare bytes."""
    case = mc.TEAM['outputs_do_not_depend_on_the_slot_count']()
    full = run_case(mapf, case, team=True)
    one = mapf.team_workspace_min_bytes(5, 2, 4, 66, 60)
    assert one < full['workspace_bytes'] == mapf.team_workspace_bytes(5, 2, 4, 66, 60)
    single = run_case(mapf, case, team=True, workspace_bytes=one)
    three = run_case(mapf, case, team=True, workspace_bytes=one + 2 * mapf.team_slot_bytes(4, 66, 60) + 100)
    assert single['workspace_bytes'] == one and three['workspace_bytes'] == one + 2 * (61 * 6 * 4 * 2 * 8) + 100
    assert_same_bytes(full, single)
    assert_same_bytes(full, three)
