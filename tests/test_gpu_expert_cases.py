"""MI355X: the hand-built calls of tests/expert_cases.py (the ones tests/test_emu_expert.py and
tests/test_emu_expert_team.py run under the host emulation, which executes the work-items of a workgroup one at a time)
through gnnpp_schedule_samples and gnnpp_schedule_team_samples on the device: ragged cases in one call, a map per case,
calls without an fp64 copy, status bits that flag only their case, maps and teams that leave no LDS output stage, cases of
different growths, graph outputs off the 16-byte boundary.  Every output starts out as -7; every built case equals the
sequential numpy restatement, element for element, and a flagged case leaves its rows as they were."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expert_cases as ec  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POISON = -7
KEYS = {'obs': 'input', 'S': 'GSO', 'S64': 'GSO64', 'target': 'target', 'radius': 'radius', 'growth': 'growth',
        'status': 'status', 'step_info': 'step_growth'}


@pytest.fixture(scope='module')
def expert():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from gnn_pathplanning_amd import _native, expert as ex
    _native.lib()
    return ex


def device_call(expert, call, team, misalign=False):
    """One enqueue_schedule_samples / enqueue_schedule_team_samples call on poisoned outputs; host arrays of every
    output.  misalign: S and S64 start 4 / 8 bytes past a 16-byte boundary (the narrow store path)."""
    dev = torch.device(DEV)
    grid = torch.from_numpy(call['grids']).to(dev)
    goal = torch.from_numpy(call['goals']).to(dev)
    pos = torch.from_numpy(np.ascontiguousarray(np.concatenate(call['schedules'], 0))).to(dev)
    bounds = np.cumsum([0] + [len(s) for s in call['schedules']]).tolist()
    start = torch.tensor(bounds, dtype=torch.int32, device=dev)
    C, N = call['goals'].shape[:2]
    T = bounds[-1]

    def f(*shape, dtype=torch.float32):
        return torch.full(shape, POISON, dtype=dtype, device=dev)

    def graph(dtype):
        raw = f(T * N * N + 1, dtype=dtype)
        assert raw.data_ptr() % 16 == 0
        return raw[int(misalign):int(misalign) + T * N * N].view(T, N, N)

    from gnn_pathplanning_amd import _native
    nbytes = _native.lib().gnnpp_schedule_team_workspace_bytes(N, T)
    assert nbytes > 0
    S, S64 = graph(torch.float32), graph(torch.float64) if call['fp64'] else None
    assert (S.data_ptr() % 16 != 0) == misalign and (S64 is None or (S64.data_ptr() % 16 != 0) == misalign)
    out = expert.ScheduleSamples(input=f(T, N, 3, 11, 11), GSO=S, GSO64=S64, target=f(T, N, 5),
                                 radius=f(C, dtype=torch.float64), growth=f(C, dtype=torch.int32),
                                 status=f(C, dtype=torch.int32), step_growth=f(T, dtype=torch.int32), bounds=bounds,
                                 workspace=torch.full((nbytes,), 0x5a, dtype=torch.uint8, device=dev))
    (expert.enqueue_schedule_team_samples if team else expert.enqueue_schedule_samples)(grid, goal, pos, start, out,
                                                                                       commR=call['radius0'])
    torch.cuda.synchronize()
    return {k: None if getattr(out, name) is None else getattr(out, name).cpu().numpy() for k, name in KEYS.items()}


def run_call(expert, call, team, untouched=('obs', 'S'), **kw):
    out = device_call(expert, call, team, **kw)
    ec.assert_call_outputs(out, call, POISON, untouched)
    return out


def assert_same_bytes(a, b):
    for k in KEYS:
        assert (a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes(), k


def test_ragged_cases_in_one_call(expert):
    out = run_call(expert, ec.ragged_call(0), team=False)
    assert len(set(out['growth'].tolist())) > 1        # (the parts really have radii of their own)


@pytest.mark.parametrize('ci', [0, 4])
def test_batched_maps_and_no_fp64_copy(expert, ci):
    run_call(expert, ec.batched_maps_call_without_fp64_copy(ci), team=False)


def test_status_bits_flag_only_their_case(expert):
    run_call(expert, ec.status_bits_call(), team=False)


def test_large_team_and_map_without_stage(expert):
    for call in ec.calls_without_stage():
        run_call(expert, call, team=False)


def test_radii_that_share_an_integer_bound(expert):
    """radius0 = 1.0 through the one-wave and the large-team call: the same bytes, growth over repeated thresholds."""
    call = ec.repeated_bounds_call()
    out = run_call(expert, call, team=False)
    assert (out['step_info'] & 0xffff).tolist() == [12, 12, 8, 8]
    assert_same_bytes(run_call(expert, call, team=True), out)


def test_teams_at_the_second_agent_per_lane(expert):
    for call in ec.lane_boundary_calls():
        run_call(expert, call, team=False)


@pytest.mark.parametrize('fp64', [False, True])
@pytest.mark.parametrize('ci', [4, 0])
def test_team_ragged_cases_and_batched_maps_same_bytes_as_one_wave_call(expert, ci, fp64):
    call = ec.ragged_call_with_a_map_per_case(ci, fp64)
    assert_same_bytes(run_call(expert, call, team=True), run_call(expert, call, team=False))


def test_team_unaligned_graph_outputs_give_the_same_bytes(expert):
    """S / S64 off the 16-byte boundary take the 4-byte store path of the large-team call: same values."""
    call = ec.ragged_call_with_a_map_per_case(4, True)
    assert_same_bytes(run_call(expert, call, True, misalign=True), run_call(expert, call, True))


def test_team_cases_of_different_growths_in_one_call_without_fp64_copy(expert):
    call = ec.team_growths_call()
    out = run_call(expert, call, team=True)
    wants = ec.call_wants(call)
    assert wants[0]['growth'] != wants[1]['growth']
    a = len(call['schedules'][0])                       # step_info: every step's own growths, the case's the largest
    for c, rows in enumerate((out['step_info'][:a], out['step_info'][a:])):
        assert rows.tolist() == [ec.schedule_gso(call['schedules'][c][t:t + 1])[2] for t in range(len(rows))]


def test_team_status_bits_flag_only_their_case(expert):
    call = ec.team_status_bits_call()
    out = run_call(expert, call, team=True, untouched=('obs', 'S', 'S64', 'target'))
    assert out['step_info'][3 * 4] & 0xffff == 0        # no graph search for a step with a state off the map
