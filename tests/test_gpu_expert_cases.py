"""MI355X: the hand-built calls of tests/expert_cases.py (the ones tests/test_emu_expert.py and
tests/test_emu_expert_team.py run under the host emulation, which executes the work-items of a workgroup one at a time)
through gnnpp_schedule_samples and gnnpp_schedule_team_samples on the device: ragged cases in one call, a map per case,
calls without an fp64 copy, status bits that flag only their case, maps and teams that leave no LDS output stage, cases of
different growths, graph outputs off the 16-byte boundary, the thin maps 1 x 65 536 and 65 536 x 1 (team call), the
one-wave call's map limit of 16 384 cells a side from both sides, radii beyond every distance.  Every output starts out as -7; every built case equals the
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


def per_step_growths(call, c):
    return [ec.schedule_gso(call['schedules'][c][t:t + 1], call['radius0'])[2] for t in range(len(call['schedules'][c]))]


# ---- thin maps: 1 x 65 536 and 65 536 x 1 through the large-team call ------------------------------------------------
@pytest.mark.parametrize('H,W', ec.thin_shapes(ec.THIN_SIDE))
def test_team_thin_map_two_agents_on_both_ends(expert, H, W):
    """100 growths; the bounds pass 2^31 and end in the 0xffffffff clamp."""
    out = run_call(expert, ec.both_ends_call(H, W), team=True)
    assert out['growth'][0] == 100 and out['radius'][0] == 68903.06169911187
    assert (out['step_info'] & 0xffff).tolist() == [100, 100]


@pytest.mark.parametrize('H,W', ec.thin_shapes(ec.THIN_SIDE))
def test_team_thin_map_two_halves_on_the_ends(expert, H, W):
    call = ec.two_ends_call(H, W, 129)
    out = run_call(expert, call, team=True)
    assert out['step_info'].tolist() == per_step_growths(call, 0) == [ec.call_wants(call)[0]['growth']] * 2


@pytest.mark.parametrize('H,W,fp64', [(1, ec.THIN_SIDE, True), (ec.THIN_SIDE, 1, False)])
def test_team_thin_map_two_halves_on_the_ends_full_workgroup(expert, H, W, fp64):
    """1024 agents on 65 536 cells: the observe kernel's 96 960-byte LDS request; with and without the fp64 copy."""
    call = ec.two_ends_call(H, W, 1024, fp64)
    out = run_call(expert, call, team=True)
    assert (out['step_info'] & 0xffff).tolist() == [ec.call_wants(call)[0]['growth']] * 2


@pytest.mark.parametrize('H,W', ec.thin_shapes(ec.THIN_SIDE))
def test_team_thin_map_spread_and_unaligned_graph_outputs(expert, H, W):
    call = ec.spread_call(H, W, 129)
    out = run_call(expert, call, team=True)
    assert out['step_info'].tolist() == per_step_growths(call, 0)
    assert_same_bytes(out, run_call(expert, call, team=True, misalign=True))


@pytest.mark.parametrize('H,W', ec.thin_shapes(ec.THIN_SIDE))
def test_team_thin_map_walk_with_a_map_per_case(expert, H, W):
    run_call(expert, ec.walk_call(H, W, 129), team=True)
    run_call(expert, ec.walk_call(H, W, 129, fp64=False), team=True)


def test_team_thin_map_status_bits_flag_only_their_case(expert):
    call = ec.thin_status_bits_call()
    out = run_call(expert, call, team=True, untouched=('obs', 'S', 'S64', 'target'))
    assert out['status'][3] == ec.BAD_MOVE
    assert out['step_info'][3 + 1] & 0xffff == 0 and out['step_info'][6] & 0xffff == 0   # no search with a state off the map
    alone = device_call(expert, dict(call, goals=call['goals'][:1], schedules=call['schedules'][:1]), team=True)
    T = 3
    for c in (0, 4):                                    # the legal cases: the bytes of the case run alone
        for k in ('obs', 'S', 'S64', 'target', 'step_info'):
            assert out[k][c * T:(c + 1) * T].tobytes() == alone[k].tobytes(), k
        assert out['radius'][c] == alone['radius'][0] and out['growth'][c] == alone['growth'][0]


# ---- the one-wave call's map limit: a side of 16 384 ------------------------------------------------------------------
@pytest.mark.parametrize('N', [2, 128])
@pytest.mark.parametrize('H,W', ec.thin_shapes(ec.ONE_WAVE_SIDE))
def test_one_wave_map_limit_same_bytes_as_team_call(expert, H, W, N):
    call = ec.one_wave_limit_call(H, W, N)
    assert_same_bytes(run_call(expert, call, team=False), run_call(expert, call, team=True))


@pytest.mark.parametrize('H,W', ec.thin_shapes(ec.ONE_WAVE_SIDE + 1))
def test_one_cell_beyond_the_one_wave_map_limit(expert, H, W):
    """The one-wave call refuses the map -- the project's error, naming the call -- and writes nothing; so does
    samples_from_schedules; the team call builds it."""
    from gnn_pathplanning_amd import _native
    call = ec.beyond_one_wave_limit_call(H, W)
    refusal = r'^gnnpp_schedule_samples failed: .*not supported.*\(code -2\)$'
    with pytest.raises(_native.GnnppError, match=refusal):
        expert.samples_from_schedules(call['grids'], call['goals'], call['schedules'], DEV)
    # (device_call reads its outputs back only after a call that returns: the refused one through the C ABI itself)
    dev = torch.device(DEV)
    T, N = 2, 2
    bufs = {k: torch.full(shape, POISON, dtype=dt, device=dev) for k, shape, dt in (
        ('obs', (T, N, 3, 11, 11), torch.float32), ('S', (T, N, N), torch.float32), ('S64', (T, N, N), torch.float64),
        ('target', (T, N, 5), torch.float32), ('radius', (1,), torch.float64), ('growth', (1,), torch.int32),
        ('status', (1,), torch.int32), ('step_info', (T,), torch.int32))}
    out = expert.ScheduleSamples(input=bufs['obs'], GSO=bufs['S'], GSO64=bufs['S64'], target=bufs['target'],
                                 radius=bufs['radius'], growth=bufs['growth'], status=bufs['status'],
                                 step_growth=bufs['step_info'])
    with pytest.raises(_native.GnnppError, match=refusal):
        expert.enqueue_schedule_samples(torch.from_numpy(call['grids']).to(dev), torch.from_numpy(call['goals']).to(dev),
                                        torch.from_numpy(np.concatenate(call['schedules'])).to(dev),
                                        torch.tensor([0, T], dtype=torch.int32, device=dev), out)
    torch.cuda.synchronize()
    assert all(bool((t == POISON).all()) for t in bufs.values())
    run_call(expert, call, team=True)
    got = expert.samples_from_schedules_team(call['grids'], call['goals'], call['schedules'], DEV, keep_fp64_gso=True)
    assert np.array_equal(got.GSO64.cpu().numpy(), ec.call_wants(call)[0]['GSO'])


# ---- radii beyond every distance --------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius0', ec.HUGE_RADII, ids=repr)
def test_radius_beyond_every_distance(expert, radius0):
    """Status 0, growth 0, radius = radius0 bit for bit, every pair an edge: three agents on 1 x 40 through both calls,
    129 agents spread over 1 x 65 536 through the large-team call."""
    tiny, thin = ec.huge_radius_calls(radius0)
    for call in (tiny, thin):
        out = run_call(expert, call, team=True)
        N = call['goals'].shape[1]
        assert out['status'][0] == 0 and out['growth'][0] == 0 and (out['step_info'] == 0).all()
        assert out['radius'].tobytes() == np.array([radius0]).tobytes()
        assert ((out['S'] != 0) == ~np.eye(N, dtype=bool)).all() and ((out['S64'] != 0) == ~np.eye(N, dtype=bool)).all()
    assert_same_bytes(run_call(expert, tiny, team=False), run_call(expert, tiny, team=True))
