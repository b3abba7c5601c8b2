"""CPU: gnnpp_schedule_samples (csrc/expert_kernels.hip), compiled unmodified for the host emulation, against what the
REAL reference transformer made of the golden cases (tests/golden/expert_schedules.npz): equality, every element."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expert_cases as ec  # noqa: E402
from gnn_pathplanning_amd._native import ERR_ARG, ERR_UNSUPPORTED, ScheduleStruct  # noqa: E402
from gnn_pathplanning_amd._native import SCHEDULE_BAD_MOVE as BAD_MOVE, SCHEDULE_BAD_STATE as BAD_STATE  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


@pytest.fixture(scope='module')
def lib():
    import emu_lib
    return emu_lib.load()


def call(lib, grids, goals, schedules, radius0=5.0, fp64=True, expect=0, poison=np.nan):
    """One gnnpp_schedule_samples call on host arrays; outputs start out poisoned, so an element the call does not
    write cannot pass for one it wrote."""
    grid = np.ascontiguousarray(grids, dtype=np.uint8)
    goal = np.ascontiguousarray(goals, dtype=np.int32)
    C, N = goal.shape[:2]
    pos = np.ascontiguousarray(np.concatenate(schedules, 0), dtype=np.int32)
    start = np.ascontiguousarray(np.cumsum([0] + [len(s) for s in schedules]), dtype=np.int32)
    T = int(start[-1])
    out = {'obs': np.full((T, N, 3, 11, 11), poison, np.float32), 'S': np.full((T, N, N), poison, np.float32),
           'S64': np.full((T, N, N), poison, np.float64), 'target': np.full((T, N, 5), poison, np.float32),
           'radius': np.full(C, poison, np.float64), 'growth': np.full(C, -1, np.int32),
           'status': np.full(C, -1, np.int32), 'step_info': np.full(T, -1, np.int32), 'start': start}
    s = ScheduleStruct()
    s.grid, s.grid_batched, s.goal, s.pos = grid.ctypes.data, int(grid.ndim == 3), goal.ctypes.data, pos.ctypes.data
    s.case_start, s.C, s.N, s.H, s.W, s.T_total = start.ctypes.data, C, N, grid.shape[-2], grid.shape[-1], T
    s.radius0 = radius0
    s.obs, s.S, s.target = out['obs'].ctypes.data, out['S'].ctypes.data, out['target'].ctypes.data
    s.S64 = out['S64'].ctypes.data if fp64 else None
    s.radius, s.growth, s.status = out['radius'].ctypes.data, out['growth'].ctypes.data, out['status'].ctypes.data
    s.step_info = out['step_info'].ctypes.data
    assert lib.gnnpp_schedule_samples(ctypes.byref(s), None) == expect
    return out


def assert_case_equals_golden(out, c, m, g):
    a, b = int(out['start'][c]), int(out['start'][c + 1])
    assert out['status'][c] == 0
    assert out['growth'][c] == m['growth']
    assert out['radius'][c] == float.fromhex(m['radius'])
    assert np.array_equal(out['obs'][a:b], g['input'].astype(np.float32))
    assert np.array_equal(out['target'][a:b], g['target'].astype(np.float32))
    assert np.array_equal(out['S64'][a:b], g['GSO'])
    assert np.array_equal(out['S'][a:b], g['GSO'].astype(np.float32))
    assert (out['step_info'][a:b] >> 16 == 0).all() and (out['step_info'][a:b] & 0xffff).max() == m['growth']


@pytest.mark.parametrize('ci', range(8))
def test_golden_case(lib, ci):
    m, g = ec.load_golden()[ci]
    out = call(lib, g['grid'], g['goal'][None], [g['schedule']])
    assert_case_equals_golden(out, 0, m, g)


def test_ragged_cases_in_one_call(lib):
    """Cases of 25, 7 and 3 steps share a call: the 10-agent 20 x 20 case, its first 7 steps and its last 3 (each a
    schedule of its own, with its own radius)."""
    m, g = ec.load_golden()[0]
    case = ec.ragged_call(0)
    parts, goals = case['schedules'], case['goals']
    out = call(lib, case['grids'], goals, parts)
    ec.assert_call_outputs(out, case, np.nan)
    assert_case_equals_golden(out, 0, m, g)
    assert list(out['start']) == [0, 25, 32, 35]
    for c, part in enumerate(parts):
        want = ec.reference_samples(g['grid'], goals[c], part)
        a, b = int(out['start'][c]), int(out['start'][c + 1])
        assert out['radius'][c] == want['radius'] and out['growth'][c] == want['growth']
        assert np.array_equal(out['S64'][a:b], want['GSO'])
        assert np.array_equal(out['obs'][a:b], want['input'])
        assert np.array_equal(out['target'][a:b], want['target'])
    assert len(set(out['growth'].tolist())) > 1        # (the parts really have radii of their own)


def test_batched_maps_and_no_fp64_copy(lib):
    """One map per case (grid_batched), S64 = NULL."""
    gold = ec.load_golden()
    for ci in (0, 4):                                   # 10 and 24 agents: two calls; per call two maps
        m, g = gold[ci]
        case = ec.batched_maps_call_without_fp64_copy(ci)
        other, fgoal, flipped = case['grids'][0], case['goals'][0], case['schedules'][0]
        out = call(lib, case['grids'], case['goals'], case['schedules'], fp64=False)
        a = int(out['start'][1])
        assert out['status'].tolist() == [0, 0] and out['growth'].tolist() == [m['growth']] * 2
        assert np.array_equal(out['obs'][a:], g['input'].astype(np.float32))
        assert np.array_equal(out['S'][a:], g['GSO'].astype(np.float32))
        assert np.isnan(out['S64']).all()
        want = ec.reference_samples(other, fgoal, flipped)
        assert np.array_equal(out['obs'][:a], want['input']) and np.array_equal(out['target'][:a], want['target'])
        assert np.array_equal(out['S'][:a], want['GSO'].astype(np.float32))


def test_restatement_equals_reference():
    """tests/expert_cases.py (the yardstick of the random cases) against the real reference's tensors."""
    for m, g in ec.load_golden():
        want = ec.reference_samples(g['grid'], g['goal'], g['schedule'])
        assert want['radius'] == float.fromhex(m['radius']) and want['growth'] == m['growth']
        assert np.array_equal(want['GSO'], g['GSO'])
        assert np.array_equal(want['input'], g['input'].astype(np.float32))
        assert np.array_equal(want['target'], g['target'].astype(np.float32))


def test_status_bits_flag_only_their_case(lib):
    m, g = ec.load_golden()[2]
    case = ec.status_bits_call()
    sched, jump, stuck, off, late, _ = case['schedules']
    assert [len(x) for x in case['schedules']] == [len(sched)] * 6
    out = call(lib, g['grid'], np.stack([g['goal']] * 6), [sched, jump, stuck, off, late, sched])
    ec.assert_call_outputs(out, case, np.nan)
    assert out['status'][0] == 0 and out['status'][5] == 0
    assert out['status'][1] == BAD_MOVE
    assert out['status'][2] & BAD_STATE and out['status'][3] & BAD_STATE
    assert out['status'][4] & BAD_MOVE
    T = len(sched)
    for c in (0, 5):                                    # the legal cases next to them: untouched by their neighbours
        view = {k: v[c * T:(c + 1) * T] if k in ('obs', 'S', 'S64', 'target', 'step_info') else v[c:c + 1]
                for k, v in out.items() if k != 'start'}
        view['start'] = np.array([0, T])
        assert_case_equals_golden(view, 0, m, g)
    for c in (1, 2, 3, 4):                              # a flagged case is not built
        assert np.isnan(out['obs'][c * T:(c + 1) * T]).all() and np.isnan(out['S'][c * T:(c + 1) * T]).all()


def test_argument_errors(lib):
    m, g = ec.load_golden()[7]
    ok = dict(grids=g['grid'], goals=g['goal'][None], schedules=[g['schedule']])
    call(lib, **ok)
    one = dict(grids=g['grid'], goals=g['goal'][None, :1], schedules=[g['schedule'][:, :1]])
    out = call(lib, expect=ERR_UNSUPPORTED, **one)
    assert np.isnan(out['obs']).all() and (out['status'] == -1).all()          # nothing enqueued
    big = dict(grids=g['grid'], goals=np.zeros((1, 129, 2), np.int32), schedules=[np.zeros((2, 129, 2), np.int32)])
    call(lib, expect=ERR_ARG, **big)
    call(lib, radius0=0.0, expect=ERR_ARG, **ok)
    call(lib, radius0=float('nan'), expect=ERR_ARG, **ok)
    huge = dict(grids=np.zeros((300, 300), np.uint8), goals=g['goal'][None], schedules=[g['schedule']])
    out = call(lib, expect=ERR_UNSUPPORTED, **huge)                            # the map does not fit the LDS grid
    assert np.isnan(out['obs']).all()
    assert lib.gnnpp_schedule_samples(None, None) == ERR_ARG
    s = ScheduleStruct()
    assert lib.gnnpp_schedule_samples(ctypes.byref(s), None) == ERR_ARG        # NULL pointers
    assert lib.gnnpp_version() == 330


def test_large_team_and_map_without_stage(lib):
    """128 agents (both halves of every lane pair) and a 230 x 230 map: the occupancy grid leaves no room for the LDS
    output stage, the rows go straight to memory."""
    full, wide = ec.calls_without_stage()
    for case in (full, wide):
        out = call(lib, case['grids'], case['goals'], case['schedules'])
        ec.assert_call_outputs(out, case, np.nan)
        want = ec.call_wants(case)[0]
        assert out['status'][0] == 0 and out['radius'][0] == want['radius'] and out['growth'][0] == want['growth']
        assert np.array_equal(out['obs'], want['input']) and np.array_equal(out['S64'], want['GSO'])
        assert np.array_equal(out['target'], want['target'])
    assert full['goals'].shape[1] == 128 and wide['grids'].shape == (230, 230)


def test_radii_that_share_an_integer_bound(lib):
    """radius0 = 1.0: growth counts the trips whose integer threshold equals the one before (nothing is rebuilt there)."""
    case = ec.repeated_bounds_call()
    out = call(lib, case['grids'], case['goals'], case['schedules'], radius0=case['radius0'])
    ec.assert_call_outputs(out, case, np.nan)
    assert (out['step_info'] & 0xffff).tolist() == [12, 12, 8, 8]


def run_case(lib, case, **kw):
    out = call(lib, case['grids'], case['goals'], case['schedules'], radius0=case['radius0'], fp64=case['fp64'], **kw)
    ec.assert_call_outputs(dict(out, S64=out['S64'] if case['fp64'] else None), case, np.nan)
    return out


@pytest.mark.parametrize('N', [2, 128])
@pytest.mark.parametrize('H,W', ec.thin_shapes(ec.ONE_WAVE_SIDE))
def test_map_limit_of_16384_cells_a_side(lib, H, W, N):
    """A walk with a map per case and the team on the two ends of the strip, on the longest map the launcher takes."""
    case = ec.one_wave_limit_call(H, W, N)
    out = run_case(lib, case)
    want = ec.call_wants(case)[2]
    assert (out['growth'][2], out['radius'][2]) == ec.growth_to_span(5.0, ec.ONE_WAVE_SIDE - N + 1) == \
        (want['growth'], want['radius'])


@pytest.mark.parametrize('H,W', ec.thin_shapes(ec.ONE_WAVE_SIDE + 1))
def test_one_cell_beyond_the_map_limit_is_refused(lib, H, W):
    case = ec.beyond_one_wave_limit_call(H, W)
    out = call(lib, case['grids'], case['goals'], case['schedules'], expect=ERR_UNSUPPORTED)
    assert all(np.isnan(out[k]).all() for k in ('obs', 'S', 'S64', 'target', 'radius'))
    assert (out['status'] == -1).all() and (out['growth'] == -1).all() and (out['step_info'] == -1).all()


def test_python_side_names_the_call_that_refused_the_map(lib, monkeypatch):
    """expert.enqueue_schedule_samples, which samples_from_schedules goes through, on the emulated library with host
    tensors: the project's error, naming the call and "not supported", and nothing else."""
    import torch
    from gnn_pathplanning_amd import _native, expert
    case = ec.beyond_one_wave_limit_call(1, ec.ONE_WAVE_SIDE + 1)
    monkeypatch.setattr(_native, 'lib', lambda: lib)
    monkeypatch.setattr(_native, 'require_gpu', lambda *t: torch.device('cpu'))
    monkeypatch.setattr(_native, 'stream_ptr', lambda dev: None)
    monkeypatch.setattr(_native.device_guard, '__enter__', lambda self: self)

    def enqueue(case):
        bounds = np.cumsum([0] + [len(s) for s in case['schedules']]).tolist()
        (C, N), T = case['goals'].shape[:2], bounds[-1]
        out = expert.ScheduleSamples(
            input=torch.full((T, N, 3, 11, 11), -7.0), GSO=torch.full((T, N, N), -7.0), GSO64=None,
            target=torch.full((T, N, 5), -7.0), radius=torch.full((C,), -7.0, dtype=torch.float64),
            growth=torch.full((C,), -7, dtype=torch.int32), status=torch.full((C,), -7, dtype=torch.int32),
            step_growth=torch.full((T,), -7, dtype=torch.int32))
        expert.enqueue_schedule_samples(torch.from_numpy(case['grids']), torch.from_numpy(case['goals']),
                                        torch.from_numpy(np.concatenate(case['schedules'])),
                                        torch.tensor(bounds, dtype=torch.int32), out)
        return out

    with pytest.raises(_native.GnnppError, match=r'^gnnpp_schedule_samples failed: .*not supported.*\(code -2\)$'):
        enqueue(case)
    limit = ec.one_wave_limit_call(1, ec.ONE_WAVE_SIDE, 2)              # one cell shorter: the same path builds it
    out = enqueue(limit)
    assert out.status.tolist() == [0, 0, 0] and out.growth.tolist() == [w['growth'] for w in ec.call_wants(limit)]


@pytest.mark.parametrize('radius0', ec.HUGE_RADII, ids=repr)
def test_radius_beyond_every_distance(lib, radius0):
    """Three agents on 1 x 40: status 0, growth 0, radius = radius0 bit for bit, every pair an edge."""
    tiny, _ = ec.huge_radius_calls(radius0)
    out = run_case(lib, tiny)
    assert out['status'][0] == 0 and out['growth'][0] == 0 and (out['step_info'] == 0).all()
    assert out['radius'].tobytes() == np.array([radius0]).tobytes()
    assert ((out['S64'] != 0) == ~np.eye(3, dtype=bool)).all() and ((out['S'] != 0) == ~np.eye(3, dtype=bool)).all()


def test_teams_at_the_second_agent_per_lane(lib):
    for case in ec.lane_boundary_calls():
        out = call(lib, case['grids'], case['goals'], case['schedules'])
        ec.assert_call_outputs(out, case, np.nan)
