"""CPU: gnnpp_schedule_team_samples (csrc/expert_team_kernels.hip), compiled unmodified for the host emulation, against
what the REAL reference transformer made of teams of 130 ... 1024 agents (tests/golden/expert_schedules_team.npz),
against gnnpp_schedule_samples on everything both accept, and against the sequential restatement
tests/expert_cases.py::reference_samples on random cases: equality, every element."""
import ctypes
import json
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

OUTPUTS = ('obs', 'S', 'S64', 'target', 'radius', 'growth', 'status', 'step_info')


def load_team_golden():
    """[(meta, dict of arrays)] of tests/golden/expert_schedules_team.npz (tools/gen_expert_golden_team.py)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'expert_schedules_team.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    keys = ('grid', 'goal', 'schedule', 'input', 'GSO', 'target')
    return [(m, {k: z['c%d_%s' % (ci, k)] for k in keys}) for ci, m in enumerate(meta)]


@pytest.fixture(scope='module')
def lib():
    import emu_lib
    return emu_lib.load()


def call(lib, grids, goals, schedules, radius0=5.0, fp64=True, expect=0, poison=np.nan, team=True, workspace='exact',
         misalign=False):
    """One call on host arrays; outputs start out poisoned, so an element the call does not write cannot pass for one
    it wrote.  team=False: gnnpp_schedule_samples.  workspace: 'exact' (what the library asks for), 'short' (8 bytes
    less) or None.  misalign: S and S64 start 4 / 8 bytes past a 16-byte boundary (the scalar store path)."""
    grid = np.ascontiguousarray(grids, dtype=np.uint8)
    goal = np.ascontiguousarray(goals, dtype=np.int32)
    C, N = goal.shape[:2]
    pos = np.ascontiguousarray(np.concatenate(schedules, 0), dtype=np.int32)
    start = np.ascontiguousarray(np.cumsum([0] + [len(s) for s in schedules]), dtype=np.int32)
    T = int(start[-1])

    def graph(dtype):
        size = np.dtype(dtype).itemsize
        raw = np.full(T * N * N + 32 // size, poison, dtype)
        off = (-raw.ctypes.data % 16) // size + (1 if misalign else 0)
        return raw[off:off + T * N * N].reshape(T, N, N)

    out = {'obs': np.full((T, N, 3, 11, 11), poison, np.float32), 'S': graph(np.float32), 'S64': graph(np.float64),
           'target': np.full((T, N, 5), poison, np.float32),
           'radius': np.full(C, poison, np.float64), 'growth': np.full(C, -1, np.int32),
           'status': np.full(C, -1, np.int32), 'step_info': np.full(T, -1, np.int32), 'start': start}
    assert (out['S'].ctypes.data % 16 != 0) == misalign and (out['S64'].ctypes.data % 16 != 0) == misalign
    s = ScheduleStruct()
    s.grid, s.grid_batched, s.goal, s.pos = grid.ctypes.data, int(grid.ndim == 3), goal.ctypes.data, pos.ctypes.data
    s.case_start, s.C, s.N, s.H, s.W, s.T_total = start.ctypes.data, C, N, grid.shape[-2], grid.shape[-1], T
    s.radius0 = radius0
    s.obs, s.S, s.target = out['obs'].ctypes.data, out['S'].ctypes.data, out['target'].ctypes.data
    s.S64 = out['S64'].ctypes.data if fp64 else None
    s.radius, s.growth, s.status = out['radius'].ctypes.data, out['growth'].ctypes.data, out['status'].ctypes.data
    s.step_info = out['step_info'].ctypes.data
    if not team:
        assert lib.gnnpp_schedule_samples(ctypes.byref(s), None) == expect
        return out
    need = lib.gnnpp_schedule_team_workspace_bytes(N, T)
    ws = np.full(max(need, 8) // 8 + 1, poison, np.float64)
    nbytes = {'exact': need, 'short': need - 8, None: need}[workspace]
    assert lib.gnnpp_schedule_team_samples(ctypes.byref(s), ws.ctypes.data if workspace else None, nbytes, None) == expect
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


def assert_same_bytes(x, y):
    for k in OUTPUTS:
        assert x[k].tobytes() == y[k].tobytes(), k       # (NaN poison included: the same elements are left unwritten)


def assert_case_equals_restatement(out, c, grid, goal, sched, fp64=True):
    want = ec.reference_samples(grid, goal, sched)
    a, b = int(out['start'][c]), int(out['start'][c + 1])
    assert out['status'][c] == 0 and out['radius'][c] == want['radius'] and out['growth'][c] == want['growth']
    assert np.array_equal(out['obs'][a:b], want['input']) and np.array_equal(out['target'][a:b], want['target'])
    assert np.array_equal(out['S'][a:b], want['GSO'].astype(np.float32))
    if fp64:
        assert np.array_equal(out['S64'][a:b], want['GSO'])
    return want


def test_team_golden_file_keeps_what_it_must():
    gold = load_team_golden()
    sizes = [m['N'] for m, _ in gold]
    assert 1024 in sizes and any(n % 64 for n in sizes) and any(n % 4 for n in sizes) and min(sizes) > 128
    assert any(m['growth'] == 0 for m, _ in gold) and any(m['growth'] >= 10 for m, _ in gold)


@pytest.mark.parametrize('ci', range(5))
def test_team_golden_case(lib, ci):
    m, g = load_team_golden()[ci]
    out = call(lib, g['grid'], g['goal'][None], [g['schedule']])
    assert_case_equals_golden(out, 0, m, g)


@pytest.mark.parametrize('ci', range(8))
def test_small_team_golden_case_same_bytes_as_one_wave_call(lib, ci):
    m, g = ec.load_golden()[ci]
    out = call(lib, g['grid'], g['goal'][None], [g['schedule']])
    assert_case_equals_golden(out, 0, m, g)
    assert_same_bytes(out, call(lib, g['grid'], g['goal'][None], [g['schedule']], team=False))


def test_radii_that_share_an_integer_bound_same_bytes_as_one_wave_call(lib):
    """radius0 = 1.0: growth counts the trips whose integer threshold equals the one before, in both calls."""
    case = ec.repeated_bounds_call()
    out = call(lib, case['grids'], case['goals'], case['schedules'], radius0=case['radius0'])
    ec.assert_call_outputs(out, case, np.nan)
    assert (out['step_info'] & 0xffff).tolist() == [12, 12, 8, 8]
    assert_same_bytes(out, call(lib, case['grids'], case['goals'], case['schedules'], radius0=case['radius0'], team=False))


def test_ragged_cases_and_batched_maps_same_bytes_as_one_wave_call(lib):
    """Cases of 20, 7 and 3 steps with a map each (24 agents: 16-byte stores; 10 agents: 4-byte stores)."""
    for ci in (4, 0):
        m, g = ec.load_golden()[ci]
        for fp64 in (False, True):
            case = ec.ragged_call_with_a_map_per_case(ci, fp64)
            parts, goals, grids = case['schedules'], case['goals'], case['grids']
            out = call(lib, grids, np.stack(goals), parts, fp64=fp64)
            ec.assert_call_outputs(dict(out, S64=out['S64'] if fp64 else None), case, np.nan)
            assert_same_bytes(out, call(lib, grids, np.stack(goals), parts, fp64=fp64, team=False))
            assert out['status'].tolist() == [0, 0, 0]
            if not fp64:
                assert np.isnan(out['S64']).all()
        assert_case_equals_golden(out, 0, m, g)
        for c in (1, 2):
            assert_case_equals_restatement(out, c, grids[c], goals[c], parts[c])


def test_unaligned_graph_outputs_give_the_same_bytes(lib):
    """S / S64 off the 16-byte boundary take the 4-byte store path: same values."""
    m, g = load_team_golden()[0]
    out = call(lib, g['grid'], g['goal'][None], [g['schedule']], misalign=True)
    assert_case_equals_golden(out, 0, m, g)
    case = ec.ragged_call_with_a_map_per_case(4, True)  # (24 agents: the rows are 16-byte multiples)
    out = call(lib, case['grids'], case['goals'], case['schedules'], misalign=True)
    ec.assert_call_outputs(out, case, np.nan)
    assert_same_bytes(out, call(lib, case['grids'], case['goals'], case['schedules']))


@pytest.mark.parametrize('N,side,steps', [(129, 40, 3), (130, 60, 3), (191, 50, 2), (512, 90, 2)])
def test_random_case_against_restatement(lib, N, side, steps):
    rng = np.random.default_rng(1000 + N)
    grid, goal, paths = ec.random_case(rng, N, side, side, density=0.1, max_steps=steps)
    sched = ec.schedule_of(paths, goal)
    out = call(lib, grid, goal[None], [sched])
    assert_case_equals_restatement(out, 0, grid, goal, sched)


def test_cases_of_different_growths_in_one_call_without_fp64_copy(lib):
    """A team spread over the map and one kept in a box share a call: each gets its own radius."""
    case = ec.team_growths_call()
    scheds = case['schedules']
    out = call(lib, case['grids'], case['goals'], scheds, fp64=False)
    wants = [assert_case_equals_restatement(out, c, case['grids'][c], case['goals'][c], scheds[c], fp64=False)
             for c in (0, 1)]
    assert wants[0]['growth'] != wants[1]['growth']
    assert np.isnan(out['S64']).all()
    for c in (0, 1):                                    # step_info: every step's own growths, the case's the largest
        a, b = int(out['start'][c]), int(out['start'][c + 1])
        own = [ec.schedule_gso(scheds[c][t:t + 1])[2] for t in range(b - a)]
        assert out['step_info'][a:b].tolist() == own


def test_status_bits_flag_only_their_case(lib):
    case = ec.team_status_bits_call()
    grid, goal = case['grids'], case['goals'][0]
    sched, jump, stuck, off, off2, _ = case['schedules']
    out = call(lib, grid, np.stack([goal] * 6), [sched, jump, stuck, off, off2, sched])
    ec.assert_call_outputs(out, case, np.nan, untouched=('obs', 'S', 'S64', 'target'))
    assert out['status'][0] == 0 and out['status'][5] == 0
    assert out['status'][1] == BAD_MOVE
    assert out['status'][2] & BAD_STATE and out['status'][3] & BAD_STATE and out['status'][4] & BAD_STATE
    assert out['step_info'][3 * 4] & 0xffff == 0        # no graph search for a step with a state off the map
    alone = call(lib, grid, goal[None], [sched])
    assert_case_equals_restatement(alone, 0, grid, goal, sched)
    T = len(sched)
    for c in (0, 5):                                    # the legal cases next to them: untouched by their neighbours
        for k in ('obs', 'S', 'S64', 'target', 'step_info'):
            assert np.array_equal(out[k][c * T:(c + 1) * T], alone[k]), k
        assert out['radius'][c] == alone['radius'][0] and out['growth'][c] == alone['growth'][0]
    for c in (1, 2, 3, 4):                              # a flagged case is not built
        for k in ('obs', 'S', 'S64', 'target'):
            assert np.isnan(out[k][c * T:(c + 1) * T]).all(), k


def run_case(lib, case, untouched=('obs', 'S'), **kw):
    """A call of tests/expert_cases.py on poisoned host arrays, against the restatement."""
    out = call(lib, case['grids'], case['goals'], case['schedules'], radius0=case['radius0'], fp64=case['fp64'], **kw)
    ec.assert_call_outputs(dict(out, S64=out['S64'] if case['fp64'] else None), case, np.nan, untouched)
    if not case['fp64'] and kw.get('team', True):
        assert np.isnan(out['S64']).all()
    return out


def per_step_growths(case, c):
    return [ec.schedule_gso(case['schedules'][c][t:t + 1], case['radius0'])[2] for t in range(len(case['schedules'][c]))]


# ---- thin maps: 1 x 65 536 and 65 536 x 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', ec.thin_shapes(ec.THIN_SIDE))
def test_thin_map_two_agents_on_both_ends(lib, H, W):
    """100 growths; the bounds pass 2^31 and end in the 0xffffffff clamp."""
    out = run_case(lib, ec.both_ends_call(H, W))
    assert out['growth'][0] == 100 and out['radius'][0] == 68903.06169911187
    assert (out['step_info'] & 0xffff).tolist() == [100, 100]


@pytest.mark.parametrize('H,W', ec.thin_shapes(ec.THIN_SIDE))
def test_thin_map_two_halves_on_the_ends(lib, H, W):
    """129 agents: the halves meet only at the final growth, at every step on its own."""
    case = ec.two_ends_call(H, W, 129)
    out = run_case(lib, case)
    assert out['step_info'].tolist() == per_step_growths(case, 0) == [ec.call_wants(case)[0]['growth']] * 2


@pytest.mark.parametrize('H,W,fp64', [(1, ec.THIN_SIDE, True), (ec.THIN_SIDE, 1, False)])
def test_thin_map_two_halves_on_the_ends_full_workgroup(lib, H, W, fp64):
    """1024 agents (the full workgroup), one call with and one without the fp64 copy.  About 6 s each on the host, nearly
    all of it the restatement's 100 radius trips over a 1024 x 1024 distance matrix; the emulated call takes 0.3 s."""
    case = ec.two_ends_call(H, W, 1024, fp64)
    out = run_case(lib, case)
    assert (out['step_info'] & 0xffff).tolist() == [ec.call_wants(case)[0]['growth']] * 2


@pytest.mark.parametrize('H,W', ec.thin_shapes(ec.THIN_SIDE))
def test_thin_map_spread_and_unaligned_graph_outputs(lib, H, W):
    """129 agents 512 cells apart; S / S64 off the 16-byte boundary give the same bytes."""
    case = ec.spread_call(H, W, 129)
    out = run_case(lib, case)
    assert out['step_info'].tolist() == per_step_growths(case, 0)
    assert_same_bytes(out, run_case(lib, case, misalign=True))


@pytest.mark.parametrize('H,W', ec.thin_shapes(ec.THIN_SIDE))
def test_thin_map_walk_with_a_map_per_case(lib, H, W):
    run_case(lib, ec.walk_call(H, W, 129))
    run_case(lib, ec.walk_call(H, W, 129, fp64=False))


def test_thin_map_status_bits_flag_only_their_case(lib):
    case = ec.thin_status_bits_call()
    out = run_case(lib, case, untouched=('obs', 'S', 'S64', 'target'))
    assert out['status'][[0, 4]].tolist() == [0, 0] and out['status'][3] == BAD_MOVE
    assert out['status'][1] & BAD_STATE and out['status'][2] & BAD_STATE
    assert out['step_info'][3 + 1] & 0xffff == 0 and out['step_info'][6] & 0xffff == 0   # no search with a state off the map
    alone = call(lib, case['grids'], case['goals'][:1], case['schedules'][:1])
    T = 3
    for c in (0, 4):                                    # the legal cases: the bytes of the case run alone
        for k in ('obs', 'S', 'S64', 'target', 'step_info'):
            assert out[k][c * T:(c + 1) * T].tobytes() == alone[k].tobytes(), k
        assert out['radius'][c] == alone['radius'][0] and out['growth'][c] == alone['growth'][0]
    for c in (1, 2, 3):                                 # a flagged case is not built
        for k in ('obs', 'S', 'S64', 'target'):
            assert np.isnan(out[k][c * T:(c + 1) * T]).all(), k


# ---- the one-wave call's map limit: a side of 16 384 ----------------------------------------------------------------
@pytest.mark.parametrize('N', [2, 128])
@pytest.mark.parametrize('H,W', ec.thin_shapes(ec.ONE_WAVE_SIDE))
def test_one_wave_map_limit_same_bytes_as_team_call(lib, H, W, N):
    case = ec.one_wave_limit_call(H, W, N)
    assert_same_bytes(run_case(lib, case, team=False), run_case(lib, case))


@pytest.mark.parametrize('H,W', ec.thin_shapes(ec.ONE_WAVE_SIDE + 1))
def test_one_cell_beyond_the_one_wave_map_limit(lib, H, W):
    """The one-wave call refuses the map and writes nothing; the team call builds it."""
    case = ec.beyond_one_wave_limit_call(H, W)
    out = call(lib, case['grids'], case['goals'], case['schedules'], expect=ERR_UNSUPPORTED, team=False)
    assert all(np.isnan(out[k]).all() for k in ('obs', 'S', 'S64', 'target', 'radius'))
    assert (out['status'] == -1).all() and (out['growth'] == -1).all() and (out['step_info'] == -1).all()
    run_case(lib, case)


# ---- radii beyond every distance ------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius0', ec.HUGE_RADII, ids=repr)
def test_radius_beyond_every_distance(lib, radius0):
    """Status 0, growth 0, radius = radius0 bit for bit, every pair an edge.  Before dist2_bound decided r >= 65536 on the
    double, the emulation's (long long)ceil(r * r) gave status 4, growth 65535, radius inf from 3.1e9 on."""
    tiny, thin = ec.huge_radius_calls(radius0)
    for case in (tiny, thin):
        out = run_case(lib, case)
        N = case['goals'].shape[1]
        assert out['status'][0] == 0 and out['growth'][0] == 0 and (out['step_info'] == 0).all()
        assert out['radius'].tobytes() == np.array([radius0]).tobytes()
        assert ((out['S'] != 0) == ~np.eye(N, dtype=bool)).all() and ((out['S64'] != 0) == ~np.eye(N, dtype=bool)).all()
    assert_same_bytes(run_case(lib, tiny, team=False), run_case(lib, tiny))


def test_argument_errors(lib):
    m, g = ec.load_golden()[7]
    ok = dict(grids=g['grid'], goals=g['goal'][None], schedules=[g['schedule']])
    call(lib, **ok)

    def nothing_written(out):
        assert all(np.isnan(out[k]).all() for k in ('obs', 'S', 'S64', 'target', 'radius'))
        assert (out['status'] == -1).all() and (out['growth'] == -1).all() and (out['step_info'] == -1).all()

    one = dict(grids=g['grid'], goals=g['goal'][None, :1], schedules=[g['schedule'][:, :1]])
    nothing_written(call(lib, expect=ERR_UNSUPPORTED, **one))
    full = dict(grids=g['grid'], goals=np.zeros((1, 1024, 2), np.int32), schedules=[np.zeros((1, 1024, 2), np.int32)])
    call(lib, expect=0, **full)                         # (1024 agents are taken: all on one cell, flagged or not)
    big = dict(grids=g['grid'], goals=np.zeros((1, 1025, 2), np.int32), schedules=[np.zeros((1, 1025, 2), np.int32)])
    assert lib.gnnpp_schedule_team_workspace_bytes(1025, 1) == 0
    nothing_written(call(lib, expect=ERR_ARG, **big))
    nothing_written(call(lib, radius0=0.0, expect=ERR_ARG, **ok))
    nothing_written(call(lib, radius0=float('nan'), expect=ERR_ARG, **ok))
    nothing_written(call(lib, radius0=1e300, expect=ERR_ARG, **ok))
    nothing_written(call(lib, workspace='short', expect=ERR_ARG, **ok))
    nothing_written(call(lib, workspace=None, expect=ERR_ARG, **ok))
    limit = dict(grids=np.zeros((256, 256), np.uint8), goals=g['goal'][None], schedules=[g['schedule']])
    assert call(lib, expect=0, **limit)['status'][0] == 0                      # the cell limit itself is taken
    huge = dict(grids=np.zeros((256, 257), np.uint8), goals=g['goal'][None], schedules=[g['schedule']])
    nothing_written(call(lib, expect=ERR_UNSUPPORTED, **huge))                 # the map does not fit the LDS grid
    more_cases = dict(grids=g['grid'], goals=np.stack([g['goal']] * 2), schedules=[g['schedule'][:1]])
    s = ScheduleStruct()
    ws = np.zeros(64, np.float64)
    assert lib.gnnpp_schedule_team_samples(None, ws.ctypes.data, 512, None) == ERR_ARG
    assert lib.gnnpp_schedule_team_samples(ctypes.byref(s), ws.ctypes.data, 512, None) == ERR_ARG      # NULL pointers
    # C > T_total: two cases, one step
    out = {'goal': np.ascontiguousarray(more_cases['goals'], np.int32)}
    grid = np.ascontiguousarray(g['grid'], np.uint8)
    pos = np.ascontiguousarray(g['schedule'][:1], np.int32)
    start = np.array([0, 1, 1], np.int32)
    bufs = [np.full(4096, np.nan, np.float64) for _ in range(8)]
    s.grid, s.goal, s.pos, s.case_start = grid.ctypes.data, out['goal'].ctypes.data, pos.ctypes.data, start.ctypes.data
    s.C, s.N, s.H, s.W, s.T_total, s.radius0 = 2, 2, grid.shape[0], grid.shape[1], 1, 5.0
    (s.obs, s.S, s.S64, s.target, s.radius, s.growth, s.status, s.step_info) = [b.ctypes.data for b in bufs]
    assert lib.gnnpp_schedule_team_samples(ctypes.byref(s), ws.ctypes.data, 512, None) == ERR_ARG
    assert all(np.isnan(b).all() for b in bufs)
    assert lib.gnnpp_schedule_team_workspace_bytes(0, 5) == 0 and lib.gnnpp_schedule_team_workspace_bytes(5, 0) == 0
    assert lib.gnnpp_schedule_team_workspace_bytes(1024, 2100) >= 1024 * 2100 * 8
    big129 = dict(grids=g['grid'], goals=np.zeros((1, 129, 2), np.int32), schedules=[np.zeros((2, 129, 2), np.int32)])
    call(lib, expect=ERR_ARG, team=False, **big129)     # the one-wave call keeps its limit
    assert lib.gnnpp_version() == 330
