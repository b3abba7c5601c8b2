"""CPU: gnnpp_mapf_team_solve (csrc/mapf_team_kernels.hip), compiled unmodified for the host emulation, against the
sequential numpy restatement of the contract (tests/mapf_cases.py): equality of every output element.  The shapes are
small (a lane-accurate workgroup is slow) but cross every boundary of the layout: teams beyond 128 agents, rows of two
and three words (W = 65, 128, 129), more than one wave of rows (H = 65 .. 70), and the one-wave call's own sizes, where
the two entry points must write the same bytes.  The cases are built in mapf_cases.TEAM and mapf_cases.BOTH, with the
facts the yardstick's answer must show; tests/test_gpu_mapf_cases.py runs the same ones on the device."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mapf_cases as mc  # noqa: E402
from gnn_pathplanning_amd._native import ERR_ARG, ERR_UNSUPPORTED, MapfStruct  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')

POISON = mc.POISON
KEYS = ('status', 'restart', 'makespan', 'flowtime', 'failing', 'arrival', 'schedule')


@pytest.fixture(scope='module')
def lib():
    import emu_lib
    return emu_lib.load()


def one_slot_bytes(lib, C, R, H, W, T):
    """The summary and exactly one slot: the smallest workspace the call accepts."""
    slot = (T + 1) * 6 * H * ((W + 63) // 64) * 8
    full = lib.gnnpp_mapf_team_workspace_bytes(C, R, H, W, T)
    return full - (min(C * R, 256) - 1) * slot


def call(lib, grids, starts, goals, T, orders=None, expect=0, ws_bytes=None, team=True, poison_ws=False):
    """One call on host arrays; outputs start out poisoned, so an element the call does not write cannot pass for one
    it wrote.  ws_bytes: what the call is told (the buffer is never smaller than that)."""
    grid = np.ascontiguousarray(grids, dtype=np.uint8)
    start = np.ascontiguousarray(starts, dtype=np.int32)
    goal = np.ascontiguousarray(goals, dtype=np.int32)
    C, N = start.shape[:2]
    order = None if orders is None else np.ascontiguousarray(orders, dtype=np.int32)
    R = 1 if order is None else order.shape[1]
    H, W = grid.shape[-2:]
    if team:
        need = lib.gnnpp_mapf_team_workspace_bytes(C, R, min(H, 256), min(W, 256), max(0, min(T, 2048)))
    else:
        need = lib.gnnpp_mapf_workspace_bytes(C, R, H, T)
    told = need if ws_bytes is None else ws_bytes
    ws = np.full(max(need, told, 8) // 8 + 1, 0x5a5a5a5a5a5a5a5a if poison_ws else 0, np.uint64)
    out = {'schedule': np.full((C, T + 1 if T >= 0 else 1, N, 2), POISON, np.int32),
           'arrival': np.full((C, N), POISON, np.int32)}
    for k in ('makespan', 'flowtime', 'status', 'failing', 'restart'):
        out[k] = np.full(C, POISON, np.int32)
    m = MapfStruct()
    m.grid, m.grid_batched, m.start, m.goal = grid.ctypes.data, int(grid.ndim == 3), start.ctypes.data, goal.ctypes.data
    m.order = order.ctypes.data if order is not None else None
    m.C, m.N, m.H, m.W, m.R, m.T_max = C, N, H, W, R, T
    for k in out:
        setattr(m, k, out[k].ctypes.data)
    m.workspace, m.workspace_bytes = ws.ctypes.data, told
    fn = lib.gnnpp_mapf_team_solve if team else lib.gnnpp_mapf_solve
    assert fn(ctypes.byref(m), None) == expect
    return out


def assert_same_bytes(a, b):
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def run_case(lib, name, shared=False, ws_bytes=None):
    """One call of a case of mapf_cases.TEAM: every output of every case equal to the yardstick's, the case's facts
    asserted on the yardstick's answer (mc.wants_of).  shared: the map of case 0 passed once, for the whole call."""
    case = mc.TEAM[name]()
    out = call(lib, case['grid'][0] if shared else case['grid'], case['starts'], case['goals'], case['T'], case['orders'],
               ws_bytes=ws_bytes, poison_ws=case['poison_ws'])
    wants = mc.wants_of(case)
    mc.assert_outputs_equal(out, wants)
    return out, wants


def test_more_than_128_agents_on_one_word_rows(lib):
    run_case(lib, 'more_than_128_agents_on_one_word_rows')


@pytest.mark.parametrize('W', [65, 128, 129])
def test_random_cases_on_rows_of_several_words(lib, W):
    run_case(lib, 'random_cases_on_rows_of_several_words_W%d' % W)


@pytest.mark.parametrize('W', [65, 128, 129])
def test_corridor_forces_the_crossing_both_ways(lib, W):
    run_case(lib, 'corridor_forces_the_crossing_both_ways_W%d' % W)


def test_swap_refused_across_the_word_boundary(lib):
    run_case(lib, 'swap_refused_across_the_word_boundary')
    run_case(lib, 'no_way_round_on_the_1x66_strip')


@pytest.mark.parametrize('H,W', [(65, 6), (70, 9), (66, 65)])
def test_more_than_one_wave_of_rows(lib, H, W):
    """The vertical exchange across waves: a wall with one door between rows 63 and 64."""
    run_case(lib, 'more_than_one_wave_of_rows_%dx%d' % (H, W))


def test_random_cases_on_tall_maps(lib):
    run_case(lib, 'random_cases_on_tall_maps')


def test_several_waves_of_rows_of_several_words(lib):
    """70 x 130: 210 threads in four waves, rows of three words, 140 agents."""
    run_case(lib, 'several_waves_of_rows_of_several_words')


def test_given_orders_with_a_failing_restart(lib):
    run_case(lib, 'given_orders_with_a_tie')
    run_case(lib, 'failing_restart_on_2x67')


def test_crowded_cases_solved_and_failing(lib):
    run_case(lib, 'crowded_cases_solved_and_failing')


def test_bad_cases_flag_only_themselves(lib):
    out, _ = run_case(lib, 'bad_cases_flag_only_themselves')
    assert out['status'][0] == 0 and out['status'][-1] == 0


def test_batched_grid_next_to_shared_grid(lib):
    shared, _ = run_case(lib, 'batched_grid_next_to_shared_grid', shared=True)
    batched, _ = run_case(lib, 'batched_grid_next_to_shared_grid')
    assert_same_bytes(shared, batched)


def test_same_bytes_as_the_one_wave_call(lib):
    """Every case both entry points accept: all outputs byte-equal (random, crowded with failures, restarts with a bad
    order, the widest one-word map, 128 agents, the unplanned tail behind a failing agent 70 of 72)."""
    for name in ('random_10x10', 'crowded_with_failures', 'restarts_with_a_bad_order', 'widest_one_word_map',
                 '128_agents_on_16x16', 'unplanned_tail_past_one_wave_of_agents'):
        case = mc.BOTH[name]()
        args = (lib, case['grid'], case['starts'], case['goals'], case['T'], case['orders'])
        a = call(*args, team=False)
        b = call(*args, team=True, poison_ws=True)
        assert_same_bytes(a, b)
        mc.assert_outputs_equal(a, mc.wants_of(case))


def test_outputs_do_not_depend_on_the_slot_count(lib):
    name = 'outputs_do_not_depend_on_the_slot_count'
    full, _ = run_case(lib, name)
    one = one_slot_bytes(lib, 5, 2, 4, 66, 60)
    assert one < lib.gnnpp_mapf_team_workspace_bytes(5, 2, 4, 66, 60)
    single, _ = run_case(lib, name, ws_bytes=one)
    three, _ = run_case(lib, name, ws_bytes=one + 2 * (61 * 6 * 4 * 2 * 8) + 100)
    assert_same_bytes(full, single)
    assert_same_bytes(full, three)


def test_zero_horizon_and_single_agent(lib):
    out, _ = run_case(lib, 'zero_horizon_agent_on_its_goal')
    assert out['status'][0] == 0 and out['arrival'][0, 0] == 0
    out, _ = run_case(lib, 'zero_horizon_agent_off_its_goal')
    assert out['status'][0] == mc.NO_PATH


def test_argument_errors(lib):
    grid = np.zeros((4, 4), np.uint8)
    s, g = np.array([[[0, 0], [1, 1]]]), np.array([[[3, 3], [2, 2]]])
    assert call(lib, grid, s, g, 8)['status'][0] == 0
    one = one_slot_bytes(lib, 1, 1, 4, 4, 8)
    for kw in (dict(T=-1), dict(T=2049), dict(ws_bytes=0), dict(ws_bytes=one - 1)):
        out = call(lib, grid, s, g, kw.pop('T', 8), expect=ERR_ARG, **kw)
        for k in KEYS:
            assert (out[k] == POISON).all(), k                  # nothing enqueued
    for shape in ((257, 4), (4, 257)):
        out = call(lib, np.zeros(shape, np.uint8), s, g, 8, expect=ERR_UNSUPPORTED)
        for k in KEYS:
            assert (out[k] == POISON).all(), k
    many = np.zeros((1, 1025, 2), np.int32)
    out = call(lib, np.zeros((64, 64), np.uint8), many, many, 4, expect=ERR_ARG)
    assert (out['status'] == POISON).all() and (out['schedule'] == POISON).all()
    # N and T_max are refused before the map size is looked at
    call(lib, np.zeros((257, 4), np.uint8), many, many, 4, expect=ERR_ARG)
    call(lib, np.zeros((257, 4), np.uint8), s, g, 2049, expect=ERR_ARG)
    # orders without R, NULLs
    assert lib.gnnpp_mapf_team_solve(None, None) == ERR_ARG
    assert lib.gnnpp_mapf_team_solve(ctypes.byref(MapfStruct()), None) == ERR_ARG
    W = lib.gnnpp_mapf_team_workspace_bytes
    assert W(1, 1, 4, 4, 8) > 0 and W(1, 1, 256, 256, 2048) > 0
    for bad in ((0, 1, 4, 4, 8), (1, 0, 4, 4, 8), (1, 1, 257, 4, 8), (1, 1, 4, 257, 8), (1, 1, 0, 4, 8), (1, 1, 4, 0, 8),
                (1, 1, 4, 4, -1), (1, 1, 4, 4, 2049), (1 << 20, 1 << 12, 4, 4, 8)):
        assert W(*bad) == 0, bad
    # the full size is for min(C R, 256) slots
    slot = 9 * 6 * 4 * 8
    assert W(300, 1, 4, 4, 8) - W(256, 1, 4, 4, 8) == (300 * 16 + 255) // 256 * 256 - 256 * 16
    assert W(2, 1, 4, 4, 8) - W(1, 1, 4, 4, 8) == slot
