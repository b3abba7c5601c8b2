"""CPU: gnnpp_mapf_solve (csrc/mapf_kernels.hip), compiled unmodified for the host emulation, against the sequential
numpy restatement of the contract (tests/mapf_cases.py): equality of every output element, on small random cases and
on hand-built edge cases.  The cases are built in mapf_cases.ONE_WAVE, with the facts the yardstick's answer must show;
tests/test_gpu_mapf_cases.py runs the same ones on the device."""
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


@pytest.fixture(scope='module')
def lib():
    import emu_lib
    return emu_lib.load()


def call(lib, grids, starts, goals, T, orders=None, expect=0, ws_bytes=None):
    """One gnnpp_mapf_solve call on host arrays; outputs start out poisoned, so an element the call does not write
    cannot pass for one it wrote."""
    grid = np.ascontiguousarray(grids, dtype=np.uint8)
    start = np.ascontiguousarray(starts, dtype=np.int32)
    goal = np.ascontiguousarray(goals, dtype=np.int32)
    C, N = start.shape[:2]
    order = None if orders is None else np.ascontiguousarray(orders, dtype=np.int32)
    R = 1 if order is None else order.shape[1]
    H, W = grid.shape[-2:]
    need = lib.gnnpp_mapf_workspace_bytes(C, R, min(H, 64), T)
    ws = np.zeros(max(need, 8) // 8 + 1, np.uint64)
    out = {'schedule': np.full((C, T + 1, N, 2), POISON, np.int32), 'arrival': np.full((C, N), POISON, np.int32)}
    for k in ('makespan', 'flowtime', 'status', 'failing', 'restart'):
        out[k] = np.full(C, POISON, np.int32)
    m = MapfStruct()
    m.grid, m.grid_batched, m.start, m.goal = grid.ctypes.data, int(grid.ndim == 3), start.ctypes.data, goal.ctypes.data
    m.order = order.ctypes.data if order is not None else None
    m.C, m.N, m.H, m.W, m.R, m.T_max = C, N, H, W, R, T
    for k in out:
        setattr(m, k, out[k].ctypes.data)
    m.workspace, m.workspace_bytes = ws.ctypes.data, need if ws_bytes is None else ws_bytes
    assert lib.gnnpp_mapf_solve(ctypes.byref(m), None) == expect
    return out


def run_case(lib, name, shared=False):
    """One call of a case of mapf_cases.ONE_WAVE: every output of every case equal to the yardstick's, the case's facts
    asserted on the yardstick's answer (mc.wants_of).  shared: the map of case 0 passed once, for the whole call."""
    case = mc.ONE_WAVE[name]()
    out = call(lib, case['grid'][0] if shared else case['grid'], case['starts'], case['goals'], case['T'], case['orders'])
    wants = mc.wants_of(case)
    mc.assert_outputs_equal(out, wants)
    return out, wants


def test_random_cases_equal_the_restatement(lib):
    run_case(lib, 'random_10x10')


def test_crowded_cases_with_failures(lib):
    """Dense maps and many agents: some cases end with NO_PATH, the agents after the failing one left unplanned."""
    run_case(lib, 'crowded_cases_with_failures')


def test_agent_on_its_goal_steps_aside_and_comes_back(lib):
    run_case(lib, 'agent_on_its_goal_steps_aside_and_comes_back')


def test_target_conflict(lib):
    run_case(lib, 'target_conflict')


def test_swap_is_not_a_shortcut(lib):
    run_case(lib, 'swap_is_not_a_shortcut')


def test_walled_in_agent_stops_the_plan(lib):
    out, _ = run_case(lib, 'walled_in_agent_stops_the_plan')
    assert out['makespan'][0] == -1 and out['flowtime'][0] == -1


def test_bad_cases_flag_only_themselves(lib):
    out, _ = run_case(lib, 'bad_cases_flag_only_themselves')
    assert out['status'][0] == 0 and out['status'][-1] == 0


@pytest.mark.parametrize('H,W', [(64, 64), (5, 64), (64, 5)])
def test_widest_and_tallest_maps(lib, H, W):
    """Bit 63 of a row and lane 63 of the wave."""
    run_case(lib, 'widest_and_tallest_maps_%dx%d' % (H, W))


def test_non_square_random_maps(lib):
    run_case(lib, 'non_square_7x13')
    run_case(lib, 'non_square_13x7')


def test_restarts_pick_the_best_and_ties_the_lowest(lib):
    out, _ = run_case(lib, 'restarts_pick_the_best_and_ties_the_lowest')
    assert out['restart'][1] != 2
    run_case(lib, 'only_the_reversed_order_solves')


def test_batched_grid_next_to_shared_grid(lib):
    shared, _ = run_case(lib, 'batched_grid_next_to_shared_grid', shared=True)
    batched, _ = run_case(lib, 'batched_grid_next_to_shared_grid')
    for k in shared:
        assert np.array_equal(shared[k], batched[k]), k


def test_argument_errors(lib):
    grid = np.zeros((4, 4), np.uint8)
    s, g = np.array([[[0, 0], [1, 1]]]), np.array([[[3, 3], [2, 2]]])
    call(lib, grid, s, g, 8)
    for kw in (dict(T=-1), dict(T=1025), dict(orders=None, ws_bytes=0)):
        out = call(lib, grid, s, g, kw.pop('T', 8), expect=ERR_ARG, **kw)
        assert (out['status'] == POISON).all()                 # nothing enqueued
    big = np.zeros((65, 4), np.uint8)
    out = call(lib, big, s, g, 8, expect=ERR_UNSUPPORTED)
    assert (out['status'] == POISON).all() and (out['schedule'] == POISON).all()
    many = np.zeros((1, 129, 2), np.int32)
    call(lib, np.zeros((64, 64), np.uint8), many, many, 4, expect=ERR_ARG)
    assert lib.gnnpp_mapf_solve(None, None) == ERR_ARG
    assert lib.gnnpp_mapf_solve(ctypes.byref(MapfStruct()), None) == ERR_ARG
    assert lib.gnnpp_mapf_workspace_bytes(1, 1, 65, 8) == 0 and lib.gnnpp_mapf_workspace_bytes(1, 1, 4, 8) > 0
