"""CPU: gnnpp_casegen (csrc/casegen_kernels.hip), compiled unmodified for the host emulation, against the numpy / queue
yardstick of tests/casegen_cases.py: exact equality of every output element on every named case, on poisoned outputs;
two calls give the same bytes; the documented error codes with nothing written; and the chain at the C level --
gnnpp_casegen -> gnnpp_mapf_distances gives dist >= 1 for every agent of every OK case, and -> gnnpp_mapf_orders ->
gnnpp_mapf_solve on the whole 20 x 20 set equals the solver's yardstick.  tests/test_gpu_casegen.py runs the same cases on
the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import casegen_cases as cc  # noqa: E402
import mapf_cases as mc  # noqa: E402
import mapf_distance_cases as dc  # noqa: E402
from gnn_pathplanning_amd._native import ERR_ARG, ERR_UNSUPPORTED  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')
POISON = cc.POISON


@pytest.fixture(scope='module')
def lib():
    import emu_lib
    return emu_lib.load()


def _ptr(a):
    return None if a is None else a.ctypes.data


def call(lib, C, N, H, W, threshold=0, seed=0, grids=None, expect=0, null=None, dims=None, facts=None):
    """One call on host arrays with poisoned outputs.  null: the name of an output passed as NULL; dims: (C, N, H, W)
    the call is TOLD (the arrays are never smaller than what a call that passes its checks writes)."""
    out = {'grid': np.full((C, H, W), 0x5a, np.uint8), 'start': np.full((C, N, 2), POISON, np.int32),
           'goal': np.full((C, N, 2), POISON, np.int32), 'cells': np.full(C, POISON, np.int32),
           'status': np.full(C, POISON, np.int32)}
    g = None if grids is None else np.ascontiguousarray(grids, dtype=np.uint8)
    tC, tN, tH, tW = dims or (C, N, H, W)
    rc = lib.gnnpp_casegen(_ptr(g), int(g is not None and g.ndim == 3), threshold, seed, tC, tN, tH, tW,
                           *[None if k == null else _ptr(out[k]) for k in cc.OUTPUTS], None)
    assert rc == expect, rc
    return out


def run_case(lib, name):
    case = cc.CASES[name]()
    out = call(lib, **case)
    cc.assert_equal_to_yardstick(name, out)
    cc.assert_properties(dict(out, raw=cc.wants_of(name)['raw']))
    return out


@pytest.mark.parametrize('name', cc.EMU_CASES)
def test_named_cases_equal_the_yardstick(lib, name):
    run_case(lib, name)


def test_two_calls_give_the_same_bytes(lib):
    for name in ('random_40x40', 'many_components_at_density_045', 'team_fills_the_region_next_to_one_agent_too_many'):
        case = cc.CASES[name]()
        a, b = call(lib, **case), call(lib, **case)
        for k in cc.OUTPUTS:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


def test_seed_and_case_index_decide_the_case(lib):
    """Another seed gives other maps; the cases of a call do not depend on how many cases the call has."""
    a = call(lib, 4, 10, 20, 20, cc.threshold_of(0.1), 13)
    b = call(lib, 4, 10, 20, 20, cc.threshold_of(0.1), 14)
    assert a['grid'].tobytes() != b['grid'].tobytes() and a['start'].tobytes() != b['start'].tobytes()
    want = cc.wants_of('random_20x20')
    for k in cc.OUTPUTS:
        assert np.array_equal(a[k], want[k][:4]), k


def test_argument_errors_leave_the_outputs_untouched(lib):
    ok = call(lib, 1, 2, 4, 4)
    assert ok['status'].tolist() == [0] and ok['cells'].tolist() == [16]
    for kw, code in ((dict(dims=(1, 1025, 4, 4)), ERR_ARG), (dict(dims=(1, 2, 257, 4)), ERR_UNSUPPORTED),
                     (dict(dims=(1, 2, 4, 257)), ERR_UNSUPPORTED), (dict(null='grid'), ERR_ARG),
                     (dict(null='start'), ERR_ARG), (dict(null='goal'), ERR_ARG), (dict(null='cells'), ERR_ARG),
                     (dict(null='status'), ERR_ARG), (dict(dims=(0, 2, 4, 4)), ERR_ARG), (dict(dims=(1, 0, 4, 4)), ERR_ARG),
                     (dict(dims=(1, 2, 0, 4)), ERR_ARG), (dict(dims=(1, 2, 4, 0)), ERR_ARG),
                     (dict(dims=(2 ** 22, 1024, 4, 4)), ERR_ARG),
                     # N is refused before the map size is looked at
                     (dict(dims=(1, 1025, 257, 4)), ERR_ARG)):
        out = call(lib, 1, 2, 4, 4, expect=code, **kw)
        assert (out['grid'] == 0x5a).all(), kw
        for k in cc.OUTPUTS[1:]:
            assert (out[k] == POISON).all(), (kw, k)            # nothing enqueued


# ---- the chain generate -> distances -> orders -> solve ------------------------------------------------------------
@pytest.mark.parametrize('name', ['random_20x20', 'random_40x40', 'hashed_rows_W65', 'hashed_tall_map_of_two_waves',
                                  'team_fills_the_region_next_to_one_agent_too_many', 'many_components_at_density_045'])
def test_every_agent_of_a_generated_case_has_a_path(lib, name):
    from test_emu_mapf_distance import call_distances
    out = run_case(lib, name)
    ok = out['status'] == cc.OK
    assert ok.any()
    d = call_distances(lib, out['grid'][ok], out['start'][ok], out['goal'][ok])
    assert (d['dist'] >= 1).all() and (d['lower_makespan'] >= 1).all()
    assert np.array_equal(d['dist'], dc.want_distances(out['grid'][ok], out['start'][ok], out['goal'][ok])[0])


def test_generated_cases_through_orders_and_the_solver(lib):
    """The 20 x 20 set, 64 cases of 10 agents: 'mixed' orders with four restarts ranked from the generated cases'
    distances, then gnnpp_mapf_solve -- every output equals the solver's yardstick on the twin's orders."""
    from test_emu_mapf_distance import solve_with_rules
    gen = run_case(lib, 'random_20x20')
    grids, starts, goals = gen['grid'], gen['start'], gen['goal']
    T = mc.default_horizon(20, 20)
    out, d, order = solve_with_rules(lib, grids, starts, goals, T, dc.mixed_rules(4), seed=3)
    assert (d['dist'] >= 1).all()
    twin = dc.rank_orders(d['dist'], dc.mixed_rules(4), seed=3)
    assert np.array_equal(order, twin)
    mc.assert_outputs_equal(out, [mc.solve_case(grids[c], starts[c].astype(np.int64), goals[c].astype(np.int64), T,
                                                list(twin[c])) for c in range(len(grids))])
    assert (out['status'] == 0).any() and set(out['status'].tolist()) <= {0, mc.NO_PATH}
