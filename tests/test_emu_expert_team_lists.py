"""CPU: gnnpp_schedule_team_plan, gnnpp_schedule_team_fill_lists and gnnpp_team_lists_gather
(csrc/expert_team_lists_kernel.hip, compiled unmodified for the host emulation): the graphs of expert schedules as capped
neighbour lists against the lists of what the REAL reference transformer made (tests/golden/expert_schedules_team.npz),
of the sequential restatement tests/expert_cases.py::reference_samples on random cases, and of
gnnpp_schedule_team_samples' own S; every other output against that call's, byte for byte.  Equality everywhere.
Statement, runner and the hand-built cases (run on the device too): tests/expert_team_lists_cases.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expert_cases as ec  # noqa: E402
import expert_team_lists_cases as lc  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')

GOLD = lc.load_team_golden()


@pytest.fixture(scope='module')
def lib():
    import emu_lib
    return emu_lib.load()


assert_plan_outputs_equal_dense = lc.assert_plan_outputs_equal_dense


def true_step_deg(S32):
    return (S32 != 0).sum(1).max(1)


@pytest.mark.parametrize('ci,N,deg', [(1, 130, 15), (0, 160, 18), (3, 200, 37), (2, 256, 21)])
def test_golden_case(lib, ci, N, deg):
    m, g = GOLD[ci]
    assert m['N'] == N
    h = lc.HostCall(lib, g['grid'], g['goal'][None], [g['schedule']]).plan()
    assert np.isnan(h.out['obs']).all()                                        # the plan writes no observation
    S32 = g['GSO'].astype(np.float32)
    assert h.out['step_deg'].max() == deg and (h.out['step_deg'] == true_step_deg(S32)).all()
    h.fill(lc.roundup4(deg))
    lc.check_lists('golden %d' % ci, *h.lists(), lc.lists_of_dense(S32))
    assert h.margins_intact()
    assert h.out['radius'][0] == float.fromhex(m['radius']) and h.out['growth'][0] == m['growth']
    assert np.array_equal(h.out['obs'], g['input'].astype(np.float32))
    assert_plan_outputs_equal_dense(h, h.dense())
    again = lc.HostCall(lib, g['grid'], g['goal'][None], [g['schedule']]).plan().fill(lc.roundup4(deg))
    for a, b in zip(h.lists(), again.lists()):                                 # two calls: the same bytes, poison included
        assert a.tobytes() == b.tobytes()


_random, _want = lc.random_schedule, lc.want_gso


@pytest.mark.parametrize('N,side', [(2, 3), (5, 4), (7, 4), (130, 17)])
def test_tiny_map_where_everybody_neighbours_everybody(lib, N, side):
    assert (N, side) in lc.TINY_MAPS
    lc.case_tiny_map_where_everybody_neighbours_everybody(lib, N, side)


@pytest.mark.parametrize('N,side,steps', [(2, 6, 3), (5, 9, 4), (7, 12, 4), (130, 60, 3)])
def test_random_case_against_restatement(lib, N, side, steps):
    grid, goal, sched = _random(N, side, steps, 1000 + N, density=0.1)
    want = lc.lists_of_dense(_want(grid, goal, sched))
    h = lc.plan_and_fill(lib, grid, goal[None], [sched])
    lc.check_lists('random %d' % N, *h.lists(), want)
    assert h.margins_intact()
    assert_plan_outputs_equal_dense(h, h.dense())


@pytest.mark.parametrize('N', [7, 130])
def test_set_four_entries_wider_than_needed(lib, N):
    lc.case_set_four_entries_wider_than_needed(lib, N)


def test_largest_degree_exactly_cap(lib):
    lc.case_largest_degree_exactly_cap(lib)


def test_flagged_case_between_two_good_ones(lib):
    lc.case_flagged_case_between_two_good_ones(lib)


@pytest.mark.parametrize('N,side,radius0', [(130, 60, 5.0), (7, 4, 30.0)])
def test_cap_four_below_the_need(lib, N, side, radius0):
    assert (N, side, radius0) in lc.SHORT_CAPS
    lc.case_cap_four_below_the_need(lib, N, side, radius0)


@pytest.mark.parametrize('name', lc.THIN_CALLS)
def test_thin_map(lib, name):
    lc.case_thin_map(lib, name)


@pytest.mark.parametrize('name', lc.THIN_SHORT_CAPS)
def test_thin_map_cap_four_below_the_need(lib, name):
    lc.case_thin_map(lib, name, short=True)


# ---- gnnpp_team_lists_gather ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pool(lib):
    """The capped set of the 5 steps of a 130-agent case, its dense S and the standard blocks of S."""
    return lc.gather_pool(lib)


@pytest.mark.parametrize('index', [[0, 1, 2, 3, 4], [2, 2, 0, 2], [4, 3, 2, 1, 0], [3]],
                         ids=['identity', 'repeated', 'reversed', 'B1'])
def test_gather(lib, pool, index):
    assert index in lc.GATHERS.values()
    lc.case_gather(lib, pool, index)


def test_gather_clamps_an_index_out_of_range(lib, pool):
    lc.case_gather_clamps_an_index_out_of_range(lib, pool)


def test_gather_from_a_set_at_the_standard_stride(lib):
    lc.case_gather_from_a_set_at_the_standard_stride(lib)


def test_runner_with_twins_of_every_array(lib):
    """lc.DeviceRunner, which the device tests run every case through, on twins in host memory: the emulated library
    sees only the twins, and the cases hold as they do on the arrays themselves."""
    run = lc.DeviceRunner('cpu')
    lc.case_tiny_map_where_everybody_neighbours_everybody(lib, 5, 4, run)
    lc.case_flagged_case_between_two_good_ones(lib, run)
    lc.case_gather(lib, lc.gather_pool(lib, run), [2, 2, 0, 2], run)
    with pytest.raises(AssertionError, match='lies in none of the buffers'):
        run(lib.gnnpp_team_lists_bytes, (1 << 40, 4), [])


# ---- errors -----------------------------------------------------------------------------------------------------------
def test_argument_errors(lib):
    """The codes of the three calls; nothing is written on any of them."""
    m, g = ec.load_golden()[7]
    ok = (g['grid'], g['goal'][None], [g['schedule']])
    N = g['goal'].shape[0]
    good = lc.plan_and_fill(lib, *ok)
    assert good.out['status'][0] == 0 and (good.out['cnt'] >= 0).all()

    def plan_untouched(h):
        assert all(np.isnan(h.out[k]).all() for k in ('obs', 'target', 'radius')) and np.isnan(h.ws).all()
        assert all((h.out[k] == -1).all() for k in ('growth', 'status', 'step_info', 'step_deg'))

    plan_untouched(lc.HostCall(lib, *ok).plan(expect=lc.ERR_ARG, step_deg=False))
    plan_untouched(lc.HostCall(lib, *ok).plan(expect=lc.ERR_ARG, ws=False))
    h = lc.HostCall(lib, *ok)
    plan_untouched(h.plan(expect=lc.ERR_ARG, ws_bytes=h.need - 8))
    for radius0 in (0.0, float('nan'), 1e300):
        plan_untouched(lc.HostCall(lib, *ok, radius0=radius0).plan(expect=lc.ERR_ARG))
    h = lc.HostCall(lib, *ok)
    h.s.target = None
    plan_untouched(h.plan(expect=lc.ERR_ARG))
    one = (g['grid'], g['goal'][None, :1], [g['schedule'][:, :1]])
    plan_untouched(lc.HostCall(lib, *one).plan(expect=lc.ERR_UNSUPPORTED))
    big = (g['grid'], np.zeros((1, 1025, 2), np.int32), [np.zeros((1, 1025, 2), np.int32)])
    plan_untouched(lc.HostCall(lib, *big).plan(expect=lc.ERR_ARG))
    huge = (np.zeros((256, 257), np.uint8), g['goal'][None], [g['schedule']])
    plan_untouched(lc.HostCall(lib, *huge).plan(expect=lc.ERR_UNSUPPORTED))
    assert lib.gnnpp_schedule_team_plan(None, good.ws.ctypes.data, good.need, good.out['step_deg'].ctypes.data, None) \
        == lc.ERR_ARG
    h = lc.HostCall(lib, *ok)                            # obs, S and S64 may be NULL for the plan
    h.s.obs = None
    assert h.plan().out['status'][0] == 0 and h.out['step_deg'].max() == good.out['step_deg'].max()

    def fill_untouched(**kw):
        h = lc.HostCall(lib, *ok).plan()
        before = {k: v.copy() for k, v in h.out.items()}
        cap = kw.pop('cap', good.cap)
        mutate = kw.pop('mutate', None)
        if mutate:
            mutate(h)
        h.fill(cap, expect=kw.pop('expect', lc.ERR_ARG), **kw)
        assert h.lists_untouched() and np.isnan(h.out['obs']).all()
        for k in lc.PLAN_OUTPUTS + ('step_deg',):
            assert h.out[k].tobytes() == before[k].tobytes(), k

    Np = lc.roundup4(N)
    for pass_cap in (0, -4, 2, good.cap + 1, Np + 4):
        fill_untouched(cap=Np + 4, pass_cap=pass_cap)
    for null in ('cnt', 'idx', 'val'):
        fill_untouched(null=null)
    for mis in ((4, 0, 0), (0, 8, 0), (0, 0, 4)):
        fill_untouched(misalign=mis)
    fill_untouched(ws=False)
    fill_untouched(ws_bytes=good.need - 8)
    fill_untouched(mutate=lambda h: setattr(h.s, 'obs', None))
    fill_untouched(mutate=lambda h: setattr(h.s, 'radius', None))
    fill_untouched(mutate=lambda h: setattr(h.s, 'H', 256) or setattr(h.s, 'W', 257), expect=lc.ERR_UNSUPPORTED)

    def gather_untouched(**kw):
        raw, block = lc.host_gather(lib, good.lists(), good.T, good.cap, [0, 1], N, expect=lc.ERR_ARG, **kw)
        assert (block == 0xFF).all() and lc.margins_intact(raw, block)

    for kw in (dict(cnt=None), dict(idx=None), dict(val=None), dict(index=None), dict(lists=None),
               dict(cnt=good.out['cnt'].ctypes.data + 4), dict(idx=good.out['idx'].ctypes.data + 8),
               dict(val=good.out['val'].ctypes.data + 4), dict(graphs_src=0), dict(B=0), dict(N=0), dict(N=1025),
               dict(cap=0), dict(cap=6), dict(cap=Np + 4),
               dict(lists_bytes=lib.gnnpp_team_lists_bytes(2, N) - 1)):
        gather_untouched(**kw)
    raw, block = lc.guarded(lib.gnnpp_team_lists_bytes(2, N) + 16)
    index = np.zeros(2, np.int32)
    assert lib.gnnpp_team_lists_gather(good.out['cnt'].ctypes.data, good.out['idx'].ctypes.data,
                                       good.out['val'].ctypes.data, good.T, good.cap, index.ctypes.data, 2,
                                       block.ctypes.data + 8, block.size - 8, N, None) == lc.ERR_ARG      # misaligned block
    assert (block == 0xFF).all()
    assert lib.gnnpp_version() == 330
