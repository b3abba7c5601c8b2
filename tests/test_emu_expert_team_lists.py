"""CPU: gnnpp_schedule_team_plan, gnnpp_schedule_team_fill_lists and gnnpp_team_lists_gather
(csrc/expert_team_lists_kernel.hip, compiled unmodified for the host emulation): the graphs of expert schedules as capped
neighbour lists against the lists of what the REAL reference transformer made (tests/golden/expert_schedules_team.npz),
of the sequential restatement tests/expert_cases.py::reference_samples on random cases, and of
gnnpp_schedule_team_samples' own S; every other output against that call's, byte for byte.  Equality everywhere.
Statement and runner: tests/expert_team_lists_cases.py."""
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
    return lc.bind(emu_lib.load())


def assert_plan_outputs_equal_dense(h, dense, obs=True):
    """target, radius, growth, status, step_info, the workspace (and obs) byte for byte what the dense call writes --
    NaN poison included: the same elements are left unwritten."""
    for k in lc.PLAN_OUTPUTS + (('obs',) if obs else ()):
        assert h.out[k].tobytes() == dense[k].tobytes(), k
    assert h.ws.tobytes() == dense['ws'].tobytes()


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


def _random(N, side, steps, seed, **kw):
    rng = np.random.default_rng(seed)
    grid, goal, paths = ec.random_case(rng, N, side, side, max_steps=steps, **kw)
    return grid, goal, ec.schedule_of(paths, goal)


def _want(grid, goal, sched, radius0=5.0):
    return ec.reference_samples(grid, goal, sched, radius0)['GSO'].astype(np.float32)


@pytest.mark.parametrize('N,side', [(2, 3), (5, 4), (7, 4), (130, 17)])
def test_tiny_map_where_everybody_neighbours_everybody(lib, N, side):
    """radius0 = 30 spans the whole map: degree N - 1 everywhere.  cap = roundup4(N - 1), which is roundup4(N) -- the
    standard block's stride -- unless N = 1 mod 4; at N = 5 the degree 4 IS cap: a column without padding."""
    grid, goal, sched = _random(N, side, 3, 40 + N, density=0.0)
    h = lc.plan_and_fill(lib, grid, goal[None], [sched], radius0=30.0)
    assert (h.out['step_deg'] == N - 1).all() and h.cap == lc.roundup4(N - 1)
    assert h.cap == (lc.roundup4(N) if N % 4 != 1 else N - 1)
    assert (h.out['cnt'] == N - 1).all()
    lc.check_lists('full %d' % N, *h.lists(), lc.lists_of_dense(_want(grid, goal, sched, 30.0)))
    assert h.margins_intact()
    assert_plan_outputs_equal_dense(h, h.dense())


@pytest.mark.parametrize('N,side,steps', [(2, 6, 3), (5, 9, 4), (7, 12, 4), (130, 60, 3)])
def test_random_case_against_restatement(lib, N, side, steps):
    grid, goal, sched = _random(N, side, steps, 1000 + N, density=0.1)
    want = lc.lists_of_dense(_want(grid, goal, sched))
    h = lc.plan_and_fill(lib, grid, goal[None], [sched])
    lc.check_lists('random %d' % N, *h.lists(), want)
    assert h.margins_intact()
    assert_plan_outputs_equal_dense(h, h.dense())


def _chain7():
    """Seven agents waiting in a row, four cells apart: at most two neighbours each under radius 5."""
    pos = np.stack([np.zeros(7, np.int64), 4 * np.arange(7)], 1)
    return np.zeros((1, 30), np.uint8), pos, np.stack([pos, pos])


@pytest.mark.parametrize('N', [7, 130])
def test_set_four_entries_wider_than_needed(lib, N):
    """The tail of every column stays poison (a chain of 7 at the standard stride 8; a random team of 130)."""
    grid, goal, sched = _chain7() if N == 7 else _random(N, 60, 3, 1000 + N, density=0.1)
    want = lc.lists_of_dense(_want(grid, goal, sched))
    h = lc.plan_and_fill(lib, grid, goal[None], [sched])
    assert h.cap + 4 <= lc.roundup4(N)
    wide = lc.plan_and_fill(lib, grid, goal[None], [sched], extra=4)
    assert wide.cap == h.cap + 4
    lc.check_lists('wide %d' % N, *wide.lists(), want)
    assert (wide.out['idx'][:, :, h.cap:] == 0xFFFF).all()
    assert (wide.out['val'][:, :, h.cap:].view(np.uint32) == 0xFFFFFFFF).all()
    assert wide.margins_intact()
    lc.same_lists('wide %d' % N, wide.lists(), h.lists())


def test_largest_degree_exactly_cap(lib):
    """129 agents on a 17 x 17 map that radius0 = 30 spans: degree 128 = cap, below the standard stride of 132; every
    column is full, no padding anywhere, and the last store of a column ends where the next column begins."""
    N = 129
    grid, goal, sched = _random(N, 17, 2, 7, density=0.0)
    h = lc.plan_and_fill(lib, grid, goal[None], [sched], radius0=30.0)
    assert h.cap == 128 and (h.out['cnt'] == 128).all() and h.cap < lc.roundup4(N)
    lc.check_lists('exact', *h.lists(), lc.lists_of_dense(_want(grid, goal, sched, 30.0)))
    assert h.margins_intact()


def test_flagged_case_between_two_good_ones(lib):
    N = 130
    grid, goal, sched = _random(N, 44, 3, 5, density=0.1)
    bad = sched.copy()
    bad[1, 70] = np.argwhere(grid != 0)[0]              # a state on an obstacle
    h = lc.HostCall(lib, grid, np.stack([goal] * 3), [sched, bad, sched]).plan()
    T = len(sched)
    assert h.out['status'][0] == 0 and h.out['status'][1] != 0 and h.out['status'][2] == 0
    assert (h.out['step_deg'][T:2 * T] == 0).all() and (h.out['step_deg'][:T] > 0).all()
    h.fill(max(4, lc.roundup4(h.out['step_deg'].max())))
    want = lc.lists_of_dense(_want(grid, goal, sched))
    lc.check_lists('left', *h.lists(), want, graphs=[(t, t) for t in range(T)])
    lc.check_lists('right', *h.lists(), want, graphs=[(2 * T + t, t) for t in range(T)])
    for k in ('cnt', 'idx', 'val'):                     # the flagged case's steps stay poison
        assert (h.out[k][T:2 * T].view(np.uint8) == 0xFF).all(), k
    assert np.isnan(h.out['obs'][T:2 * T]).all() and np.isnan(h.out['target'][T:2 * T]).all()
    assert h.margins_intact()
    assert_plan_outputs_equal_dense(h, h.dense())
    alone = lc.plan_and_fill(lib, grid, goal[None], [sched])
    for k in ('cnt', 'idx', 'val', 'obs'):              # the neighbours are unaffected
        assert h.out[k][:T].tobytes() == alone.out[k].tobytes() == h.out[k][2 * T:].tobytes(), k


@pytest.mark.parametrize('N,side,radius0', [(130, 60, 5.0), (7, 4, 30.0)])
def test_cap_four_below_the_need(lib, N, side, radius0):
    """cnt is the true degree, the first cap entries are right, nothing is written outside a column's cap entries."""
    grid, goal, sched = _random(N, side, 3, 1000 + N, density=0.1 if N > 7 else 0.0)
    h = lc.HostCall(lib, grid, goal[None], [sched], radius0).plan()
    need = lc.roundup4(h.out['step_deg'].max())
    assert need >= 8
    h.fill(need - 4)
    assert (h.out['cnt'] > need - 4).any() and h.out['cnt'].max() == h.out['step_deg'].max()
    lc.check_lists('short %d' % N, *h.lists(), lc.lists_of_dense(_want(grid, goal, sched, radius0)), cap=need - 4)
    assert h.margins_intact()
    full = lc.HostCall(lib, grid, goal[None], [sched], radius0).plan().fill(need)
    assert (h.out['cnt'] == full.out['cnt']).all()
    live = np.arange(need - 4)[None, None, :] < ((full.out['cnt'] + 3) & ~3)[:, :, None]
    assert (h.out['idx'][live] == full.out['idx'][:, :, :need - 4][live]).all()


# ---- gnnpp_team_lists_gather ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pool(lib):
    """The capped set of the 5 steps of a 130-agent case, its dense S and the standard blocks of S."""
    grid, goal, sched = _random(130, 60, 5, 2030, density=0.1)
    h = lc.plan_and_fill(lib, grid, goal[None], [sched])
    return h, h.dense()['S']


def _from_dense(lib, S):
    graphs, N = S.shape[:2]
    nbytes = lib.gnnpp_team_lists_bytes(graphs, N)
    raw, block = lc.guarded(nbytes)
    S = np.ascontiguousarray(S)
    assert lib.gnnpp_team_lists_from_dense(S.ctypes.data, block.ctypes.data, nbytes, graphs, N, 0, None) == 0
    return block


@pytest.mark.parametrize('index', [[0, 1, 2, 3, 4], [2, 2, 0, 2], [4, 3, 2, 1, 0], [3]],
                         ids=['identity', 'repeated', 'reversed', 'B1'])
def test_gather(lib, pool, index):
    h, S = pool
    N, B = h.N, len(index)
    raw, block = lc.host_gather(lib, h.lists(), h.T, h.cap, index, N)
    assert lc.margins_intact(raw, block)
    got = lc.block_views(block, B, N)
    want = _from_dense(lib, S[index])
    lc.same_lists('gather', got, lc.block_views(want, B, N))
    lc.check_lists('gather', *got, lc.lists_of_dense(S[index]))
    nbytes = lib.gnnpp_team_lists_bytes(B, N)                                  # symmetry: the lists of S^T are the same
    rawt, blockt = lc.guarded(nbytes)
    assert lib.gnnpp_team_lists_transpose(block.ctypes.data, blockt.ctypes.data, nbytes, B, N, None) == 0
    lc.same_lists('transpose', got, lc.block_views(blockt, B, N))
    # entries behind roundup4(cnt) are not copied
    cnt, idx, _ = got
    behind = np.arange(idx.shape[2])[None, None, :] >= ((cnt + 3) & ~3)[:, :, None]
    assert (idx[behind] == 0xFFFF).all()


def test_gather_clamps_an_index_out_of_range(lib, pool):
    """include/gnnpp.h: an index outside [0, graphs_src) is clamped into that range."""
    h, S = pool
    raw, block = lc.host_gather(lib, h.lists(), h.T, h.cap, [-3, 5, 1 << 30, 1], h.N)
    assert lc.margins_intact(raw, block)
    lc.check_lists('clamped', *lc.block_views(block, 4, h.N), lc.lists_of_dense(S[[0, 4, 4, 1]]))


def test_gather_from_a_set_at_the_standard_stride(lib):
    """cap == roundup4(N), N % 4 != 0: the three arrays are the regions of a standard block."""
    N = 7
    grid, goal, sched = _random(N, 4, 3, 47, density=0.0)
    h = lc.plan_and_fill(lib, grid, goal[None], [sched], radius0=30.0)
    assert h.cap == 8 == lc.roundup4(N)
    raw, block = lc.host_gather(lib, h.lists(), h.T, h.cap, np.arange(h.T), N)
    for a, b in zip(lc.block_views(block, h.T, N), h.lists()):
        assert a.tobytes() == b.tobytes()
    assert lc.margins_intact(raw, block)


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
