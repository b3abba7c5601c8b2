"""MI355X: gnnpp_mapf_distances / gnnpp_mapf_orders through mapf.distances, mapf.heuristic_orders and the string
priorities of mapf.solve / mapf.solve_team, on the cases of tests/mapf_distance_cases.py (the ones the host emulation
runs): exact equality with a queue-based breadth-first search and an np.lexsort restatement of the ranking rules; the
case the index order fails and longest first solves; the same bytes as explicit orders and as the solver's yardstick
on seeded sets; 'mixed' never worse than the default call; the lower bounds; the chain on a side stream and replayed
from a captured graph; the documented error codes on poisoned device buffers."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mapf_cases as mc  # noqa: E402
import mapf_distance_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OUTS = ('schedules', 'arrival', 'makespan', 'flowtime', 'status', 'failing', 'restart')


@pytest.fixture(scope='module')
def mapf():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from gnn_pathplanning_amd import _native, mapf as m
    _native.lib()
    return m


def stacked(cases):
    return np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])


def host(sol):
    return {k: getattr(sol, k).cpu().numpy() for k in OUTS}


# ---- distances -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(dc.CASES))
def test_distances_equal_the_queue_search(mapf, name):
    case = dc.CASES[name]()
    d = mapf.distances(case['grid'], case['starts'], case['goals'], DEV)
    dist, lm, lf = (t.cpu().numpy() for t in d)
    assert d.dist.dtype == torch.int32 and d.lower_makespan.dtype == torch.int32
    dc.assert_equal_to_yardstick(case, dist, lm, lf)


def test_shared_grid_next_to_batched_grid(mapf):
    case = dc.CASES['shared_grid_next_to_batched_grid']()
    a = mapf.distances(case['grid'][0], case['starts'], case['goals'], DEV)
    b = mapf.distances(case['grid'], case['starts'], case['goals'], DEV)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    dc.assert_equal_to_yardstick(case, *(t.cpu().numpy() for t in a))


# ---- orders --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', dc.ORDER_SIZES)
def test_orders_equal_the_lexsort_twin(mapf, N):
    keys = dc.synthetic_keys(N)
    dev_keys = torch.from_numpy(keys).to(torch.int32).to(DEV)
    got = mapf.heuristic_orders(dev_keys, dc.ALL_RULES, seed=5)
    assert got.dtype == torch.int32 and tuple(got.shape) == (3, 4, N)
    dc.assert_permutations(got.cpu().numpy(), N)
    assert np.array_equal(got.cpu().numpy(), dc.rank_orders(keys, dc.ALL_RULES, seed=5))
    for rule in dc.ALL_RULES:
        alone = mapf.heuristic_orders(dev_keys, [rule], seed=5).cpu().numpy()
        assert np.array_equal(alone, dc.rank_orders(keys, [rule], seed=5)), rule


def test_more_rules_than_one_launch_takes(mapf):
    keys = dc.synthetic_keys(65)
    rules = (dc.ALL_RULES * 9)[:35]
    got = mapf.heuristic_orders(torch.from_numpy(keys).to(torch.int32).to(DEV), rules, seed=9)
    assert np.array_equal(got.cpu().numpy(), dc.rank_orders(keys, rules, seed=9))


# ---- end to end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fn', ['solve', 'solve_team'])
def test_longest_first_solves_what_the_index_order_does_not(mapf, fn):
    grid, starts, goals, T = dc.corridor_2x4()
    solve = getattr(mapf, fn)
    sol = solve(grid, starts[None], goals[None], DEV, max_steps=T)
    assert (int(sol.status[0]), int(sol.failing[0]), sol.arrival[0].tolist()) == (mapf.NO_PATH, 1, [1, -1])
    assert not hasattr(sol, 'distance')
    sol = solve(grid, starts[None], goals[None], DEV, max_steps=T, priorities='longest_first')
    assert (int(sol.status[0]), int(sol.failing[0]), sol.arrival[0].tolist()) == (0, -1, [3, 3])
    assert sol.distance.tolist() == [[1, 3]] and sol.lower_makespan.tolist() == [3] and sol.lower_flowtime.tolist() == [4]
    assert sol.priorities.tolist() == [[[1, 0]]]
    mc.assert_outputs_equal({k if k != 'schedules' else 'schedule': v for k, v in host(sol).items()},
                            [mc.solve_case(grid, starts, goals, T, [[1, 0]])])
    sol = solve(grid, starts[None], goals[None], DEV, max_steps=T, priorities='mixed')
    assert (int(sol.status[0]), int(sol.restart[0]), tuple(sol.priorities.shape)) == (0, 1, (1, 3, 2))


# ---- the same bytes as explicit orders, and as the solver's yardstick ----------------------------------------------
@pytest.fixture(scope='module')
def order_sets():
    """Per solver: (cases, T, the queue search's distances, {priorities: (twin orders, yardstick outputs)}), computed
    once.  The large-team set is planned with a horizon of 160 steps, beyond every arrival on 40 x 70."""
    made = {}
    for fn, cases in zip(('solve', 'solve_team'), dc.explicit_order_sets()):
        grids, starts, goals = stacked(cases)
        T = mc.default_horizon(20, 20) if fn == 'solve' else 160
        dist = dc.want_distances(grids, starts, goals)[0]
        per = {}
        for prio, rules in (('longest_first', ['longest_first']), ('mixed', dc.mixed_rules(4))):
            twin = dc.rank_orders(dist, rules, seed=3)
            per[prio] = (twin, [mc.solve_case(*cases[c], T, list(twin[c])) for c in range(len(cases))])
        made[fn] = (cases, T, dist, per)
    return made


@pytest.mark.parametrize('fn', ['solve', 'solve_team'])
@pytest.mark.parametrize('prio', ['longest_first', 'mixed'])
def test_string_priorities_equal_explicit_orders(mapf, order_sets, fn, prio):
    """6 cases of 10 agents on 20 x 20 (solve), 3 cases of 130 agents on 40 x 70 (solve_team)."""
    cases, T, dist, per = order_sets[fn]
    twin, wants = per[prio]
    solve = getattr(mapf, fn)
    sol = solve(*stacked(cases), DEV, max_steps=T, restarts=4, seed=3, priorities=prio)
    explicit = solve(*stacked(cases), DEV, max_steps=T, priorities=twin)
    assert np.array_equal(sol.priorities.cpu().numpy(), twin) and np.array_equal(sol.distance.cpu().numpy(), dist)
    for k in OUTS:
        assert torch.equal(getattr(sol, k), getattr(explicit, k)), k
    h = host(sol)
    mc.assert_outputs_equal({k if k != 'schedules' else 'schedule': v for k, v in h.items()}, wants)
    print(fn, prio, 'status', h['status'].tolist(), 'restart', h['restart'].tolist())
    # the lower bounds hold for every solved case
    solved = h['status'] == 0
    assert solved.any()
    assert (h['arrival'][solved] >= dist[solved]).all()
    assert (h['makespan'][solved] >= sol.lower_makespan.cpu().numpy()[solved]).all()
    assert (h['flowtime'][solved] >= sol.lower_flowtime.cpu().numpy()[solved]).all()
    assert (sol.lower_makespan.cpu().numpy() == dist.max(1)).all() and (sol.lower_flowtime.cpu().numpy() == dist.sum(1)).all()


def test_mixed_is_never_worse_than_the_default_call(mapf):
    """32 cases of 10 agents on 12 x 12 at density 0.2.  Restart 0 of 'mixed' is the index order, so every case the
    default call solves is solved by 'mixed' with a flowtime that is no larger.  The set must hold solved and unsolved
    cases under the index order -- asserted on the yardstick's answer, so the test cannot pass on an empty premise."""
    cases = dc.mixed_set()
    T = mc.default_horizon(12, 12)
    index_status = np.array([mc.solve_case(g, s, gl, T)['status'] for g, s, gl in cases])
    assert (index_status == 0).any() and (index_status == mc.NO_PATH).any()
    default = mapf.solve(*stacked(cases), DEV)
    assert np.array_equal(default.status.cpu().numpy(), index_status)
    mixed = mapf.solve(*stacked(cases), DEV, restarts=4, seed=1, priorities='mixed')
    d, m = host(default), host(mixed)
    was = d['status'] == 0
    assert (m['status'][was] == 0).all() and (m['flowtime'][was] <= d['flowtime'][was]).all()
    print('solved: default %d, mixed %d of %d' % (was.sum(), (m['status'] == 0).sum(), len(cases)))
    now = m['status'] == 0
    assert (m['arrival'][now] >= mixed.distance.cpu().numpy()[now]).all()
    assert (m['makespan'][now] >= mixed.lower_makespan.cpu().numpy()[now]).all()
    assert (m['flowtime'][now] >= mixed.lower_flowtime.cpu().numpy()[now]).all()


def test_maxstep_from_distances_on_the_device(mapf):
    """Distances 10, 10, 10, 4 (invalid_ends_flag_only_themselves): lower makespan 10, so rate 1.25 gives 13 and rate
    0.01 the least limit, 1; the case with invalid ends raises."""
    from gnn_pathplanning_amd import _native
    case = dc.CASES['invalid_ends_flag_only_themselves']()
    d = mapf.distances(case['grid'], case['starts'], case['goals'], DEV)
    with pytest.raises(_native.GnnppError, match=r'cases \[1\]'):
        mapf.maxstep_from_distances(d.lower_makespan, 2)
    ok = d.lower_makespan[[0, 2]]
    got = mapf.maxstep_from_distances(ok, 1.25)
    assert got.is_cuda and got.dtype == torch.int32 and got.tolist() == [13, 13]
    assert mapf.maxstep_from_distances(ok, 0.01).tolist() == [1, 1]


# ---- streams and graphs --------------------------------------------------------------------------------------------
def test_chain_on_a_side_stream_and_from_a_captured_graph(mapf):
    """distances -> orders -> solve_team as one linear chain of launches on one stream: enqueued on a side stream, and
    captured once and replayed, it writes the bytes of the eager call."""
    cases = dc.explicit_order_sets()[1]
    dev = torch.device(DEV)
    grid, start, goal = (torch.from_numpy(a).to(dev) for a in stacked(cases))
    start, goal = start.to(torch.int32), goal.to(torch.int32)
    C, N, H, W = 3, 130, 40, 70
    T, rules = 160, [mapf.ORDER_RULES[r] for r in dc.mixed_rules(4)]

    def fresh():
        out = mapf.empty_solutions(C, N, H, T, DEV, 4, W=W, team=True)
        for k in OUTS:
            getattr(out, k).fill_(-7)
        out.workspace.fill_(0x5a)
        d = mapf.Distances(*(torch.full(s, -7, dtype=torch.int32, device=dev) for s in ((C, N), (C,), (C,))))
        return out, d, torch.full((C, 4, N), -7, dtype=torch.int32, device=dev)

    def chain(out, d, order):
        mapf.enqueue_distances(grid, start, goal, d)
        mapf.enqueue_orders(d.dist, rules, 3, order)
        mapf.enqueue_solve_team(grid, start, goal, order, out)

    eager = fresh()
    chain(*eager)
    torch.cuda.synchronize()
    side_bufs = fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain(*side_bufs)
    side.synchronize()
    graphed = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain(*graphed)
    torch.cuda.synchronize()
    assert (graphed[0].status == -7).all() and (graphed[2] == -7).all()     # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    for out, d, order in (side_bufs, graphed):
        for k in OUTS:
            assert torch.equal(getattr(eager[0], k), getattr(out, k)), k
        for x, y in zip(eager[1], d):
            assert torch.equal(x, y)
        assert torch.equal(eager[2], order)
    assert (eager[0].status == 0).any() and not (eager[2] == -7).any() and not (eager[1].dist == -7).any()
    want = dc.rank_orders(dc.want_distances(*stacked(cases))[0], dc.mixed_rules(4), seed=3)
    assert np.array_equal(eager[2].cpu().numpy(), want)


# ---- errors --------------------------------------------------------------------------------------------------------
def test_error_codes_leave_poisoned_device_buffers_untouched(mapf):
    import ctypes
    from gnn_pathplanning_amd import _native
    L = _native.lib()
    dev = torch.device(DEV)
    grid = torch.zeros((4, 4), dtype=torch.uint8, device=dev)
    pts = torch.zeros((1, 1025, 2), dtype=torch.int32, device=dev)
    dist = torch.full((1, 1025), -7, dtype=torch.int32, device=dev)
    lm, lf = torch.full((1,), -7, dtype=torch.int32, device=dev), torch.full((1,), -7, dtype=torch.int32, device=dev)
    order = torch.full((1, 1, 1024), -7, dtype=torch.int32, device=dev)
    st = _native.stream_ptr(dev)

    def distances(N=2, H=4, W=4, d=dist, m=lm):
        return L.gnnpp_mapf_distances(grid.data_ptr(), 0, pts.data_ptr(), pts.data_ptr(), 1, N, H, W,
                                      d.data_ptr() if d is not None else None,
                                      m.data_ptr() if m is not None else None, lf.data_ptr(), st)
    assert distances(N=1025) == _native.ERR_ARG
    assert distances(H=257) == _native.ERR_UNSUPPORTED and distances(W=257) == _native.ERR_UNSUPPORTED
    assert distances(N=1025, H=257) == _native.ERR_ARG
    assert distances(d=None) == _native.ERR_ARG and distances(m=None) == _native.ERR_ARG
    one = (ctypes.c_int * 1)(_native.MAPF_ORDER_LONGEST_FIRST)
    assert L.gnnpp_mapf_orders(dist.data_ptr(), 1, 1025, 1, one, 0, order.data_ptr(), st) == _native.ERR_ARG
    assert L.gnnpp_mapf_orders(dist.data_ptr(), 1, 4, 1, one, 0, None, st) == _native.ERR_ARG
    assert L.gnnpp_mapf_orders(None, 1, 4, 1, one, 0, order.data_ptr(), st) == _native.ERR_ARG
    one[0] = 4
    assert L.gnnpp_mapf_orders(dist.data_ptr(), 1, 4, 1, one, 0, order.data_ptr(), st) == _native.ERR_ARG
    torch.cuda.synchronize()
    for t in (dist, lm, lf, order):
        assert (t == -7).all()
    with pytest.raises(_native.GnnppError, match='1 to 1024 agents'):
        mapf.distances(grid, pts, pts, DEV)
    with pytest.raises(_native.GnnppError, match='at most 256 x 256'):
        mapf.distances(torch.zeros((257, 4)), pts[:, :2], pts[:, :2], DEV)
    with pytest.raises(_native.GnnppError, match='rules'):
        mapf.heuristic_orders(dist[:, :4], ['shortest'])
    with pytest.raises(_native.GnnppError, match='priorities as a string'):
        mapf.solve(grid, pts[:, :2], pts[:, :2], DEV, priorities='random')
