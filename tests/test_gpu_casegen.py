"""MI355X: gnnpp_casegen through casegen.generate / enqueue_generate on the named cases of tests/casegen_cases.py (the ones
the host emulation runs, and the call's limits: 256 x 256 with 1024 agents): exact equality with the numpy / queue
yardstick; the same bytes from two calls, on a side stream, and from a captured graph of the whole chain generate ->
distances -> orders -> solve; every agent of a generated case has a path; generated cases go as they are to
mapf.distances, mapf.solve, mapf.solve_team and BatchedRollout; the documented error codes on poisoned device buffers."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import casegen_cases as cc  # noqa: E402
import mapf_cases as mc  # noqa: E402
import mapf_distance_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def casegen():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from gnn_pathplanning_amd import _native, casegen as m
    _native.lib()
    return m


def density_of(threshold):
    """A density whose casegen.threshold_of is exactly `threshold` (thresholds of the named cases are below 2^32 - 1)."""
    d = threshold / 2 ** 32
    assert cc.threshold_of(d) == threshold
    return d


def run(casegen, case):
    return casegen.generate(case['C'], case['N'], case['H'], case['W'], DEV, density=density_of(case['threshold']),
                            seed=case['seed'], grids=case['grids'])


def host(cases):
    return {k: getattr(cases, k).cpu().numpy() for k in cc.OUTPUTS}


@pytest.mark.parametrize('name', sorted(cc.CASES))
def test_named_cases_equal_the_yardstick(casegen, name):
    got = run(casegen, cc.CASES[name]())
    assert got.grid.dtype == torch.uint8 and got.start.dtype == torch.int32 and got.status.dtype == torch.int32
    out = host(got)
    cc.assert_equal_to_yardstick(name, out)
    assert np.array_equal(got.ok.cpu().numpy(), cc.wants_of(name)['status'] == cc.OK)


def test_properties_and_the_same_bytes_twice(casegen):
    for name in ('random_40x40', 'many_components_at_density_045', 'team_fills_the_region_next_to_one_agent_too_many'):
        case = cc.CASES[name]()
        a, b = host(run(casegen, case)), host(run(casegen, case))
        for k in cc.OUTPUTS:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
        cc.assert_properties(dict(a, raw=cc.wants_of(name)['raw']))


def test_caller_maps_on_the_device_and_yaml(casegen):
    """grids as a device tensor, shared by the cases; a case as the reference's solver input."""
    import yaml
    case = cc.CASES['serpentine_shared_W65']()
    got = casegen.generate(case['C'], case['N'], 5, 65, DEV, seed=case['seed'], grids=torch.from_numpy(case['grids']).to(DEV))
    cc.assert_equal_to_yardstick('serpentine_shared_W65', host(got))
    doc = yaml.safe_load(got.yaml(1))
    assert doc['map']['dimensions'] == [5, 65] and len(doc['map']['obstacles']) == int(got.grid[1].sum())
    assert [a['start'] for a in doc['agents']] == got.start[1].tolist()
    assert [a['goal'] for a in doc['agents']] == got.goal[1].tolist()
    small = run(casegen, cc.CASES['one_by_one_is_too_small']())
    from gnn_pathplanning_amd import _native
    with pytest.raises(_native.GnnppError, match='too small'):
        small.yaml(0)


def test_every_agent_of_a_generated_case_has_a_path(casegen):
    """generate -> mapf.distances on the device tensors as they are: 64 x 10 agents on 20 x 20, 8 x 64 on 40 x 40 and
    2 x 1024 on 256 x 256, every distance >= 1 and equal to the queue search on the generated case."""
    from gnn_pathplanning_amd import mapf
    for name in ('random_20x20', 'random_40x40', 'largest_map_largest_team'):
        got = run(casegen, cc.CASES[name]())
        assert bool(got.ok.all())
        d = mapf.distances(got.grid, got.start, got.goal, DEV)
        assert int(d.dist.min()) >= 1 and int(d.lower_makespan.min()) >= 1, name
        if name != 'largest_map_largest_team':
            want = cc.wants_of(name)
            assert np.array_equal(d.dist.cpu().numpy(), dc.want_distances(want['grid'], want['start'], want['goal'])[0])


def test_generated_cases_go_to_both_solvers(casegen):
    """mapf.solve and mapf.solve_team take Cases.grid / .start / .goal as they are, and answer what the solver's
    yardstick answers on the yardstick's case (the first 8 cases of the 20 x 20 set, index order)."""
    from gnn_pathplanning_amd import mapf
    case = dict(cc.CASES['random_20x20'](), C=8)
    got = run(casegen, case)
    want = cc.wants_of('random_20x20')
    T = mc.default_horizon(20, 20)
    wants = [mc.solve_case(want['grid'][c], want['start'][c], want['goal'][c], T) for c in range(8)]
    for fn in (mapf.solve, mapf.solve_team):
        sol = fn(got.grid, got.start, got.goal, DEV)
        out = {k: getattr(sol, k).cpu().numpy() for k in ('arrival', 'makespan', 'flowtime', 'status', 'failing', 'restart')}
        out['schedule'] = sol.schedules.cpu().numpy()
        mc.assert_outputs_equal(out, wants)
    assert any(w['status'] == 0 for w in wants)


@pytest.mark.parametrize('N,side', [(10, 20), (200, 64)])
def test_generated_cases_go_to_the_rollout(casegen, N, side):
    """BatchedRollout constructs and observes on generated device tensors: the small-team and the large-team kernels."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    got = casegen.generate(4, N, side, side, DEV, density=0.1, seed=21)
    assert bool(got.ok.all())
    env = BatchedRollout(got.grid, got.start, got.goal, 4 * side, DEV)
    obs = env.observe()
    torch.cuda.synchronize()
    assert tuple(obs.shape) == (4, N, 3, 11, 11) and bool(torch.isfinite(obs).all())
    assert torch.equal(env.pos, got.start) and torch.equal(env.goal, got.goal)


def test_side_stream_and_the_captured_chain(casegen):
    """generate -> distances -> orders -> solve_team as one linear chain of launches on one stream: enqueued on a side
    stream, and captured once and replayed, it writes the bytes of the eager call (3 cases of 130 agents on 40 x 70)."""
    from gnn_pathplanning_amd import mapf
    dev = torch.device(DEV)
    C, N, H, W, T = 3, 130, 40, 70, 160
    rules = [mapf.ORDER_RULES[r] for r in dc.mixed_rules(4)]
    solve_outs = ('schedules', 'arrival', 'makespan', 'flowtime', 'status', 'failing', 'restart')

    def fresh():
        cases = casegen.empty_cases(C, N, H, W, DEV)
        cases.grid.fill_(0x5a)
        for k in cc.OUTPUTS[1:]:
            getattr(cases, k).fill_(-7)
        out = mapf.empty_solutions(C, N, H, T, DEV, 4, W=W, team=True)
        for k in solve_outs:
            getattr(out, k).fill_(-7)
        out.workspace.fill_(0x5a)
        d = mapf.Distances(*(torch.full(s, -7, dtype=torch.int32, device=dev) for s in ((C, N), (C,), (C,))))
        return cases, out, d, torch.full((C, 4, N), -7, dtype=torch.int32, device=dev)

    def chain(cases, out, d, order):
        casegen.enqueue_generate(cases, density=0.1, seed=31)
        mapf.enqueue_distances(cases.grid, cases.start, cases.goal, d)
        mapf.enqueue_orders(d.dist, rules, 3, order)
        mapf.enqueue_solve_team(cases.grid, cases.start, cases.goal, order, out)

    def tensors(bufs):
        cases, out, d, order = bufs
        return [getattr(cases, k) for k in cc.OUTPUTS] + [getattr(out, k) for k in solve_outs] + list(d) + [order]

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
    assert (graphed[0].status == -7).all() and (graphed[1].status == -7).all()     # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    for bufs in (side_bufs, graphed):
        for x, y in zip(tensors(eager), tensors(bufs)):
            assert torch.equal(x, y)
    want = cc.generate(C, N, H, W, cc.threshold_of(0.1), 31)
    cc.assert_properties(dict(host(eager[0]), raw=want['raw']))
    for k in cc.OUTPUTS:
        assert np.array_equal(getattr(eager[0], k).cpu().numpy(), want[k]), k
    assert int(eager[2].dist.min()) >= 1 and (eager[1].status == 0).any() and not (eager[3] == -7).any()


def test_error_codes_leave_poisoned_device_buffers_untouched(casegen):
    from gnn_pathplanning_amd import _native
    L = _native.lib()
    dev = torch.device(DEV)
    out = casegen.empty_cases(1, 2, 4, 4, DEV)
    out.grid.fill_(0x5a)
    for k in cc.OUTPUTS[1:]:
        getattr(out, k).fill_(-7)
    st = _native.stream_ptr(dev)

    def call(C=1, N=2, H=4, W=4, null=None):
        ptrs = [None if k == null else getattr(out, k).data_ptr() for k in cc.OUTPUTS]
        return L.gnnpp_casegen(None, 0, 0, 0, C, N, H, W, *ptrs, st)
    assert call(N=1025) == _native.ERR_ARG and call(N=0) == _native.ERR_ARG and call(C=0) == _native.ERR_ARG
    assert call(H=257) == _native.ERR_UNSUPPORTED and call(W=257) == _native.ERR_UNSUPPORTED
    assert call(N=1025, H=257) == _native.ERR_ARG and call(H=0) == _native.ERR_ARG and call(W=0) == _native.ERR_ARG
    assert call(C=2 ** 22, N=1024) == _native.ERR_ARG
    for k in cc.OUTPUTS:
        assert call(null=k) == _native.ERR_ARG
    torch.cuda.synchronize()
    assert (out.grid == 0x5a).all() and all((getattr(out, k) == -7).all() for k in cc.OUTPUTS[1:])
    with pytest.raises(_native.GnnppError, match='N = 1025'):
        casegen.generate(1, 1025, 8, 8, DEV)
    with pytest.raises(_native.GnnppError, match=r'257 x 8'):
        casegen.generate(1, 4, 257, 8, DEV)
    with pytest.raises(_native.GnnppError, match='grids must be'):
        casegen.generate(2, 4, 8, 8, DEV, grids=np.zeros((3, 8, 8)))
    with pytest.raises(_native.GnnppError, match='density'):
        casegen.generate(2, 4, 8, 8, DEV, density=1.5)
