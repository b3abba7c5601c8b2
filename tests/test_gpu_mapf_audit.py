"""MI355X: gnnpp_mapf_audit through mapf.enqueue_audit / mapf.audit / Solutions.audit on the whole table of
tests/mapf_audit_cases.py (the 128 KB owner table of 256 x 256 maps and teams of 1024 included): exact equality with the
sequential restatement, on poisoned device outputs and a poisoned workspace, every call made twice with the same bytes;
the solvers' own answers audit clean with the solvers' arrivals and costs; a call on a side stream and a replay of
generate -> distances -> orders -> solve -> audit from one captured graph give the bytes of the eager chain;
samples_from_solutions(audit=True) builds the same samples from clean solutions and refuses a corrupted schedule by case,
t and agents; mapf.quality is >= 1 on solved cases.  The corrupted schedules are plain integer data inside the call's
contract."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mapf_audit_cases as ac  # noqa: E402
import mapf_distance_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def mapf():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from gnn_pathplanning_amd import _native, mapf as m
    _native.lib()
    return m


def poisoned_audit(mapf, C, N, T):
    out = mapf.empty_audit(C, N, T, DEV)
    for k in ac.OUTPUTS:
        getattr(out, k).fill_(ac.POISON)
    out.workspace.fill_(0x5a)
    return out


def device_call(mapf):
    def call(case, out):
        dev = torch.device(DEV)
        C, T1, N, _ = case['schedule'].shape
        t = {k: None if case[k] is None else torch.from_numpy(case[k]).to(dev)
             for k in ('grid', 'start', 'goal', 'schedule', 'steps')}
        got = poisoned_audit(mapf, C, N, T1 - 1)
        mapf.enqueue_audit(t['grid'], t['start'], t['goal'], t['schedule'], t['steps'], got)
        torch.cuda.synchronize()
        for k in ac.OUTPUTS:
            out[k][...] = getattr(got, k).cpu().numpy()
    return call


@pytest.mark.parametrize('name', sorted(ac.CASES))
def test_named_cases_equal_the_restatement(mapf, name):
    ac.run(device_call(mapf), name)


def test_audit_takes_host_arrays_and_lists_of_schedules(mapf):
    """mapf.audit on host arrays; and on a list of schedules of different lengths, padded, with steps from the lengths."""
    case, want = ac.wants_of('sparse_walkers_meet_every_class')
    got = mapf.audit(case['grid'], case['start'], case['goal'], case['schedule'], DEV)
    ac.assert_equal('sparse_walkers_meet_every_class', {k: getattr(got, k).cpu().numpy() for k in ac.OUTPUTS}, want)
    assert got.ok().tolist() == [True, False]
    text = got.describe(1)
    assert 'a vertex conflict at t = 5: agent 2 and agent 3' in text and 'status 15' in text and '2 x swap' in text
    assert 'collision-free' in got.describe(0)
    case, want = ac.wants_of('mixed_steps_in_one_call')
    keep = [1, 3, 4]                                         # steps 3, 2 and 0: schedules of 4, 3 and 1 rows
    rows = [case['schedule'][c, :int(case['steps'][c]) + 1] for c in keep]
    got = mapf.audit(case['grid'], None, case['goal'][keep], rows, DEV)
    for k in ac.OUTPUTS:
        assert np.array_equal(getattr(got, k).cpu().numpy(), want[k][keep]), k


def _solver_outputs(sol):
    return {k: getattr(sol, k).cpu().numpy() for k in ('status', 'arrival', 'makespan', 'flowtime')}


@pytest.mark.parametrize('team', [False, True], ids=['solve', 'solve_team'])
def test_the_solvers_own_answers_audit_clean(mapf, team):
    """Solutions.audit() on the seeded sets of mapf_distance_cases.py: status 0 and the solver's arrivals and costs for
    every solved case, SKIPPED for every unsolved one; mapf.quality >= 1 where solved, NaN elsewhere."""
    small, large = dc.explicit_order_sets()
    sets = [large] if team else [small, dc.mixed_set()]
    seen_unsolved = False
    for cases in sets:
        grids, starts, goals = (np.stack([c[k] for c in cases]) for k in range(3))
        sol = (mapf.solve_team if team else mapf.solve)(grids, starts, goals, DEV)
        found = sol.audit()
        lower = mapf.distances(grids, starts, goals, DEV)
        s, a = _solver_outputs(sol), {k: getattr(found, k).cpu().numpy() for k in ac.OUTPUTS}
        solved = s['status'] == 0
        assert solved.any()
        seen_unsolved |= bool((~solved).any())
        assert (a['status'][solved] == 0).all() and (a['status'][~solved] == ac.SKIPPED).all()
        assert np.array_equal(found.ok(), solved)
        for k in ('arrival', 'makespan', 'flowtime'):
            assert np.array_equal(a[k][solved], s[k][solved]), k
            assert (a[k][~solved] == -1).all(), k
        assert (a['counts'][solved] == 0).all() and (a['first'] == -1).all() and (a['counts'][~solved] == -1).all()
        for q in mapf.quality(found, lower) + mapf.quality(sol, lower):
            q = q.cpu().numpy()
            assert q.dtype == np.float64 and (q[solved] >= 1).all() and np.isnan(q[~solved]).all()
    assert team or seen_unsolved


def test_side_stream_and_the_captured_chain(mapf):
    """generate -> distances -> orders -> solve_team -> audit as one linear chain of launches on one stream: enqueued on a
    side stream, and captured once and replayed, it writes the bytes of the eager call (3 cases of 130 agents on 40 x 70)."""
    from gnn_pathplanning_amd import casegen
    dev = torch.device(DEV)
    C, N, H, W, T = 3, 130, 40, 70, 160
    rules = [mapf.ORDER_RULES[r] for r in dc.mixed_rules(4)]
    case_outs = ('grid', 'start', 'goal', 'cells', 'status')
    solve_outs = ('schedules', 'arrival', 'makespan', 'flowtime', 'status', 'failing', 'restart')

    def fresh():
        cases = casegen.empty_cases(C, N, H, W, DEV)
        cases.grid.fill_(0x5a)
        for k in case_outs[1:]:
            getattr(cases, k).fill_(-7)
        out = mapf.empty_solutions(C, N, H, T, DEV, 4, W=W, team=True)
        for k in solve_outs:
            getattr(out, k).fill_(-7)
        out.workspace.fill_(0x5a)
        d = mapf.Distances(*(torch.full(s, -7, dtype=torch.int32, device=dev) for s in ((C, N), (C,), (C,))))
        return cases, out, d, torch.full((C, 4, N), -7, dtype=torch.int32, device=dev), poisoned_audit(mapf, C, N, T)

    def chain(cases, out, d, order, found):
        casegen.enqueue_generate(cases, density=0.1, seed=31)
        mapf.enqueue_distances(cases.grid, cases.start, cases.goal, d)
        mapf.enqueue_orders(d.dist, rules, 3, order)
        mapf.enqueue_solve_team(cases.grid, cases.start, cases.goal, order, out)
        mapf.enqueue_audit(cases.grid, cases.start, cases.goal, out.schedules, out.makespan, found)

    def tensors(bufs):
        cases, out, d, order, found = bufs
        return ([getattr(cases, k) for k in case_outs] + [getattr(out, k) for k in solve_outs] + list(d) + [order] +
                [getattr(found, k) for k in ac.OUTPUTS])

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
    assert (graphed[4].status == ac.POISON).all() and (graphed[1].status == -7).all()       # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    for bufs in (side_bufs, graphed):
        for x, y in zip(tensors(eager), tensors(bufs)):
            assert torch.equal(x, y)
    sol, found = eager[1], eager[4]
    solved = sol.status == 0
    assert bool(solved.any()) and bool((found.status[solved] == 0).all())
    assert bool((found.status[~solved] == ac.SKIPPED).all())
    assert torch.equal(found.arrival[solved], sol.arrival[solved]) and torch.equal(found.flowtime[solved], sol.flowtime[solved])
    # the restatement on what the chain produced
    case = ac.make_case('chain', eager[0].grid.cpu().numpy(), eager[0].goal.cpu().numpy(), sol.schedules.cpu().numpy(),
                        start=eager[0].start.cpu().numpy(), steps=sol.makespan.cpu().numpy())
    ac.assert_equal('chain', {k: getattr(found, k).cpu().numpy() for k in ac.OUTPUTS}, ac.audit(case))


def _same_samples(a, b):
    for k in ('input', 'GSO', 'target', 'radius', 'growth', 'status', 'step_growth'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.bounds == b.bounds


@pytest.mark.parametrize('team', [False, True], ids=['solve', 'solve_team'])
def test_samples_from_audited_solutions(mapf, team):
    """audit=True builds the samples of audit=False from clean solutions, and refuses a schedule in which one agent was
    put on another's cell by hand, naming the case, t and both agents."""
    from gnn_pathplanning_amd import _native, expert
    small, large = dc.explicit_order_sets()
    cases = large[:2] if team else small
    grids, starts, goals = (np.stack([c[k] for c in cases]) for k in range(3))
    sol = (mapf.solve_team if team else mapf.solve)(grids, starts, goals, DEV, priorities='longest_first')
    plain, ids = expert.samples_from_solutions(sol, grids, goals, team=team)
    audited, ids2 = expert.samples_from_solutions(sol, grids, goals, team=team, audit=True)
    assert len(ids) and np.array_equal(ids, ids2)
    _same_samples(plain, audited)
    bad = mapf.Solutions(**vars(sol))
    bad.schedules = sol.schedules.clone()
    c, t = int(ids[-1]), 1
    assert int(sol.makespan[c]) >= 2
    bad.schedules[c, t, 4] = bad.schedules[c, t, 2]
    with pytest.raises(_native.GnnppError, match=r'case %d \(of %d\) fails its audit: a vertex conflict at t = 1: agent 2 and '
                                                 r'agent 4' % (len(ids) - 1, len(ids))):
        expert.samples_from_solutions(bad, grids, goals, team=team, audit=True)


def test_a_swap_from_another_solver_is_refused_only_when_audited(mapf):
    """Two agents that exchange their cells: every move is one of the five actions and every state is free, so the
    per-agent checks of the sample builder pass it; the audit names the swap."""
    from gnn_pathplanning_amd import _native, expert
    grid = np.zeros((6, 6), np.uint8)
    clean = np.array([[(0, 0), (3, 3)], [(0, 1), (3, 4)], [(0, 2), (3, 5)]])
    swap = np.array([[(2, 2), (2, 3)], [(2, 2), (2, 3)], [(2, 3), (2, 2)]])
    goals = np.stack([clean[-1], swap[-1]])
    plain = expert.samples_from_schedules(grid, goals, [clean, swap], DEV)
    assert plain.bounds == [0, 3, 6]
    with pytest.raises(_native.GnnppError, match=r'case 1 \(of 2\) fails its audit: a swap conflict at t = 1: agent 0 and '
                                                 r'agent 1 .*status 8'):
        expert.samples_from_schedules(grid, goals, [clean, swap], DEV, audit=True)
    _same_samples(expert.samples_from_schedules(grid, goals[:1], [clean], DEV),
                  expert.samples_from_schedules(grid, goals[:1], [clean], DEV, audit=True))


def test_error_codes_leave_poisoned_device_buffers_untouched(mapf):
    from gnn_pathplanning_amd import _native
    L = _native.lib()
    dev = torch.device(DEV)
    case, _ = ac.wants_of('vertex_t4')
    C, T1, N, _ = case['schedule'].shape
    H, W = case['grid'].shape
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ('grid', 'start', 'goal', 'schedule')}
    out = poisoned_audit(mapf, C, N, T1 - 1)
    st = _native.stream_ptr(dev)

    def call(C=C, N=N, H=H, W=W, T=T1 - 1, null=None, short=0):
        p = {k: v.data_ptr() for k, v in t.items()}
        p.update({k: getattr(out, k).data_ptr() for k in ac.OUTPUTS + ('workspace',)})
        if null:
            p[null] = None
        return L.gnnpp_mapf_audit(p['grid'], 0, p['start'], p['goal'], p['schedule'], None, C, N, H, W, T,
                                  *[p[k] for k in ac.OUTPUTS], p['workspace'], out.workspace.numel() - short, st)
    assert call(N=1025) == call(N=0) == call(C=0) == call(H=0) == call(T=-1) == call(T=2049) == _native.ERR_ARG
    assert call(H=257) == call(W=257) == call(H=257, T=2049) == _native.ERR_UNSUPPORTED
    assert call(short=1) == _native.ERR_ARG and call(N=1025, W=257) == _native.ERR_ARG
    for k in ('grid', 'goal', 'schedule', 'workspace') + ac.OUTPUTS:
        assert call(null=k) == _native.ERR_ARG, k
    torch.cuda.synchronize()
    assert all((getattr(out, k) == ac.POISON).all() for k in ac.OUTPUTS) and (out.workspace == 0x5a).all()
    assert call(null='start') == 0
    torch.cuda.synchronize()
    assert out.counts[0].tolist() == [0, 2, 0, 0]
