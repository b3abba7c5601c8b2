"""MI355X: expert.SchedulePool, the pool that stores schedules and builds every batch when it is drawn
(gnnpp_schedule_draw), against the materialised pools it replaces -- expert.SamplePool and expert.SampleListPool fed with
samples_from_schedules_team of the same cases.  Equality everywhere: the batches are the same bytes, so the losses and
the parameters after training on them are too.
Every test ends on a device synchronisation; once one has raised, the tests after it fail at once and start nothing
more on the card.  Run the file under a time limit of its own."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expert_cases as ec  # noqa: E402
import expert_team_lists_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_faulted = []


@pytest.fixture(autouse=True)
def nothing_after_a_fault():
    if _faulted:
        pytest.fail('an earlier test of this file left the device in error: %s' % _faulted[0])
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                              # noqa: BLE001 (a HIP error surfaces as RuntimeError)
        _faulted.append(repr(e))
        raise


@pytest.fixture(scope='module')
def expert():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from gnn_pathplanning_amd import _native, expert as ex
    _native.lib()
    return ex


_CASES = {}


def cases_of(N, side, count=4):
    """`count` random cases of 3 .. 5 steps, a map per case: (grids [C,H,W], goals [C,N,2], schedules)."""
    if (N, side, count) not in _CASES:
        rng = np.random.default_rng(500 + N)
        made = [ec.random_case(rng, N, side, side, density=0.08, wait=0.2, max_steps=3 + k % 3) for k in range(count)]
        _CASES[N, side, count] = (np.stack([g for g, _, _ in made]), np.stack([g for _, g, _ in made]),
                                  [ec.schedule_of(paths, goal) for _, goal, paths in made])
    return _CASES[N, side, count]


def both_pools(expert, N, side, graph='dense'):
    """The same cases in two appends each: (materialised pool, SchedulePool)."""
    grids, goals, sched = cases_of(N, side)
    old = expert.SamplePool() if graph == 'dense' else expert.SampleListPool()
    new = expert.SchedulePool(DEV)
    for part in (slice(0, 1), slice(1, None)):
        old.append(expert.samples_from_schedules_team(grids[part], goals[part], sched[part], DEV, graph=graph))
        new.append(grids[part], goals[part], sched[part])
    assert len(old) == len(new) == sum(len(s) for s in sched) and new.cases == len(sched)
    return old, new


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def host_block(block, graphs, N):
    return lc.block_views(block.cpu().numpy(), graphs, N)


@pytest.mark.parametrize('N,side', [(5, 9), (130, 40)])
def test_draws_equal_sample_pool(expert, N, side):
    old, new = both_pools(expert, N, side)
    T = len(old)
    assert T > 4
    for batch in (4, T + 3):                             # without replacement, and more than the pool holds
        for g in (lambda: gen(11), lambda: torch.Generator().manual_seed(11)):
            want, got = old.draw(batch, g()), new.draw(batch, g())
            assert got[0].shape == (batch, N, 3, 11, 11) and got[2].shape == (batch, N, N)
            for w, x in zip(want, got):
                assert torch.equal(w, x)
    idx = [T - 1, 0, 0, 3]
    for w, x in zip(old.gather(idx), new.gather(idx)):
        assert torch.equal(w, x)


def test_draws_equal_sample_list_pool(expert):
    N = 130
    old, new = both_pools(expert, N, 40, graph='lists')
    T = len(old)
    for batch in (4, T + 3):
        want, got = old.draw(batch, gen(5)), new.draw(batch, gen(5), graph='lists')
        assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
        assert got[2].dtype is torch.uint8 and got[2].numel() == want[2].numel()
        lc.same_lists('draw %d' % batch, host_block(got[2], batch, N), host_block(want[2], batch, N))


def test_append_solutions_on_a_tiny_solve(expert):
    from gnn_pathplanning_amd import mapf
    import mapf_cases as mc
    N, side = 5, 9
    cases = mc.random_cases(np.random.default_rng(21), 4, N, side, density=0.1)
    grid = np.zeros((side, side), np.uint8)              # a fifth case: agent 1 starts walled in -> no path
    grid[6, 6:9] = 1
    grid[6:9, 6] = 1
    cases.append((grid, np.array([[0, 0], [8, 8], [0, 5], [2, 0], [4, 4]]), np.array([[1, 1], [0, 3], [2, 5], [1, 0], [4, 5]])))
    grids, starts, goals = (np.stack([c[k] for c in cases]) for k in range(3))
    sol = mapf.solve(grids, starts, goals, DEV)
    status = sol.status.cpu().numpy()
    assert status[4] != 0 and (status[:4] == 0).any()
    samples, ids = expert.samples_from_solutions(sol, grids, goals)
    old, new = expert.SamplePool(), expert.SchedulePool(DEV)
    old.append(samples)
    got_ids = new.append_solutions(sol, grids, goals)
    assert got_ids.tolist() == ids.tolist() == np.nonzero(status == 0)[0].tolist() and 4 not in got_ids
    assert len(new) == len(old) == len(samples) and new.cases == len(ids)
    for batch in (4, len(old) + 2):
        for w, x in zip(old.draw(batch, gen(3)), new.draw(batch, gen(3))):
            assert torch.equal(w, x)
    for w, x in zip(old.gather(torch.arange(len(old))), new.gather(torch.arange(len(old)))):
        assert torch.equal(w, x)


def test_flagged_case_in_append_leaves_the_pool_unchanged(expert):
    from gnn_pathplanning_amd._native import GnnppError
    old, new = both_pools(expert, 5, 9)
    grids, goals, sched = cases_of(5, 9)
    before = (len(new), new.cases, new.nbytes, new.pos.data_ptr(), [t.clone() for t in new.draw(4, gen(2))])
    bad = sched[1].copy()
    bad[1, 2] = bad[0, 2] + [2, 0]                       # two cells in one step
    with pytest.raises(GnnppError, match=r'case 1 \(of 3\).*not one of the five actions'):
        new.append(grids[:3], goals[:3], [sched[0], bad, sched[2]])
    with pytest.raises(GnnppError, match=r'case 1 \(of 3\).*not one of the five actions'):    # ... what the builders raise
        expert.samples_from_schedules_team(grids[:3], goals[:3], [sched[0], bad, sched[2]], DEV)
    assert (len(new), new.cases, new.nbytes, new.pos.data_ptr()) == before[:4]
    for w, x in zip(before[4], new.draw(4, gen(2))):
        assert torch.equal(w, x)
    with pytest.raises(GnnppError, match='one team size and one map size'):
        new.append(*cases_of(7, 9, 1))
    with pytest.raises(GnnppError, match='unknown graph'):
        new.draw(2, graph='csr')
    with pytest.raises(GnnppError, match='empty'):
        expert.SchedulePool(DEV).draw(2)


def _planner(N, K=3):
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from oracle import policy_oracle as orc
    dev = torch.device(DEV)

    class Cfg:
        num_agents, nGraphFilterTaps, device = N, K, dev
    net = DecentralPlannerNet(Cfg()).to(dev)
    net.load_state_dict(orc.init_state_dict(K, seed=7))
    return net.train()


def test_training_from_either_pool_gives_the_same_bits(expert):
    """Two train_step calls at N = 5, B = 4 fed from each pool with the same seed: losses and every parameter equal."""
    from gnn_pathplanning_amd import training as tr
    pools = both_pools(expert, 5, 9)
    runs = []
    for pool in pools:
        net = _planner(5)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        g = gen(9)
        losses = [tr.train_step(net, opt, *pool.draw(4, g)).detach().clone() for _ in range(2)]
        runs.append((losses, {k: p.detach().clone() for k, p in net.named_parameters()}))
    (la, pa), (lb, pb) = runs
    assert all(torch.isfinite(x) for x in la) and all(torch.equal(x, y) for x, y in zip(la, lb))
    assert pa.keys() == pb.keys() and len(pa) > 10
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k


@pytest.mark.parametrize('N,side,shared', [(5, 9, True), (130, 40, True), (5, 9, False)])
def test_memory_bound(expert, N, side, shared):
    """nbytes <= 2 * (steps * (8 N + 8) + cases * (H W + 8 N + 32)): the factor 2 is the capacity slack, the rest the
    positions and a word per step, and map, goals, first step, radius and status per case.  With one shared map (the
    training set-up) no tensor of the pool has more than steps * N * 4 elements: nothing observation-, [steps,N,N]- or
    lists-shaped is kept."""
    grids, goals, sched = cases_of(N, side)
    if shared:
        rng = np.random.default_rng(3)
        made = [ec.random_case(rng, N, side, side, density=0.0, max_steps=4) for _ in range(4)]
        grids, goals, sched = None, np.stack([g for _, g, _ in made]), [ec.schedule_of(p, g) for _, g, p in made]
    pool = expert.SchedulePool(DEV, grid=np.zeros((side, side), np.uint8) if shared else None)
    pool.append(None if shared else grids[:1], goals[:1], sched[:1])
    pool.append(None if shared else grids[1:], goals[1:], sched[1:])
    pool.draw(4, gen(1))                                 # (a draw leaves nothing behind in the pool)
    steps, cases = len(pool), pool.cases
    assert pool.nbytes <= 2 * (steps * (8 * N + 8) + cases * (side * side + 8 * N + 32)), pool.nbytes
    held = [v for v in vars(pool).values() if torch.is_tensor(v)]
    assert sum(t.numel() * t.element_size() for t in held) == pool.nbytes and len(held) >= 6
    assert not any(isinstance(v, (list, tuple, dict)) and any(torch.is_tensor(x) for x in (v.values() if isinstance(v, dict) else v))
                   for v in vars(pool).values())
    if shared:
        assert max(t.numel() for t in held) <= steps * N * 4
    assert pool.nbytes * 20 < steps * N * 1472          # the observations and targets alone of a SamplePool


def test_capacity_growth(expert):
    grids, goals, sched = cases_of(5, 9)
    pool = expert.SchedulePool(DEV)
    pool.append(grids[:2], goals[:2], sched[:2])
    pool.append(grids[2:3], goals[2:3], sched[2:3])      # beyond the first capacity: doubled
    cap_steps, cap_cases = pool.pos.shape[0], pool.goal.shape[0]
    room = min(cap_steps - len(pool), cap_cases - pool.cases)
    assert cap_steps >= len(pool) and room >= 1
    ptrs = [t.data_ptr() for t in (pool.pos, pool.goal, pool.case_start, pool.radius, pool.grids)]
    one = (grids[3:4], goals[3:4], [sched[3][-1:]])      # one more case of ONE step: within both capacities
    pool.append(*one)
    assert ptrs == [t.data_ptr() for t in (pool.pos, pool.goal, pool.case_start, pool.radius, pool.grids)]
    assert pool.pos.shape[0] == cap_steps
    want = expert.SamplePool()
    want.append(expert.samples_from_schedules_team(grids, goals, sched[:3] + one[2], DEV))
    for w, x in zip(want.gather(torch.arange(len(want))), pool.gather(torch.arange(len(pool)))):
        assert torch.equal(w, x)
    pool.reserve(10 * cap_steps, 10 * cap_cases)
    assert pool.pos.shape[0] >= 10 * cap_steps and pool.pos.data_ptr() != ptrs[0]
    for w, x in zip(want.gather([1, 0]), pool.gather([1, 0])):
        assert torch.equal(w, x)


def test_graph_capture(expert, monkeypatch):
    """One HIP graph over enqueue_draw at N = 5, B = 4, replayed twice with the contents of `index` changed in place."""
    from gnn_pathplanning_amd import _native
    old, pool = both_pools(expert, 5, 9)
    T = len(pool)
    index = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=DEV)
    out = pool.draw_buffers(4)
    for t in (out.input, out.target, out.GSO):
        t.fill_(-7)
    streams = []
    real = _native.stream_ptr
    monkeypatch.setattr(_native, 'stream_ptr', lambda dev: streams.append(real(dev)) or streams[-1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        capture_stream = torch.cuda.current_stream().cuda_stream
        before = torch.cuda.memory_allocated()
        pool.enqueue_draw(index, out)
        assert torch.cuda.memory_allocated() == before   # no allocation
    torch.cuda.synchronize()
    assert [s.value for s in streams] == [capture_stream]  # one call, every launch on the capture stream: a single chain
    assert (out.input == -7).all() and (out.GSO == -7).all()                  # captured, not run
    for pick in ([T - 1, 0, 2, 2], [3, T - 2, 1, 0]):
        index.copy_(torch.tensor(pick, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        for w, x in zip(old.gather(pick), (out.input, out.target, out.GSO)):
            assert torch.equal(w, x)
        for w, x in zip(pool.gather(pick), (out.input, out.target, out.GSO)):
            assert torch.equal(w, x)


def test_largest_team_once(expert):
    """1024 agents on a 48 x 48 map, a 2-step schedule, B = 2, lists: the block of fill-lists + gather."""
    N, side = 1024, 48
    grid, goal, sched = lc.random_schedule(N, side, 2, 4096, density=0.05)
    assert len(sched) >= 2
    if len(sched) > 2:                                   # (a schedule cut short: its "goal" is the state that followed)
        goal, sched = sched[2], sched[:2]
    args = (grid, goal[None], [sched])
    old, new = expert.SampleListPool(), expert.SchedulePool(DEV)
    old.append(expert.samples_from_schedules_team(*args, DEV, graph='lists'))
    new.append(*args)
    assert len(new) == len(old) == len(sched)
    pick = [len(sched) - 1, 0]
    want, got = old.gather(pick), new.gather(pick, graph='lists')
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    lc.same_lists('1024', host_block(got[2], 2, N), host_block(want[2], 2, N))
    assert host_block(got[2], 2, N)[0].max() >= 4
