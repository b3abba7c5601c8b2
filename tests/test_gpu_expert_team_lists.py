"""MI355X: expert samples of large teams kept as neighbour lists up to the training step --
expert.samples_from_schedules_team(graph='lists') (gnnpp_schedule_team_plan + gnnpp_schedule_team_fill_lists),
expert.SampleListPool (gnnpp_team_lists_gather) and training.train_step_lists -- against the golden cases of the real
reference, the dense route followed by graphML.team_lists_from_dense, and forward_train_lists on the lists of the dense
GSO.  Equality everywhere: integers, {0, 1} values and fp64 products in a fixed order.
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
import mapf_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLD = lc.load_team_golden()
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


def host_lists(s, a=0, b=None):
    """(cnt int32, idx uint16, val float32) numpy arrays of steps a .. b of lists samples."""
    b = len(s) if b is None else b
    return (s.cnt[a:b].cpu().numpy(), s.idx[a:b].cpu().numpy().view(np.uint16), s.val[a:b].cpu().numpy())


def host_block(block, graphs, N):
    return lc.block_views(block.cpu().numpy(), graphs, N)


@pytest.mark.parametrize('ci,cap', [(1, 16), (0, 20), (2, 24), (4, 24), (3, 40)])
def test_golden_case(expert, ci, cap):
    m, g = GOLD[ci]
    s = expert.samples_from_schedules_team(g['grid'], g['goal'][None], [g['schedule']], DEV, graph='lists')
    T, N = m['T'], m['N']
    assert s.GSO is None and s.GSO64 is None and s.cap == cap
    assert s.cnt.shape == (T, N) and s.idx.shape == (T, N, cap) and s.val.shape == (T, N, cap)
    S32 = g['GSO'].astype(np.float32)
    lc.check_lists('golden %d' % ci, *host_lists(s), lc.lists_of_dense(S32))
    assert s.step_deg.cpu().tolist() == (S32 != 0).sum(1).max(1).tolist()
    assert s.radius[0].item() == float.fromhex(m['radius']) and s.growth[0].item() == m['growth']
    assert torch.equal(s.input.cpu(), torch.from_numpy(g['input'].astype(np.float32)))
    assert torch.equal(s.target.cpu(), torch.from_numpy(g['target'].astype(np.float32)))
    assert s.step_growth.max().item() == m['growth'] and s.step_growth.min().item() >= 0


def _random_cases(N, side, cases, cap):
    rng = np.random.default_rng(1000 * N + side)
    made = [ec.random_case(rng, N, side, side, density=0.08, wait=0.2, max_steps=int(rng.integers(3, cap + 1)))
            for _ in range(cases)]
    return made, [ec.schedule_of(paths, goal) for _, goal, paths in made]


@pytest.mark.parametrize('N,side,cases,cap', [(129, 40, 4, 8), (384, 48, 2, 4)])
def test_equal_to_the_dense_route(expert, N, side, cases, cap):
    from gnn_pathplanning_amd import graphML as gml
    made, sched = _random_cases(N, side, cases, cap)
    args = (np.stack([g for g, _, _ in made]), np.stack([g for _, g, _ in made]), sched, DEV)
    dense = expert.samples_from_schedules_team(*args)
    lists = expert.samples_from_schedules_team(*args, graph='lists')
    T = len(dense)
    for k in ('input', 'target', 'radius', 'growth', 'status', 'step_growth'):
        assert torch.equal(getattr(dense, k), getattr(lists, k)), k
    assert lists.cap == max(4, lc.roundup4(int(lists.step_deg.max())))
    want = host_block(gml.team_lists_from_dense(dense.GSO), T, N)
    lc.same_lists('N%d' % N, host_lists(lists), want)
    assert (want[0].max(1) == lists.step_deg.cpu().numpy()).all()
    pool = expert.SampleListPool()                       # ... and the draw gives the standard block of those lists
    pool.append(lists)
    inp, tgt, block = pool.gather(torch.arange(T - 1, -1, -1))
    assert torch.equal(inp, dense.input.flip(0)) and torch.equal(tgt, dense.target.flip(0))
    lc.same_lists('N%d/gather' % N, host_block(block, T, N), tuple(w[::-1] for w in want))
    c_in, (c_cnt, c_idx, c_val), c_tgt = lists.case(1)
    a, b = lists.bounds[1], lists.bounds[2]
    assert torch.equal(c_in, dense.input[a:b]) and torch.equal(c_cnt, lists.cnt[a:b]) and c_idx.shape[0] == b - a


def test_refusals(expert):
    from gnn_pathplanning_amd._native import GnnppError
    m, g = GOLD[1]
    with pytest.raises(GnnppError, match='keep_fp64_gso'):
        expert.samples_from_schedules_team(g['grid'], g['goal'][None], [g['schedule']], DEV, keep_fp64_gso=True,
                                           graph='lists')
    with pytest.raises(GnnppError, match='unknown graph'):
        expert.samples_from_schedules_team(g['grid'], g['goal'][None], [g['schedule']], DEV, graph='csr')
    bad = g['schedule'].copy()
    bad[2, 100] = bad[1, 100] + [0, 2]
    with pytest.raises(GnnppError, match=r'case 1 \(of 2\).*not one of the five actions'):
        expert.samples_from_schedules_team(g['grid'], np.stack([g['goal']] * 2), [g['schedule'], bad], DEV, graph='lists')
    pool = expert.SampleListPool()
    with pytest.raises(GnnppError, match="graph='lists'"):
        pool.append(expert.samples_from_schedules_team(g['grid'], g['goal'][None], [g['schedule']], DEV))
    good = expert.samples_from_schedules_team(g['grid'], g['goal'][None], [g['schedule']], DEV, graph='lists')
    pool.append(good)
    short = expert.ScheduleSamples(**good.__dict__)     # a set filled below its need: a count beyond cap
    short.cnt = good.cnt + good.cap
    with pytest.raises(GnnppError, match='invalid'):
        pool.append(short)
    assert len(pool) == len(good)
    m0, g0 = GOLD[0]
    with pytest.raises(GnnppError, match='one team size'):
        pool.append(expert.samples_from_schedules_team(g0['grid'], g0['goal'][None], [g0['schedule']], DEV, graph='lists'))


def _planner(N, K=3, route='dense'):
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from oracle import policy_oracle as orc
    dev = torch.device(DEV)

    class Cfg:
        num_agents, nGraphFilterTaps, device, largeGraphFilter = N, K, dev, route
    net = DecentralPlannerNet(Cfg()).to(dev)
    net.load_state_dict(orc.init_state_dict(K, seed=7))
    return net.train()


def test_pool_draw_and_train_step_lists_equal_the_lists_of_the_dense_gso(expert):
    """N = 130, B = 2, K = 3: loss, logits and every parameter gradient of train_step_lists on the pool's draw are
    bit-identical to forward_train_lists on team_lists_from_dense of the same samples' dense GSO -- the two blocks agree
    on every byte the kernels read."""
    from gnn_pathplanning_amd import graphML as gml, training as tr
    m, g = GOLD[1]
    args = (g['grid'], g['goal'][None], [g['schedule']], DEV)
    dense = expert.samples_from_schedules_team(*args)
    pool = expert.SampleListPool()
    pool.append(expert.samples_from_schedules_team(*args, graph='lists'))
    pick = torch.tensor([3, 1])
    N = m['N']

    def run(step):
        net = _planner(N)
        seen = {}
        orig = tr._policy_loss_and_grad
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(tr, '_policy_loss_and_grad', lambda lg, t: (seen.setdefault('logits', lg.detach().clone()),
                                                                   orig(lg, t))[1])
            loss = step(net, torch.optim.SGD(net.parameters(), lr=0.0))
        return loss, seen['logits'], {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}

    inp, tgt, block = pool.gather(pick)
    got = run(lambda net, opt: tr.train_step_lists(net, opt, inp, tgt, block))
    dev_pick = pick.to(DEV)
    want_block = gml.team_lists_from_dense(dense.GSO.index_select(0, dev_pick))
    lc.same_lists('draw', host_block(block, 2, N), host_block(want_block, 2, N))
    want = run(lambda net, opt: tr.train_step_lists(net, opt, dense.input.index_select(0, dev_pick),
                                                    dense.target.index_select(0, dev_pick), want_block))
    assert torch.isfinite(got[0]) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[2].keys() == want[2].keys() and len(got[2]) > 10
    for k in got[2]:
        assert torch.equal(got[2][k], want[2][k]), k
    # symmetric=False spends a transpose launch on the same lists: the same bits again
    other = run(lambda net, opt: tr.train_step_lists(net, opt, inp, tgt, block, symmetric=False))
    assert torch.equal(other[0], got[0]) and all(torch.equal(other[2][k], got[2][k]) for k in got[2])


def test_pool_grows_its_cap(expert):
    """Samples of cap 16 (golden 1) and then of cap 24 (agents drawn together in a 30 x 30 box: largest degree 24, by
    the numpy restatement): one pool, draws across both."""
    from gnn_pathplanning_amd import graphML as gml
    m, g = GOLD[1]
    N = m['N']
    first = (g['grid'], g['goal'][None], [g['schedule']], DEV)
    rng = np.random.default_rng(28)
    grid, goal, paths = ec.random_case(rng, N, 40, 40, density=0.05, box=(5, 5, 30), max_steps=3)
    second = (grid, goal[None], [ec.schedule_of(paths, goal)], DEV)
    parts = [expert.samples_from_schedules_team(*a, graph='lists') for a in (first, second)]
    assert parts[0].cap == 16 and parts[1].cap == 24 and int(parts[1].step_deg.max()) == 24
    dense = [expert.samples_from_schedules_team(*a) for a in (first, second)]
    for order in ((0, 1), (1, 0)):                      # widening the pool, and widening what arrives
        pool = expert.SampleListPool()
        for k in order:
            pool.append(parts[k])
        assert pool.cap == 24 and len(pool) == len(parts[0]) + len(parts[1])
        T = len(pool)
        inp, tgt, block = pool.gather(torch.arange(T))
        S = torch.cat([dense[k].GSO for k in order])
        lc.same_lists('grown', host_block(block, T, N), host_block(gml.team_lists_from_dense(S), T, N))
        assert torch.equal(inp, torch.cat([dense[k].input for k in order]))
        inp, tgt, block = pool.draw(3, torch.Generator(device=DEV).manual_seed(1))
        assert inp.shape == (3, N, 3, 11, 11) and block.numel() == gml.team_lists_bytes(3, N)
        inp, tgt, block = pool.draw(T + 2)              # more than the pool holds: with replacement
        assert inp.shape[0] == T + 2


def test_rollout_to_train_step_on_lists_with_130_agents(expert):
    """The closed loop without a dense matrix: BatchedRollout(graph='lists') of an untrained policy -> solve_failures ->
    samples_from_solutions(team=True, graph='lists') -> SampleListPool -> train_step_lists."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    from gnn_pathplanning_amd.training import train_step_lists
    dev = torch.device(DEV)
    B, N, side = 2, 130, 64
    cases = mc.random_cases(np.random.default_rng(31), B, N, side, density=0.1)
    grids, starts, goals = (np.stack([c[k] for c in cases]) for k in range(3))
    net = _planner(N, route='lists')
    ro = BatchedRollout(grids, starts, goals, 4, dev, tie_mode='lowest', graph='lists')
    res = ro.run(net.eval())
    assert not res['success'].any()
    sol = expert.solve_failures(ro, results=res)
    samples, ids = expert.samples_from_solutions(sol, grids, goals, team=True, graph='lists')
    assert len(ids) >= 1 and samples.GSO is None
    want = ec.reference_samples(grids[ids[0]], goals[ids[0]], sol.schedule(ids[0]))
    lc.check_lists('loop', *host_lists(samples, 0, samples.bounds[1]), lc.lists_of_dense(want['GSO'].astype(np.float32)))
    pool = expert.SampleListPool()
    pool.append(samples)
    inp, tgt, block = pool.draw(2, torch.Generator(device=dev).manual_seed(3))
    net.train()
    before = [p.detach().clone() for p in net.parameters()]
    loss = train_step_lists(net, torch.optim.Adam(net.parameters(), lr=1e-3), inp, tgt, block).item()
    assert np.isfinite(loss) and loss > 0
    assert any(not torch.equal(a, b) for a, b in zip(before, net.parameters()))


def test_lists_call_never_allocates_a_dense_graph(expert):
    """The golden 1024-agent case (T = 3): the rise of the allocator's peak over the 'lists' call stays below ONE dense
    S [T,N,N] (12.6 MB); expected are 4.4 MB of observations, 0.06 MB of targets, 0.45 MB of lists and the inputs."""
    m, g = GOLD[4]
    T, N = m['T'], m['N']
    assert (T, N) == (3, 1024)
    args = (torch.from_numpy(g['grid']).to(DEV), torch.from_numpy(g['goal'][None]).to(DEV), [g['schedule']], DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    s = expert.samples_from_schedules_team(*args, graph='lists')
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print('peak rise over the lists call: %d bytes' % rise)
    assert rise < T * N * N * 4
    assert s.cap == 24 and rise >= expert.team_lists_output_bytes(T, N, 24)


def test_graph_capture_gives_the_same_bytes(expert):
    """plan + fill_lists captured once in a HIP graph (cap from the eager run) and replayed."""
    m, g = GOLD[0]
    dev = torch.device(DEV)
    grids, goals, scheds = np.stack([g['grid']] * 2), np.stack([g['goal']] * 2), [g['schedule']] * 2
    eager = expert.samples_from_schedules_team(grids, goals, scheds, DEV, graph='lists')
    grid = torch.from_numpy(grids).to(dev)
    goal = torch.from_numpy(goals.astype(np.int32)).to(dev)
    pos = torch.from_numpy(np.concatenate(scheds).astype(np.int32)).to(dev)
    T, N, C, cap = len(eager), m['N'], 2, eager.cap

    def f(*shape, dtype=torch.float32):
        return torch.full(shape, -7, dtype=dtype, device=dev)
    out = expert.ScheduleSamples(input=f(T, N, 3, 11, 11), GSO=None, GSO64=None, target=f(T, N, 5),
                                 radius=f(C, dtype=torch.float64), growth=f(C, dtype=torch.int32),
                                 status=f(C, dtype=torch.int32), step_growth=f(T, dtype=torch.int32),
                                 step_deg=f(T, dtype=torch.int32), workspace=f(T * N, dtype=torch.float64),
                                 cnt=f(T, N, dtype=torch.int32), idx=f(T, N, cap, dtype=torch.int16), val=f(T, N, cap),
                                 cap=cap)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        expert.enqueue_schedule_team_plan(grid, goal, pos, eager.case_start, out)
        expert.enqueue_schedule_team_fill_lists(grid, goal, pos, eager.case_start, out)
    torch.cuda.synchronize()
    assert (out.input == -7).all() and (out.cnt == -7).all()                  # captured, not run
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        out.step_growth &= 0xffff
        for k in ('input', 'target', 'radius', 'growth', 'status', 'step_growth', 'step_deg', 'cnt'):
            assert torch.equal(getattr(out, k), getattr(eager, k)), k
        lc.same_lists('graph', host_lists(out), host_lists(eager))
        for t in (out.input, out.cnt, out.idx, out.val):
            t.fill_(-7)
