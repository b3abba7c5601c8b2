"""MI355X: gnnpp_schedule_team_samples through expert.samples_from_schedules_team -- the golden cases of the real
reference for teams of 130 ... 1024 agents, random cases against the sequential numpy restatement
(tests/expert_cases.py), the one-wave call on teams both take, graph capture and side streams, a call whose graphs
pass 2^31 elements, and the loop the call closes: rollout -> solve_failures -> samples_from_solutions(team=True) ->
pool -> train_step.  Equality everywhere: the work is on integers, {0, 1} values and fp64 arithmetic the reference
performs in a fixed order."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expert_cases as ec  # noqa: E402
import mapf_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def load_team_golden():
    """[(meta, dict of arrays)] of tests/golden/expert_schedules_team.npz (tools/gen_expert_golden_team.py)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'expert_schedules_team.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    keys = ('grid', 'goal', 'schedule', 'input', 'GSO', 'target')
    return [(m, {k: z['c%d_%s' % (ci, k)] for k in keys}) for ci, m in enumerate(meta)]


GOLD = load_team_golden()
FIELDS = ('input', 'GSO', 'GSO64', 'target', 'radius', 'growth', 'status', 'step_growth')


@pytest.fixture(scope='module')
def expert():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from gnn_pathplanning_amd import _native, expert as ex
    _native.lib()
    return ex


def assert_case(s, c, want_input, want_gso64, want_target, radius, growth):
    a, b = s.bounds[c], s.bounds[c + 1]
    assert s.radius[c].item() == radius and s.growth[c].item() == growth
    assert torch.equal(s.input[a:b].cpu(), torch.from_numpy(np.asarray(want_input, dtype=np.float32)))
    assert torch.equal(s.target[a:b].cpu(), torch.from_numpy(np.asarray(want_target, dtype=np.float32)))
    if s.GSO64 is not None:
        assert torch.equal(s.GSO64[a:b].cpu(), torch.from_numpy(want_gso64))
    assert torch.equal(s.GSO[a:b].cpu(), torch.from_numpy(want_gso64.astype(np.float32)))
    assert s.step_growth[a:b].max().item() == growth and s.step_growth[a:b].min().item() >= 0


@pytest.mark.parametrize('ci', range(len(GOLD)))
def test_golden_case(expert, ci):
    m, g = GOLD[ci]
    s = expert.samples_from_schedules_team(g['grid'], g['goal'][None], [g['schedule']], DEV, keep_fp64_gso=True)
    assert s.input.shape == (m['T'], m['N'], 3, 11, 11) and s.target.dtype == torch.float32
    assert_case(s, 0, g['input'], g['GSO'], g['target'], float.fromhex(m['radius']), m['growth'])


def test_golden_cases_share_calls(expert):
    """Cases of one team size and map size in ONE call each, a map per case."""
    for group in ((0, 0), (1, 1, 1), (4, 4)):
        gs = [GOLD[c] for c in group]
        s = expert.samples_from_schedules_team(np.stack([g['grid'] for _, g in gs]), np.stack([g['goal'] for _, g in gs]),
                                               [g['schedule'] for _, g in gs], DEV, keep_fp64_gso=True)
        for c, (m, g) in enumerate(gs):
            assert_case(s, c, g['input'], g['GSO'], g['target'], float.fromhex(m['radius']), m['growth'])


def _random_cases(N, H, W, cases, cap):
    rng = np.random.default_rng(1000 * N + W)
    made = [ec.random_case(rng, N, H, W, density=0.08, wait=0.2, max_steps=int(rng.integers(3, cap + 1)))
            for _ in range(cases)]
    return made, [ec.schedule_of(paths, goal) for _, goal, paths in made]


@pytest.mark.parametrize('N,H,W,cases,cap', [(129, 40, 40, 4, 8), (160, 64, 64, 4, 8), (384, 100, 100, 3, 5),
                                             (1024, 128, 128, 2, 4), (300, 256, 255, 2, 4)])
def test_random_cases_against_restatement(expert, N, H, W, cases, cap):
    """256 x 255 is the cell limit of the LDS occupancy grid (and a map whose rows are not 16-byte multiples)."""
    made, sched = _random_cases(N, H, W, cases, cap)
    s = expert.samples_from_schedules_team(np.stack([g for g, _, _ in made]), np.stack([g for _, g, _ in made]), sched,
                                           DEV, keep_fp64_gso=True)
    assert len(s) == sum(len(x) for x in sched)
    for c, (grid, goal, _) in enumerate(made):
        want = ec.reference_samples(grid, goal, sched[c])
        assert_case(s, c, want['input'], want['GSO'], want['target'], want['radius'], want['growth'])


@pytest.mark.parametrize('N,side,cases,cap', [(3, 20, 6, 20), (128, 40, 6, 20)])
def test_same_bytes_as_the_one_wave_call(expert, N, side, cases, cap):
    made, sched = _random_cases(N, side, side, cases, cap)
    args = (np.stack([g for g, _, _ in made]), np.stack([g for _, g, _ in made]), sched, DEV)
    team = expert.samples_from_schedules_team(*args, keep_fp64_gso=True)
    wave = expert.samples_from_schedules(*args, keep_fp64_gso=True)
    for k in FIELDS:
        assert torch.equal(getattr(team, k), getattr(wave, k)), k
    want = ec.reference_samples(made[0][0], made[0][1], sched[0])
    assert_case(team, 0, want['input'], want['GSO'], want['target'], want['radius'], want['growth'])


def test_bad_schedule_names_its_case(expert):
    from gnn_pathplanning_amd._native import GnnppError
    m, g = GOLD[0]
    bad = g['schedule'].copy()
    bad[2, 150] = bad[1, 150] + [0, 2]
    with pytest.raises(GnnppError, match=r'case 1 \(of 3\).*not one of the five actions'):
        expert.samples_from_schedules_team(g['grid'], np.stack([g['goal']] * 3), [g['schedule'], bad, g['schedule']], DEV)
    off = g['schedule'].copy()
    off[0, 159] = [64, 0]
    with pytest.raises(GnnppError, match=r'case 0 \(of 1\).*off the map'):
        expert.samples_from_schedules_team(g['grid'], g['goal'][None], [off], DEV)
    with pytest.raises(GnnppError, match='not supported'):                       # more than 65 536 cells
        expert.samples_from_schedules_team(np.zeros((256, 257), np.uint8), g['goal'][None], [g['schedule']], DEV)


def _device_inputs(cases):
    gs = [GOLD[c][1] for c in cases]
    dev = torch.device(DEV)
    grid = torch.from_numpy(np.stack([g['grid'] for g in gs])).to(dev)
    goal = torch.from_numpy(np.stack([g['goal'] for g in gs])).to(dev)
    pos = torch.from_numpy(np.concatenate([g['schedule'] for g in gs])).to(dev)
    bounds = np.cumsum([0] + [len(g['schedule']) for g in gs]).tolist()
    start = torch.tensor(bounds, dtype=torch.int32, device=dev)
    return grid, goal, pos, start, bounds


def _empty_out(expert, T, N, C, bounds, fp64=True):
    dev = torch.device(DEV)

    def f(*shape, dtype=torch.float32):
        return torch.full(shape, -7, dtype=dtype, device=dev)
    return expert.ScheduleSamples(input=f(T, N, 3, 11, 11), GSO=f(T, N, N),
                                  GSO64=f(T, N, N, dtype=torch.float64) if fp64 else None,
                                  target=f(T, N, 5), radius=f(C, dtype=torch.float64),
                                  growth=f(C, dtype=torch.int32), status=f(C, dtype=torch.int32),
                                  step_growth=f(T, dtype=torch.int32), bounds=bounds,
                                  workspace=f(T * N, dtype=torch.float64))


def test_graph_capture_and_side_stream_give_the_same_bytes(expert):
    cases = (0, 0, 0)
    grid, goal, pos, start, bounds = _device_inputs(cases)
    T, N, C = bounds[-1], 160, len(cases)
    plain = _empty_out(expert, T, N, C, bounds)
    expert.enqueue_schedule_team_samples(grid, goal, pos, start, plain)
    torch.cuda.synchronize()
    m, g = GOLD[0]
    plain.step_growth &= 0xffff
    for c in range(C):
        assert_case(plain, c, g['input'], g['GSO'], g['target'], float.fromhex(m['radius']), m['growth'])

    side_out = _empty_out(expert, T, N, C, bounds)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        expert.enqueue_schedule_team_samples(grid, goal, pos, start, side_out)
    side.synchronize()

    graphed = _empty_out(expert, T, N, C, bounds)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        expert.enqueue_schedule_team_samples(grid, goal, pos, start, graphed)
    torch.cuda.synchronize()
    assert (graphed.input == -7).all()                  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    side_out.step_growth &= 0xffff
    graphed.step_growth &= 0xffff
    for other in (side_out, graphed):
        for k in FIELDS:
            assert torch.equal(getattr(plain, k), getattr(other, k)), k
    # a second replay on cleared outputs writes the same bytes again
    graphed.input.fill_(-7)
    graphed.GSO.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.input, plain.input) and torch.equal(graphed.GSO, plain.GSO)


def test_graphs_beyond_2_to_the_31_elements(expert):
    """The 3-step 1024-agent golden case 700 times as 700 cases of one call: T_total = 2100, S has 2.2e9 elements
    (8.8 GB), the observations 3.1 GB; every copy compared on the device."""
    m, g = GOLD[4]
    assert m['N'] == 1024 and m['T'] == 3
    copies, N, T1 = 700, 1024, 3
    T = copies * T1
    assert T * N * N > 2 ** 31
    dev = torch.device(DEV)
    grid = torch.from_numpy(g['grid']).to(dev)
    goal = torch.from_numpy(g['goal']).to(dev)[None].expand(copies, N, 2).contiguous()
    pos = torch.from_numpy(g['schedule']).to(dev).repeat(copies, 1, 1)
    bounds = list(range(0, T + 1, T1))
    start = torch.tensor(bounds, dtype=torch.int32, device=dev)
    out = _empty_out(expert, T, N, copies, bounds, fp64=False)
    expert.enqueue_schedule_team_samples(grid, goal, pos, start, out)
    torch.cuda.synchronize()
    assert (out.status == 0).all() and (out.growth == m['growth']).all()
    assert (out.radius == float.fromhex(m['radius'])).all()
    want = [torch.from_numpy(a).to(dev) for a in (g['GSO'].astype(np.float32), g['input'].astype(np.float32),
                                                  g['target'].astype(np.float32))]
    chunk = 20                                          # copies per comparison
    for a in range(0, copies, chunk):
        for got, w in zip((out.GSO, out.input, out.target), want):
            view = got[a * T1:(a + chunk) * T1].view(chunk, *w.shape)
            assert bool((view == w).all()), a
    del out, want, pos, goal
    torch.cuda.empty_cache()


def test_rollout_to_train_step_with_160_agents(expert):
    """The loop the call closes, on 64 x 64 maps: BatchedRollout of an untrained policy (4 steps: nobody arrives) ->
    solve_failures (mapf.solve_team) -> samples_from_solutions(team=True) -> every solved case's tensors equal the
    restatement's of sol.schedule(c) -> SamplePool -> one train_step with a finite loss.  Seed 31: the host yardstick
    tests/mapf_cases.py::solve_case solves the episodes this rollout leaves (checked on the CPU with
    oracle/rollout_oracle.py + oracle/policy_oracle.py driving the same policy)."""
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from gnn_pathplanning_amd.rollout import BatchedRollout
    from gnn_pathplanning_amd.training import train_step
    from oracle import policy_oracle as orc
    dev = torch.device(DEV)
    B, N, side = 2, 160, 64
    cases = mc.random_cases(np.random.default_rng(31), B, N, side, density=0.1)
    grids, starts, goals = (np.stack([c[k] for c in cases]) for k in range(3))

    class Cfg:
        num_agents, nGraphFilterTaps, device = N, 3, dev
    net = DecentralPlannerNet(Cfg()).to(dev)
    net.load_state_dict(orc.init_state_dict(3, seed=7))
    ro = BatchedRollout(grids, starts, goals, 4, dev, tie_mode='lowest')
    res = ro.run(net.eval())
    assert not res['success'].any() and res['done'].all()
    sol = expert.solve_failures(ro, results=res)
    assert sol.episodes.tolist() == [0, 1]
    samples, ids = expert.samples_from_solutions(sol, grids, goals, team=True)
    assert len(ids) >= 1
    pos = res['positions'].numpy()
    for k, c in enumerate(ids):
        sched = sol.schedule(c)
        assert np.array_equal(sched[0], pos[c]) and np.array_equal(sched[-1], goals[c])
        want = ec.reference_samples(grids[c], goals[c], sched)
        assert_case(samples, k, want['input'], want['GSO'], want['target'], want['radius'], want['growth'])
    pool = expert.SamplePool()
    pool.append(samples)
    assert len(pool) == len(samples) == sum(len(sol.schedule(c)) for c in ids)
    inp, tgt, gso = pool.draw(4, torch.Generator(device=dev).manual_seed(3))
    assert inp.shape == (4, N, 3, 11, 11) and tgt.shape == (4, N, 5) and gso.shape == (4, N, N)
    opt = torch.optim.Adam(net.train().parameters(), lr=1e-3)
    loss = train_step(net, opt, inp, tgt, gso).item()
    assert np.isfinite(loss) and loss > 0
