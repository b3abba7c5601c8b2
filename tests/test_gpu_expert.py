"""MI355X: gnnpp_schedule_samples through gnn_pathplanning_amd/expert.py -- the golden cases of the real reference,
random cases against the sequential numpy restatement (tests/expert_cases.py), graph capture and side streams, and the
whole loop rollout -> failure case -> solution -> samples -> pool -> train_step.  Equality everywhere: the work is on
integers, {0, 1} values and fp64 arithmetic the reference performs in a fixed order."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expert_cases as ec  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def expert():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from gnn_pathplanning_amd import _native, expert as ex
    _native.lib()
    return ex


GOLD = ec.load_golden()


def assert_case(s, c, want_input, want_gso64, want_target, radius, growth):
    a, b = s.bounds[c], s.bounds[c + 1]
    assert s.radius[c].item() == radius and s.growth[c].item() == growth
    assert torch.equal(s.input[a:b].cpu(), torch.from_numpy(np.asarray(want_input, dtype=np.float32)))
    assert torch.equal(s.target[a:b].cpu(), torch.from_numpy(np.asarray(want_target, dtype=np.float32)))
    assert torch.equal(s.GSO64[a:b].cpu(), torch.from_numpy(want_gso64))
    assert torch.equal(s.GSO[a:b].cpu(), torch.from_numpy(want_gso64.astype(np.float32)))
    assert s.step_growth[a:b].max().item() == growth and s.step_growth[a:b].min().item() >= 0


@pytest.mark.parametrize('ci', range(len(GOLD)))
def test_golden_case(expert, ci):
    m, g = GOLD[ci]
    s = expert.samples_from_schedules(g['grid'], g['goal'][None], [g['schedule']], DEV, keep_fp64_gso=True)
    assert s.input.shape == (m['T'], m['N'], 3, 11, 11) and s.target.dtype == torch.float32
    assert_case(s, 0, g['input'], g['GSO'], g['target'], float.fromhex(m['radius']), m['growth'])


def test_golden_cases_share_calls(expert):
    """Cases of one team size and map size in ONE call each, a map per case."""
    for pair in ((3,), (0, 0), (1,), (6, 6, 6)):
        gs = [GOLD[c] for c in pair]
        s = expert.samples_from_schedules(np.stack([g['grid'] for _, g in gs]), np.stack([g['goal'] for _, g in gs]),
                                          [g['schedule'] for _, g in gs], DEV, keep_fp64_gso=True)
        for c, (m, g) in enumerate(gs):
            assert_case(s, c, g['input'], g['GSO'], g['target'], float.fromhex(m['radius']), m['growth'])


@pytest.mark.parametrize('N,side,cases,cap', [(128, 40, 12, 30), (10, 20, 150, 40), (64, 50, 10, 25), (65, 28, 6, 20),
                                              (3, 230, 4, 30)])
def test_random_cases_against_restatement(expert, N, side, cases, cap):
    """Up to 128 agents and a few thousand steps in one call (150 cases of 10 agents: ~3000 steps); 230 x 230: the
    map leaves no LDS for the output stage."""
    rng = np.random.default_rng(1000 * N + side)
    made = [ec.random_case(rng, N, side, side, density=0.08, wait=0.2, max_steps=int(rng.integers(3, cap + 1)))
            for _ in range(cases)]
    sched = [ec.schedule_of(paths, goal) for _, goal, paths in made]
    s = expert.samples_from_schedules(np.stack([g for g, _, _ in made]), np.stack([g for _, g, _ in made]), sched, DEV,
                                      keep_fp64_gso=True)
    assert len(s) == sum(len(x) for x in sched)
    growths = set()
    for c, (grid, goal, _) in enumerate(made):
        want = ec.reference_samples(grid, goal, sched[c])
        assert_case(s, c, want['input'], want['GSO'], want['target'], want['radius'], want['growth'])
        growths.add(want['growth'])
    assert len(growths) > 1 or cases < 6


def test_bad_schedule_names_its_case(expert):
    from gnn_pathplanning_amd._native import GnnppError
    m, g = GOLD[2]
    bad = g['schedule'].copy()
    bad[2, 3] = bad[1, 3] + [0, 2]
    with pytest.raises(GnnppError, match=r'case 1 \(of 3\).*not one of the five actions'):
        expert.samples_from_schedules(g['grid'], np.stack([g['goal']] * 3), [g['schedule'], bad, g['schedule']], DEV)
    off = g['schedule'].copy()
    off[0, 0] = [20, 0]
    with pytest.raises(GnnppError, match=r'case 0 \(of 1\).*off the map'):
        expert.samples_from_schedules(g['grid'], g['goal'][None], [off], DEV)
    with pytest.raises(GnnppError):
        expert.samples_from_schedules(g['grid'], g['goal'][None, :1], [g['schedule'][:, :1]], DEV)      # one agent


def _device_inputs(cases):
    gs = [GOLD[c][1] for c in cases]
    dev = torch.device(DEV)
    grid = torch.from_numpy(np.stack([g['grid'] for g in gs])).to(dev)
    goal = torch.from_numpy(np.stack([g['goal'] for g in gs])).to(dev)
    pos = torch.from_numpy(np.concatenate([g['schedule'] for g in gs])).to(dev)
    bounds = np.cumsum([0] + [len(g['schedule']) for g in gs]).tolist()
    start = torch.tensor(bounds, dtype=torch.int32, device=dev)
    return grid, goal, pos, start, bounds


def _empty_out(expert, T, N, C, bounds):
    dev = torch.device(DEV)

    def f(*shape, dtype=torch.float32):
        return torch.full(shape, -7, dtype=dtype, device=dev)
    return expert.ScheduleSamples(input=f(T, N, 3, 11, 11), GSO=f(T, N, N), GSO64=f(T, N, N, dtype=torch.float64),
                                  target=f(T, N, 5), radius=f(C, dtype=torch.float64),
                                  growth=f(C, dtype=torch.int32), status=f(C, dtype=torch.int32),
                                  step_growth=f(T, dtype=torch.int32), bounds=bounds)


FIELDS = ('input', 'GSO', 'GSO64', 'target', 'radius', 'growth', 'status', 'step_growth')


def test_graph_capture_and_side_stream_give_the_same_bytes(expert):
    cases = (0, 0, 0)
    grid, goal, pos, start, bounds = _device_inputs(cases)
    T, N, C = bounds[-1], 10, len(cases)
    plain = _empty_out(expert, T, N, C, bounds)
    expert.enqueue_schedule_samples(grid, goal, pos, start, plain)
    torch.cuda.synchronize()
    m, g = GOLD[0]
    plain.step_growth &= 0xffff
    for c in range(C):
        assert_case(plain, c, g['input'], g['GSO'], g['target'], float.fromhex(m['radius']), m['growth'])

    side_out = _empty_out(expert, T, N, C, bounds)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        expert.enqueue_schedule_samples(grid, goal, pos, start, side_out)
    side.synchronize()

    graphed = _empty_out(expert, T, N, C, bounds)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        expert.enqueue_schedule_samples(grid, goal, pos, start, graphed)
    torch.cuda.synchronize()
    assert (graphed.input == -7).all()                  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    side_out.step_growth &= 0xffff
    graphed.step_growth &= 0xffff
    for other in (side_out, graphed):
        for k in FIELDS:
            assert torch.equal(getattr(plain, k), getattr(other, k)), k
    # a replay follows its inputs: the last case's steps cleared, the graph run again on the same buffers
    graphed.input.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.input, plain.input)


def test_rollout_to_train_step(expert, tmp_path):
    """rollout that fails -> failure-case file -> the solver's answer (golden) -> samples -> pool -> one train_step:
    the loss equals the loss of the same step fed with the REFERENCE's tensors from the golden file."""
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from gnn_pathplanning_amd.rollout import BatchedRollout
    from gnn_pathplanning_amd.training import train_step
    from oracle import policy_oracle as orc
    m, g = GOLD[0]
    dev = torch.device(DEV)

    class Cfg:
        num_agents, nGraphFilterTaps, device = m['N'], 3, dev

    def model(zero_head):
        net = DecentralPlannerNet(Cfg()).to(dev)
        net.load_state_dict(orc.init_state_dict(3, seed=7))
        if zero_head:                                   # every logit equal: the first action ("up") wins, always
            with torch.no_grad():
                net.actionsMLP[0].weight.zero_()
                net.actionsMLP[0].bias.zero_()
        return net

    ro = BatchedRollout(g['grid'], g['rollout_start'][None], g['goal'][None], m['rollout_maxstep'], dev, commR=6.0)
    res = ro.run(model(True).eval())
    assert not bool(res['success'][0]) and bool(res['done'][0])
    assert np.array_equal(res['positions'][0].numpy(), g['schedule'][0])
    (b, path), = expert.write_failure_cases(str(tmp_path), ro, ids=[0], results=res)
    assert open(path, 'rb').read() == bytes(g['failure_yaml'])
    grid, goal, schedule = expert.read_solution(path, bytes(g['solution_yaml']).decode())
    s = expert.samples_from_schedules(grid, goal[None], [schedule], dev)
    pool = expert.SamplePool()
    pool.append(s)
    batch = pool.draw(16, torch.Generator(device=dev).manual_seed(3))
    idx = torch.randperm(len(pool), generator=torch.Generator(device=dev).manual_seed(3), device=dev)[:16].cpu()
    ref = (torch.from_numpy(g['input']).float()[idx].to(dev), torch.from_numpy(g['target']).float()[idx].to(dev),
           torch.from_numpy(g['GSO']).float()[idx].to(dev))
    for got, want in zip(batch, ref):
        assert torch.equal(got, want)
    losses = []
    for inp, tgt, gso in (batch, ref):
        net = model(False).train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        losses.append(train_step(net, opt, inp, tgt, gso).item())
    assert np.isfinite(losses[0]) and losses[0] == losses[1]
