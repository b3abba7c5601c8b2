"""GPU (-m gpu): BatchedRollout(record=...) -- the trace of a rollout on the device.  Against the real simulator's traces
(the reference's own path_predict and actions), across the rollout's routes, against an unrecorded twin (the behaviour
before recording existed), the frozen-episode rule against the sequential oracle, the team-size edges, the audit chain and
the files.  Every comparison is exact equality of integers."""
import ctypes
import os

import numpy as np
import pytest
import torch

import rollout_trace_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


def host(trace):
    torch.cuda.synchronize(trace.device)
    return {k: getattr(trace, k).cpu().numpy() for k in ('path', 'action', 'moves', 'shielded', 'steps', 'seen_done')}


def _all_golden():
    from conftest import _load
    return [(name,) + _load(name + '.npz') for name in ('rollout_traces', 'rollout_traces_large', 'rollout_traces_team')]


@pytest.fixture(scope='module')
def replays(dev):
    """Every golden trace replayed ONCE with record=True, the way tests/test_gpu_rollout.py drives them (tie_mode='replay',
    the golden logits and choices per step): [(file, case index, meta, z, rollout)]."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    out = []
    for name, z, meta in _all_golden():
        for ci, m in enumerate(meta):
            pos_all = z['t%d_pos' % ci].astype(np.int64)
            env = BatchedRollout(z['t%d_grid' % ci], pos_all[0][None], z['t%d_goal' % ci][None], m['maxstep'], dev,
                                 commR=m['commR'], tie_mode='replay', record=True)
            assert env.trace.T_cap == m['maxstep']
            used = 0
            for t in range(m['T']):
                nch = int(z['t%d_nchoices' % ci][t])
                ch = torch.zeros(1, max(nch, 1), dtype=torch.int16)
                ch[0, :nch] = torch.from_numpy(z['t%d_choices' % ci][used:used + nch].astype(np.int16))
                used += nch
                env.move(logits=torch.from_numpy(z['t%d_logits' % ci][t]).unsqueeze(1).to(dev), choices=ch)
            out.append((name, ci, m, z, env))
    return out


def test_trace_of_the_real_simulators_traces(replays):
    """Rows 0 .. T of path = the golden pos, action = the golden actions, steps = T, moves and shielded = what numpy counts
    from pos and actions -- all independent of the code under test."""
    assert sorted({m['N'] for _, _, m, _, _ in replays}) == [2, 6, 10, 12, 23, 50, 100, 160, 256]
    for name, ci, m, z, env in replays:
        want = tc.golden_expectation(z, ci, m)
        assert want['steps'].tolist() == [m['T']]
        tc.assert_trace_equals(host(env.trace), want, m['T'], what=(name, ci))
        assert np.array_equal(env.trace.schedule(0), z['t%d_pos' % ci].astype(np.int64))
    assert sum(int(tc.golden_expectation(z, ci, m)['shielded'].sum()) for _, ci, m, z, _ in replays) > 0


def test_audit_chain_on_the_replays(dev, replays):
    """trace.audit(): no STATE, MOVE or BAD_START bit (the move rule forbids all three); vertex and swap counts are numpy's
    from the golden pos (not assumed zero); mapf.audit on trace.schedule(b) gives the same record."""
    from gnn_pathplanning_amd import mapf
    seen = 0
    for name, ci, m, z, env in replays:
        a = env.trace.audit()
        torch.cuda.synchronize(dev)
        status, counts = int(a.status[0]), a.counts[0].cpu().tolist()
        assert status & (mapf.AUDIT_STATE | mapf.AUDIT_MOVE | mapf.AUDIT_BAD_START) == 0, (name, ci, a.describe(0))
        vertex, swap = tc.golden_conflicts(z, ci, m)
        assert counts == [0, vertex, 0, swap], (name, ci, counts, vertex, swap)
        seen += vertex + swap
        b = mapf.audit(z['t%d_grid' % ci], z['t%d_pos' % ci][0][None], z['t%d_goal' % ci][None], [env.trace.schedule(0)], dev)
        for k in ('status', 'arrival', 'makespan', 'flowtime', 'counts', 'first'):
            assert torch.equal(getattr(a, k), getattr(b, k)), (name, ci, k)
    print('conflicts left after shielding in the golden traces: %d' % seen)


def _golden_planner(dev, policy_golden, N, K=3, route=None):
    from conftest import golden_state_dict
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    z, _ = policy_golden

    class Cfg:
        num_agents, nGraphFilterTaps, device = N, K, dev
    if route:
        Cfg.largeGraphFilter = route
    sd = golden_state_dict(z, 3)
    if K == 5:          # the golden taps of K = 2 and K = 3 side by side: outside the one-launch step's K = 2 .. 4
        sd['GFL.0.weight'] = torch.cat([torch.from_numpy(np.array(z['gfl_w_K2'])), sd['GFL.0.weight']], 2)
    net = DecentralPlannerNet(Cfg()).to(dev).eval()
    net.load_state_dict(sd)
    return net


def _golden_episodes(rollout_golden):
    """3 episodes of 10 agents on the 20 x 20 golden map: the starts and goals of the two 10-agent traces, and the first
    one's reversed."""
    z, meta = rollout_golden
    assert (meta[0]['N'], meta[0]['W'], meta[1]['N'], meta[1]['W']) == (10, 20, 10, 20)
    grid = z['t0_grid']
    s0, g0 = z['t0_pos'][0].astype(np.int64), z['t0_goal'].astype(np.int64)
    s1, g1 = z['t1_pos'][0].astype(np.int64), z['t1_goal'].astype(np.int64)
    ok = lambda p: (grid[p[:, 0], p[:, 1]] == 0).all()                                   # noqa: E731
    if not (ok(s1) and ok(g1)):
        s1, g1 = s0[::-1].copy(), g0[::-1].copy()
    return grid, np.stack([s0, s1, g0]), np.stack([g0, g1, s0])


def _twin_rows(env, drive, T):
    """An unrecorded rollout stepped one step at a time with pos and done read back after each: the behaviour before
    recording existed.  -> rows [T+1,B,N,2], done_after [T,B], and the logits [T,N,B,5] the one-launch step left (None on
    the other routes)."""
    assert env.trace is None
    rows, done, logits = [env.pos.cpu().numpy().copy()], [], []
    for t in range(T):
        drive(env, t)
        rows.append(env.pos.cpu().numpy().copy())
        done.append(env.done.cpu().numpy().copy())
        if env._logits is not None:
            logits.append(env._logits.cpu().numpy().copy())
    return np.stack(rows), np.stack(done), np.stack(logits) if len(logits) == T else None


@pytest.mark.parametrize('graph', ['dense', 'lists'])
def test_routes_agree(dev, rollout_golden, policy_golden, graph):
    """One 10-agent model rollout of 3 episodes recorded by steps(model, n) (dense: the traced burst of the one-launch
    step), by step(model) one step at a time, and read back from an unrecorded twin: byte for byte the same.  'lists': the
    one-launch step reads the dense GSO and a lists rollout refuses a planner that qualifies for it, so the lists planner
    carries K = 5 taps (the golden K = 2 and K = 3 taps side by side)."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    grid, starts, goals = _golden_episodes(rollout_golden)
    T = 9
    net = _golden_planner(dev, policy_golden, 10) if graph == 'dense' else \
        _golden_planner(dev, policy_golden, 10, K=5, route='lists')
    make = lambda **kw: BatchedRollout(grid, starts, goals, [6, 30, 30], dev, graph=graph, **kw)      # noqa: E731
    with torch.no_grad():
        burst, single, twin = make(record=12), make(record=12), make()
        burst.steps(net, T)
        for _ in range(T):
            single.step(net)
        rows, done_after, logits = _twin_rows(twin, lambda env, t: env.step(net), T)
    a, b = host(burst.trace), host(single.trace)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.array_equal(a['path'][:, :T + 1].transpose(1, 0, 2, 3), rows)
    frozen = tc.frozen_at_entry(done_after != 0, [6, 30, 30])
    asked = np.where(frozen[:, :, None], 4, a['action'][:, :T].transpose(1, 0, 2))     # (the yardstick skips frozen steps)
    if graph == 'dense':                       # the one-launch step ran, and the twin's logits say what was asked
        assert burst._logits is not None and single._logits is not None and logits is not None
        asked = tc.first_max(logits).transpose(0, 2, 1)                                 # [T,N,B] -> [T,B,N]
    want = tc.record_rule(rows, asked, frozen, T_cap=12)
    tc.assert_trace_equals(a, want, T, what=graph)
    assert a['steps'][0] <= 6 and (a['action'][:, :T][~frozen.T] >= 0).all() and a['moves'].sum() > 0
    for k in ('pos', 'reached', 'done', 'flags', 'obs'):
        assert torch.equal(getattr(burst, k), getattr(twin, k)) and torch.equal(getattr(single, k), getattr(twin, k)), k


@pytest.mark.parametrize('N,W', [(10, 20), (50, 32), (160, 40)])
def test_recording_changes_nothing(dev, policy_golden, N, W):
    """results(), pos, obs, S and flags of a recorded rollout equal its unrecorded twin's: the one-launch step (N = 10), the
    split simulator launches (N = 50) and the team kernels (N = 160); and N = 160 on neighbour lists."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    from rollout_team_cases import make_instances
    grids, starts, goals = make_instances(np.random.default_rng(N), 3, N, W, W, 0.05)
    for graph in ('dense',) + (('lists',) if N == 160 else ()):
        net = _golden_planner(dev, policy_golden, N, route='lists' if graph == 'lists' else None)
        with torch.no_grad():
            envs = [BatchedRollout(grids, starts, goals, [4, 20, 20], dev, tie_mode='mt19937', seed=5, graph=graph, record=r)
                    for r in (True, False)]
            for env in envs:
                if env.lists is not None:
                    env.lists.zero_()                            # (the block is written only where a graph has neighbours)
                env.steps(net, 6)
        res = [env.results() for env in envs]
        for k in res[0]:
            assert res[0][k] == res[1][k] if k == 'steps' else torch.equal(res[0][k], res[1][k]), (graph, k)
        for k in ('pos', 'obs', 'S', 'lists', 'flags', 'rng_cursor', 'radius'):
            x, y = getattr(envs[0], k), getattr(envs[1], k)
            assert (x is None and y is None) or torch.equal(x, y), (graph, k)
        got = host(envs[0].trace)
        assert got['steps'].tolist() == [min(4, int(got['steps'][0])), 6, 6] and np.array_equal(got['path'][:, 6], res[1]['positions'].numpy())


def _drive_actions(case):
    acts = torch.from_numpy(np.ascontiguousarray(case['actions']))
    return lambda env, t: env.move(actions=acts[t].to(env.device))


def test_frozen_episodes(dev):
    """B = 4, maxstep = [3, 7, 12, 12]; one episode starts on its goals, one never arrives; 12 steps.  steps, rows, actions
    and counters are the yardstick's from the sequential ORACLE's trace; rows after steps[b] repeat row steps[b], their
    action is -1; record=5 raises at step 6 with nothing changed; poison beyond T_cap in an over-allocated buffer stays."""
    import rollout_cases as rc
    from gnn_pathplanning_amd import _native
    from gnn_pathplanning_amd.rollout import BatchedRollout
    case = tc.frozen_case()
    oracle = rc.oracle_trace(case)
    T, B, N = case['actions'].shape
    rows = np.concatenate([case['starts'][None], oracle['pos']], 0)
    want = tc.record_rule(rows, case['actions'], tc.frozen_at_entry(oracle['done'], case['maxstep']))
    assert want['steps'].tolist() == [3, 7, 2, 12]
    drive = _drive_actions(case)
    make = lambda **kw: BatchedRollout(case['grids'], case['starts'], case['goals'], case['maxstep'], dev, **kw)   # noqa: E731
    env = make(record=True)
    assert env.trace.T_cap == 12
    for t in range(T):
        drive(env, t)
    got = host(env.trace)
    tc.assert_trace_equals(got, want, T, what=case['name'])
    for b in range(B):
        s = int(got['steps'][b])
        assert (got['path'][b, s:] == got['path'][b, s]).all() and (got['action'][b, s:] == -1).all()
    with pytest.raises(_native.GnnppError, match='beyond the trace'):
        drive(env, 0)                                            # step 13 of a trace of 12
    # record=5: step 6 raises before anything is enqueued; neither the trace nor the episode has changed
    short = make(record=5)
    for t in range(5):
        drive(short, t)
    before = host(short.trace), short.pos.cpu().numpy().copy(), short.t
    with pytest.raises(_native.GnnppError, match='step 6 is beyond the trace'):
        drive(short, 5)
    after = host(short.trace)
    assert all(before[0][k].tobytes() == after[k].tobytes() for k in after)
    assert np.array_equal(short.pos.cpu().numpy(), before[1]) and short.t == before[2] == 5
    assert np.array_equal(after['path'], got['path'][:, :6])
    with pytest.raises(_native.GnnppError, match='in order'):
        make(record=5).move(actions=torch.zeros(B, N, dtype=torch.int32, device=dev), currentstep=3)
    # the C calls behind an unrecorded rollout, into over-allocated poisoned buffers with T_cap = 12
    plain = make()
    lib = _native.lib()
    extra = 3
    path = torch.full((B * 13 * N * 2 + extra * N * 2,), tc.POISON, dtype=torch.int32, device=dev)
    action = torch.full((B * 12 * N + extra * N,), 0x5a, dtype=torch.int8, device=dev)
    small = [torch.full((n + 1,), tc.POISON, dtype=torch.int32, device=dev) for n in (B * N, B * N, B, B)]
    s = _native.RolloutTraceStruct()
    s.path, s.action, s.T_cap = path.data_ptr(), action.data_ptr(), 12
    s.moves, s.shielded, s.steps, s.seen_done = (x.data_ptr() for x in small)
    st = _native.stream_ptr(dev)
    assert lib.gnnpp_rollout_trace_begin(ctypes.byref(plain._r), ctypes.byref(s), st) == 0
    for t in range(T):
        drive(plain, t)
        assert lib.gnnpp_rollout_trace_record(ctypes.byref(plain._r), ctypes.byref(s), st) == 0
    torch.cuda.synchronize(dev)
    assert np.array_equal(path[:B * 13 * N * 2].cpu().numpy().reshape(B, 13, N, 2), got['path'])
    assert np.array_equal(action[:B * 12 * N].cpu().numpy().reshape(B, 12, N), got['action'])
    assert (path[B * 13 * N * 2:] == tc.POISON).all() and (action[B * 12 * N:] == 0x5a).all()
    assert all(int(x[-1]) == tc.POISON for x in small)
    for x, k in zip(small, ('moves', 'shielded', 'steps', 'seen_done')):
        assert np.array_equal(x[:-1].cpu().numpy().reshape(got[k].shape), got[k]), k
    rc_step13 = plain._r.currentstep
    plain._r.currentstep = 13
    assert lib.gnnpp_rollout_trace_record(ctypes.byref(plain._r), ctypes.byref(s), st) == _native.ERR_ARG
    plain._r.currentstep = rc_step13


@pytest.mark.parametrize('ci', range(len(tc.EDGE_SHAPES)), ids=['%dx%d' % s[:2] for s in tc.EDGE_SHAPES])
def test_team_size_edges(dev, ci):
    """Hand-made action ids, 4 steps, against the read-back twin: N = 1, 128 | 129 (the seam between the one-wave and the
    team kernels) and 1024."""
    from gnn_pathplanning_amd.rollout import BatchedRollout
    case = tc.edge_cases()[ci]
    drive = _drive_actions(case)
    make = lambda **kw: BatchedRollout(case['grids'], case['starts'], case['goals'], case['maxstep'], dev, **kw)   # noqa: E731
    rows, done_after, _ = _twin_rows(make(), drive, 4)
    want = tc.record_rule(rows, case['actions'], tc.frozen_at_entry(done_after != 0, case['maxstep']), T_cap=50)
    env = make(record=True)
    for t in range(4):
        drive(env, t) if t % 2 else env.move_and_observe(actions=torch.from_numpy(case['actions'][t]).to(dev))
    got = host(env.trace)
    tc.assert_trace_equals(got, want, 4, what=case['name'])
    assert got['action'][0, 1, 0] == 7 and got['shielded'].sum() > 0 and got['moves'].sum() > 0


def test_grouped_rollout_trace_and_files(dev, rollout_golden, policy_golden, tmp_path):
    """GroupedRollout passes record on: its trace is the one-batch trace, episode for episode.  write_prediction_cases
    writes the predicted schedule next to the input file of the original starts; every row of the file is the trace's, the
    statistics are results()'s, and expert.read_solution reads the pair back: trace.schedule(b) up to the makespan the file
    states (the reference's loader takes its length from `statistics.makespan`, and a rollout's makespan runs from the first
    asked move to the last arrival -- the rows behind it are in the file and compared here directly)."""
    import yaml
    from gnn_pathplanning_amd import expert
    from gnn_pathplanning_amd.rollout import BatchedRollout, GroupedRollout
    grid, starts, goals = _golden_episodes(rollout_golden)
    net = _golden_planner(dev, policy_golden, 10)
    limits = [6, 30, 30]
    with torch.no_grad():
        one = BatchedRollout(grid, starts, goals, limits, dev, record=True)
        res_one = one.run(net, check_every=4)
        many = GroupedRollout(grid, starts, goals, limits, dev, groups=2, record=True)
        res = many.run(net, check_every=4)
    a, b = host(one.trace), host(many.trace)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert many.trace.T_cap == 30 and all(e.trace.T_cap == 30 for e in many.envs)
    trace = many.trace
    written = expert.write_prediction_cases(str(tmp_path), many, ids=[7, 8, 9], results=res)
    assert [w[0] for w in written] == [0, 1, 2]
    full = 0
    for bi, inp, pred in written:
        mode = 'success' if bool(res['success'][bi]) else 'failure'
        assert inp == os.path.join(str(tmp_path), 'input', '%sCases_ID%05d.yaml' % (mode, 7 + bi))
        assert pred == os.path.join(str(tmp_path), 'predict_' + mode, '%sCases_ID%05d.yaml' % (mode, 7 + bi))
        assert open(pred).read() == trace.prediction_yaml(bi)
        doc = yaml.safe_load(open(pred))
        assert doc['statistics'] == {'cost': int(res['flowtime'][bi]), 'makespan': int(res['makespan'][bi]),
                                     'succeed': int(res['success'][bi])}
        sched = trace.schedule(bi)
        assert sched.shape == (int(a['steps'][bi]) + 1, 10, 2) and sched.dtype == np.int64
        for n in range(10):
            plan = doc['schedule']['agent%d' % n]
            assert [(p['x'], p['y'], p['t']) for p in plan] == [(int(x), int(y), t) for t, (x, y) in enumerate(sched[:, n])]
        g, gl, read = expert.read_solution(inp, pred)
        assert np.array_equal(g, grid) and np.array_equal(gl, goals[bi])
        assert np.array_equal(yaml.safe_load(open(inp))['agents'][3]['start'], starts[bi][3])
        rows = int(res['makespan'][bi]) + 1
        assert read.shape[0] == rows <= sched.shape[0] and np.array_equal(read, sched[:rows])
        full += int(rows == sched.shape[0])
    assert full >= 1                                            # an episode whose file reads back to ALL of trace.schedule(b)
    assert res_one['steps'] == res['steps']
