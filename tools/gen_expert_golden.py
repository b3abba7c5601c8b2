"""Record what the REAL reference transformer makes of synthetic solved cases into tests/golden/expert_schedules.npz.

Build-container only: it imports the reference tree (onlineExpert/DataTransformer_local_onlineExpert.py, the
simulator's save_failure_cases) the way oracle/gen_golden_rollout.py does.  Only data is stored: per case the inputs
(map, goals, the failure-case YAML and the solver's YAML as bytes) and the reference's outputs (schedule, inputTensor
as uint8, GSO float64, target, final radius, times the radius grew).

    python tools/gen_expert_golden.py

Every graph the reference's eigenvalue test (graphTools.isConnected) sees is also put through the graph search the
kernels and tests/expert_cases.py use; the two must agree, so no case has to be left out of any test.
Case 0 also carries a rollout to start from: the positions its schedule starts at are where a team that only ever
moves "up" (a policy whose action head is all zero: every logit equal, first maximum wins) stands after `maxstep`
steps from `rollout_start`, computed with oracle/rollout_oracle.py.
"""
import json
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import expert_cases as ec  # noqa: E402
from oracle.gen_golden_rollout import REF  # noqa: E402  (where the reference tree lies)
from oracle import rollout_oracle as ro  # noqa: E402

# (N, map side, obstacle density, wait probability, box, longest path kept)
SPECS = ((10, 20, 0.10, 0.0, None, None),       # 0: the end-to-end case (starts where a rollout ended)
         (2, 50, 0.05, 0.1, None, 25),          # 1: two agents far apart: the radius grows >= 10 times
         (5, 20, 0.05, 0.2, (6, 6, 5), None),   # 2: a team that stays together: never grows, goals in each other's view
         (24, 50, 0.10, 0.1, None, 20),
         (24, 20, 0.15, 0.1, None, 12),
         (5, 50, 0.10, 0.1, None, 25),
         (10, 50, 0.05, 0.4, None, 25),         # 6: many waits: agents arrive at very different times
         (2, 20, 0.10, 0.0, None, 3))           # 7: three steps
ROLLOUT_MAXSTEP = 6


def import_reference():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import matplotlib
    matplotlib.use('Agg')
    easydict = types.ModuleType('easydict')

    class EasyDict(dict):
        __getattr__ = dict.__getitem__
    easydict.EasyDict = EasyDict
    hashids = types.ModuleType('hashids')
    hashids.Hashids = object
    sys.modules['easydict'], sys.modules['hashids'] = easydict, hashids
    for name, path in (('utils', REF + '/utils'), ('utils.graphUtils', REF + '/utils/graphUtils'),
                       ('dataloader', REF + '/dataloader'), ('onlineExpert', REF + '/onlineExpert')):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    import onlineExpert.DataTransformer_local_onlineExpert as tr
    import utils.multirobotsim_dcenlocal_onlineExpert as sim
    return tr, sim, easydict.EasyDict


def reference_failure_yaml(sim, tmp, grid, positions, goals, case_id):
    """multiRobotSim.save_failure_cases itself, on the state the simulator holds when an episode has ended."""
    s = types.SimpleNamespace()
    s.failureCases_input = tmp
    s.ID_dataset = case_id
    channel = torch.from_numpy(grid.astype(np.float32))
    s.posObstacle = sim.multiRobotSim.findpos(s, channel)
    s.numObstacle = s.posObstacle.shape[0]
    s.size_map = channel.shape
    s.config = types.SimpleNamespace(num_agents=len(positions))
    s.status_MultiAgent = {'agent%d' % n: {'goal': torch.tensor(np.array([goals[n]]), dtype=torch.float32),
                                           'nextState_predict': torch.tensor(np.array([positions[n]]), dtype=torch.float32)}
                           for n in range(len(positions))}
    sim.multiRobotSim.save_failure_cases(s)
    with open(os.path.join(tmp, 'failureCases_ID{:05d}.yaml'.format(case_id)), 'rb') as f:
        return f.read()


def main():
    tr, sim, EasyDict = import_reference()
    rng = np.random.default_rng(20261016)
    graph = tr.graph
    real_is_connected = graph.isConnected
    seen = {'graphs': 0, 'disconnected': 0}

    def checked_is_connected(W):
        ref = bool(real_is_connected(W))
        assert ref == ro._connected(W), 'graph search and the eigenvalue test disagree'
        seen['graphs'] += 1
        seen['disconnected'] += not ref
        return ref
    graph.isConnected = checked_is_connected

    store, meta, spent, nsamples = {}, [], 0.0, 0
    for ci, (N, side, dens, wait, box, cap) in enumerate(SPECS):
        rollout_start = None
        while True:
            grid, starts, goals = ec.random_map(rng, N, side, side, dens, box)
            if ci == 0:
                ep = ro.EpisodeState(grid, goals, starts, ROLLOUT_MAXSTEP)
                for t in range(1, ROLLOUT_MAXSTEP + 1):
                    ro.loop_step(ep, [0] * N, t, lambda c: c[0])
                if all(ep.reached):
                    continue
                rollout_start, starts = starts, ep.cur.copy()
            paths = ec.expert_paths(rng, grid, starts, goals, wait, cap)
            if paths is not None and 3 <= max(len(p) for p in paths) <= 25:
                break
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, 'input'))
            os.makedirs(os.path.join(tmp, 'output_ECBS'))
            fail_yaml = reference_failure_yaml(sim, os.path.join(tmp, 'input'), grid, starts, goals, ci)
            sol_yaml = ec.solution_yaml(paths).encode()
            with open(os.path.join(tmp, 'output_ECBS', 'failureCases_ID{:05d}.yaml'.format(ci)), 'wb') as f:
                f.write(sol_yaml)
            cfg = EasyDict({'num_agents': N, 'map_w': side, 'map_h': side, 'failCases_dir': tmp + '/', 'exp_net': 'dcp'})
            t0 = time.perf_counter()
            dt = tr.DataTransformer(cfg)
            dt.set_up('1')
            (state, target), goal_ref, makespan, map_ref, _ = dt.load_ExpertSolution(0)
            before = seen['disconnected']
            gso, radius = dt.computeAdjacencyMatrix(state, dt.communicationRadius)
            growth = seen['disconnected'] - before
            dt.AgentState.setmap(map_ref)
            obs = dt.AgentState.toSeqInputTensor(goal_ref, state, makespan + 1).numpy()
            spent += time.perf_counter() - t0
        nsamples += state.shape[0] * N
        assert np.array_equal(map_ref, grid) and np.array_equal(goal_ref, goals)
        assert np.array_equal(state, ec.schedule_of(paths, goals))
        assert np.array_equal(obs, obs.astype(np.uint8)) and obs.shape == (makespan + 1, N, 3, 11, 11)
        pre = 'c%d_' % ci
        store[pre + 'grid'] = grid.astype(np.uint8)
        store[pre + 'goal'] = goals.astype(np.int32)
        store[pre + 'failure_yaml'] = np.frombuffer(fail_yaml, dtype=np.uint8)
        store[pre + 'solution_yaml'] = np.frombuffer(sol_yaml, dtype=np.uint8)
        store[pre + 'schedule'] = state.astype(np.int32)
        store[pre + 'input'] = obs.astype(np.uint8)
        store[pre + 'GSO'] = gso
        store[pre + 'target'] = target.astype(np.uint8)
        if rollout_start is not None:
            store[pre + 'rollout_start'] = rollout_start.astype(np.int32)
        meta.append({'N': N, 'H': side, 'W': side, 'T': int(state.shape[0]), 'radius': float(radius).hex(),
                     'growth': int(growth), 'path_lengths': [len(p) for p in paths],
                     'rollout_maxstep': ROLLOUT_MAXSTEP if rollout_start is not None else None})
        print('case %d: N %d, %dx%d, %d steps, radius %.4f after %d growths' % (ci, N, side, side, state.shape[0],
                                                                              radius, growth))
    assert any(m['growth'] == 0 for m in meta) and any(m['growth'] >= 10 for m in meta)
    store['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, 'tests', 'golden', 'expert_schedules.npz')
    np.savez_compressed(path, **store)
    print('wrote %s (%d bytes); %d graphs checked against the eigenvalue test' % (path, os.path.getsize(path),
                                                                               seen['graphs']))
    print('reference transformer on this CPU (one process, files on tmpfs included): %d agent-samples in %.3f s = '
          '%.0f agent-samples/s' % (nsamples, spent, nsamples / spent))


if __name__ == '__main__':
    main()
