"""Record what the REAL reference transformer makes of synthetic solved cases of LARGE teams (130 ... 1024 agents) into
tests/golden/expert_schedules_team.npz: the yardstick of gnnpp_schedule_team_samples.

Build-container only, like tools/gen_expert_golden.py, whose reference import and file handling it uses: the
reference tree is imported at run time and only data is stored, under the same keys per case (no rollout_start).

    python tools/gen_expert_golden_team.py

Every graph the reference's eigenvalue test sees is also put through the graph search the kernels and
tests/expert_cases.py use; the two must agree.  The set keeps: one case of 1024 agents, one that never grows and one
that grows >= 10 times, a team size that is not a multiple of 64 and one that is not a multiple of 4, a file < 1 MB.
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import gen_expert_golden as base  # noqa: E402  (puts ROOT and tests/ on sys.path)
import expert_cases as ec  # noqa: E402
from oracle import rollout_oracle as ro  # noqa: E402

# (N, map side, obstacle density, wait probability, box, longest path kept)
SPECS = ((160, 64, 0.10, 0.1, None, 6),
         (130, 200, 0.05, 0.1, None, 4),            # 1: a sparse team: the radius grows >= 10 times (long search)
         (256, 100, 0.10, 0.2, None, 5),
         (200, 40, 0.10, 0.1, (10, 10, 24), 4),     # 3: a dense team that stays together: never grows
         (1024, 128, 0.10, 0.1, None, 3))


def main():
    tr, sim, EasyDict = base.import_reference()
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
        while True:
            grid, starts, goals = ec.random_map(rng, N, side, side, dens, box)
            paths = ec.expert_paths(rng, grid, starts, goals, wait, cap)
            if paths is not None and 3 <= max(len(p) for p in paths) <= 25:
                break
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, 'input'))
            os.makedirs(os.path.join(tmp, 'output_ECBS'))
            fail_yaml = base.reference_failure_yaml(sim, os.path.join(tmp, 'input'), grid, starts, goals, ci)
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
        meta.append({'N': N, 'H': side, 'W': side, 'T': int(state.shape[0]), 'radius': float(radius).hex(),
                     'growth': int(growth), 'path_lengths': [len(p) for p in paths]})
        print('case %d: N %d, %dx%d, %d steps, radius %.4f after %d growths' % (ci, N, side, side, state.shape[0],
                                                                              radius, growth))
    sizes = [m['N'] for m in meta]
    assert 1024 in sizes and any(n % 64 for n in sizes) and any(n % 4 for n in sizes)
    assert any(m['growth'] == 0 for m in meta) and any(m['growth'] >= 10 for m in meta)
    store['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, 'tests', 'golden', 'expert_schedules_team.npz')
    np.savez_compressed(path, **store)
    assert os.path.getsize(path) < 1000000, os.path.getsize(path)
    print('wrote %s (%d bytes); %d graphs checked against the eigenvalue test' % (path, os.path.getsize(path),
                                                                               seen['graphs']))
    print('reference transformer on this CPU (one process, files on tmpfs included): %d agent-samples in %.3f s = '
          '%.0f agent-samples/s' % (nsamples, spent, nsamples / spent))


if __name__ == '__main__':
    main()
