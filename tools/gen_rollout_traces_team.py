"""Record rollout traces of teams larger than 128 agents from the REAL reference simulator
(utils/multirobotsim_dcenlocal.py) into tests/golden/rollout_traces_team.npz.

Build-container only: it needs the reference tree that oracle/gen_golden_rollout.py imports.  Only data is stored.

    python tools/gen_rollout_traces_team.py

Scripted noisy-greedy policy (oracle/gen_golden_rollout.py::run_case) on crowded maps, so that every trace holds
tens of vertex conflicts, swaps and all-stop branches; every random.choice outcome is recorded for replay.
"""
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden_rollout import Cfg, OUT, import_reference, make_case, pack_case, run_case  # noqa: E402

SPECS = (  # (N, W, obstacle density, makespan, noise); maxstep = 2 * makespan
    (160, 64, 0.05, 5, 0.35),
    (256, 64, 0.04, 5, 0.35),
    (160, 100, 0.03, 5, 0.30),
    (256, 100, 0.03, 4, 0.30),
)


def main():
    simmod, _ = import_reference()
    rng = np.random.default_rng(20261016)
    random.seed(9090)
    store, meta = {}, []
    for ci, (N, W, dens, mk, noise) in enumerate(SPECS):
        cfg = Cfg(N)
        grid, starts, goals = make_case(rng, N, W, dens)
        rec, fin = run_case(simmod, None, cfg, grid, starts, goals, mk, 'greedy', rng, noise)
        # the GSO is stored as float32 (what the kernels are compared against: S.float() of the simulator's float64)
        rec['gso'] = [g.astype(np.float32) for g in rec['gso']]
        pack_case(store, meta, ci, cfg, grid, goals, rec, fin, 'greedy')
    store['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(OUT, 'rollout_traces_team.npz')
    np.savez_compressed(path, **store)
    print('wrote', path, os.path.getsize(path))


if __name__ == '__main__':
    main()
