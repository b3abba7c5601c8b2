"""Time one gnnpp_schedule_samples call: agent-samples per second and achieved write bandwidth.

    python tools/expert_bench.py [--agents 10] [--side 20] [--steps 1000,32000,256000] [--reps 10] [--out FILE]

Synthetic solved cases (tests/expert_cases.py: ~25 steps each, 64 distinct ones tiled up to the requested number of
steps) are transformed in ONE call, outputs preallocated, timed with HIP events after warm-up, mean over --reps calls.
The rate is set against the bytes the call MUST write, T_total * N * (3 * 121 * 4 + 4 * N + 5 * 4) (observations, fp32
GSO, targets), over the HBM peak bench.py's roofline uses.  One JSON record per size; --out collects them in a file.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HBM_PEAK_TBPS = 8.0                     # bench.py::HBM_PEAK_TBPS


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / reps                           # seconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=10)
    ap.add_argument('--side', type=int, default=20)
    ap.add_argument('--steps', default='1000,32000,256000')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X: a CPU run measures nothing'
    import expert_cases as ec
    from gnn_pathplanning_amd import expert
    dev, N = torch.device('cuda:0'), a.agents
    rng = np.random.default_rng(7)
    made = [ec.random_case(rng, N, a.side, a.side, density=0.1, wait=0.1, max_steps=25) for _ in range(64)]
    sched = [ec.schedule_of(paths, goal) for _, goal, paths in made]
    records = []
    for want in (int(s) for s in a.steps.split(',')):
        grids, goals, parts, T = [], [], [], 0
        while T < want:
            c = len(parts) % len(made)
            part = sched[c][:want - T]
            # (a schedule cut short is a schedule whose goal is the state that followed)
            goals.append(made[c][1] if len(part) == len(sched[c]) else sched[c][len(part)])
            grids.append(made[c][0])
            parts.append(part)
            T += len(part)
        C = len(parts)
        bounds = np.cumsum([0] + [len(p) for p in parts]).tolist()
        grid = torch.from_numpy(np.stack(grids)).to(dev)
        goal = torch.from_numpy(np.stack(goals).astype(np.int32)).to(dev)
        pos = torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(dev)
        start = torch.tensor(bounds, dtype=torch.int32, device=dev)
        out = expert.ScheduleSamples(
            input=torch.empty(T, N, 3, 11, 11, device=dev), GSO=torch.empty(T, N, N, device=dev), GSO64=None,
            target=torch.empty(T, N, 5, device=dev), radius=torch.empty(C, dtype=torch.float64, device=dev),
            growth=torch.empty(C, dtype=torch.int32, device=dev), status=torch.empty(C, dtype=torch.int32, device=dev),
            step_growth=torch.empty(T, dtype=torch.int32, device=dev), bounds=bounds)
        sec = timed(lambda: expert.enqueue_schedule_samples(grid, goal, pos, start, out), a.reps)
        assert int(out.status.abs().sum().item()) == 0
        nbytes = T * N * (3 * 121 * 4 + 4 * N + 5 * 4)
        rec = {'what': 'gnnpp_schedule_samples, one call (3 launches), HIP events, mean of %d calls after 3' % a.reps,
               'agents': N, 'map': '%dx%d' % (a.side, a.side), 'cases': C, 'steps': T, 'ms_per_call': round(sec * 1e3, 4),
               'agent_samples_per_s': round(T * N / sec), 'steps_per_s': round(T / sec),
               'bytes_written_min': nbytes, 'write_GBps': round(nbytes / sec / 1e9, 1),
               'frac_of_hbm_peak_%gTBps' % HBM_PEAK_TBPS: round(nbytes / sec / (HBM_PEAK_TBPS * 1e12), 4)}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del out, grid, goal, pos
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'records': records}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
