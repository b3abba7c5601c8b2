"""Policy forward of large teams under largeGraphFilter = 'dense' and 'lists', in one process on one GPU.

    python tools/filter_team_bench.py [--out profiles/filter_team.json] [--only NAME] [--reps 20]

The three configurations of DESIGN.md section 5.5 (64 x 200 agents on a 64 x 64 map, 16 x 512 on 100 x 100, 8 x 1024 on
128 x 128; K = 3), the graphs from BatchedRollout.gso.  Per configuration and route: warm-up, then the mean of `reps`
forward_logits calls timed one by one with HIP events; also the gso launch itself (the other half of a closed-loop step)
and the largest difference of the two routes' logits.  Writes one JSON file.  --only NAME runs one configuration a few
times without timing it (the run to put under `rocprofv3 --kernel-trace --stats`)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = (('64x200', 64, 200, 64), ('16x512', 16, 512, 100), ('8x1024', 8, 1024, 128))


def instances(rng, B, N, W, density=0.05):
    grids = (rng.random((B, W, W)) < density).astype(np.uint8)
    starts = np.zeros((B, N, 2), np.int32)
    goals = np.zeros((B, N, 2), np.int32)
    for b in range(B):
        free = np.argwhere(grids[b] == 0)
        starts[b] = free[rng.choice(len(free), N, replace=False)]
        goals[b] = free[rng.choice(len(free), N, replace=False)]
    return grids, starts, goals


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.mean(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'filter_team.json'))
    ap.add_argument('--only', default=None)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from gnn_pathplanning_amd.rollout import BatchedRollout
    dev = torch.device('cuda:0')
    results = []
    for name, B, N, W in CONFIGS:
        if args.only and args.only != name:
            continue
        grids, starts, goals = instances(np.random.default_rng(N), B, N, W)
        env = BatchedRollout(grids, starts, goals, 8, dev)
        obs, S = env.observe(), env.gso()
        nets = {}
        for route in ('dense', 'lists'):
            class Cfg:
                num_agents, nGraphFilterTaps, device, largeGraphFilter = N, 3, dev, route
            torch.manual_seed(1)
            nets[route] = DecentralPlannerNet(Cfg()).to(dev).eval()
            nets[route].addGSO(S)
        nets['lists'].load_state_dict(nets['dense'].state_dict())
        if args.only:
            for _ in range(5):
                for route in ('dense', 'lists'):
                    nets[route].forward_logits(obs)
            torch.cuda.synchronize()
            continue
        row = dict(config=name, B=B, N=N, map=W, K=3, mean_degree=float((S != 0).sum(1).float().mean().item()))
        for route in ('dense', 'lists'):
            mean, best = timed(lambda: nets[route].forward_logits(obs), args.reps)
            row[route + '_us'], row[route + '_min_us'] = round(mean, 1), round(best, 1)
        row['gso_us'] = round(timed(env.gso, args.reps)[0], 1)
        row['speedup'] = round(row['dense_us'] / row['lists_us'], 3)
        row['max_abs_logit_diff'] = float((nets['dense'].forward_logits(obs) - nets['lists'].forward_logits(obs))
                                          .abs().max().item())
        print(json.dumps(row))
        results.append(row)
    if not args.only:
        with open(args.out, 'w') as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=args.reps, results=results), f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
