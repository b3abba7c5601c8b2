"""Training step of large teams under largeGraphTraining = 'dense' and 'lists', in one process on one GPU.

    python tools/filter_team_train_bench.py [--out profiles/filter_team_train.json] [--only NAME] [--reps 20]

The three configurations of DESIGN.md section 5.3a (64 x 200 agents on a 64 x 64 map, 16 x 512 on 100 x 100, 8 x 1024 on
128 x 128; K = 3), the graphs from BatchedRollout.gso, the method of tools/filter_team_bench.py: warm-up, then the mean
of `reps` calls timed one by one with HIP events.  Per configuration and route: training.train_step; the filter's
forward + backward alone (graphML._LSIGFFunction on the dense S against graphML.lsigf_team_train on the lists, G = F =
128, ReLU, a fixed cotangent); the peak allocated bytes of one train_step; and the list-transposition launch.  Writes one
JSON file.  --only NAME runs one configuration's train_step a few times under both routes without timing it (the run to
put under `rocprofv3 --kernel-trace --stats`)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from filter_team_bench import CONFIGS, instances, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'filter_team_train.json'))
    ap.add_argument('--only', default=None)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    from gnn_pathplanning_amd import graphML as gml
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from gnn_pathplanning_amd.rollout import BatchedRollout
    from gnn_pathplanning_amd.training import FusedAdam, train_step
    dev = torch.device('cuda:0')
    results = []
    for name, B, N, W in CONFIGS:
        if args.only and args.only != name:
            continue
        grids, starts, goals = instances(np.random.default_rng(N), B, N, W)
        env = BatchedRollout(grids, starts, goals, 8, dev)
        obs, S = env.observe(), env.gso()
        tgt = torch.nn.functional.one_hot(torch.randint(0, 5, (B, N), device=dev), 5).float()
        nets, opts = {}, {}
        for route in ('dense', 'lists'):
            class Cfg:
                num_agents, nGraphFilterTaps, device, largeGraphTraining = N, 3, dev, route
            torch.manual_seed(1)
            nets[route] = DecentralPlannerNet(Cfg()).to(dev).train()
            opts[route] = FusedAdam(nets[route].parameters(), lr=1e-3, weight_decay=1e-5)
        if args.only:
            for _ in range(5):
                for route in ('dense', 'lists'):
                    train_step(nets[route], opts[route], obs, tgt, S)
            torch.cuda.synchronize()
            continue
        row = dict(config=name, B=B, N=N, map=W, K=3, mean_degree=float((S != 0).sum(1).float().mean().item()))
        for route in ('dense', 'lists'):
            mean, best = timed(lambda: train_step(nets[route], opts[route], obs, tgt, S), args.reps)
            row['step_%s_us' % route], row['step_%s_min_us' % route] = round(mean, 1), round(best, 1)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            train_step(nets[route], opts[route], obs, tgt, S)
            torch.cuda.synchronize()
            row['step_%s_peak_bytes' % route] = int(torch.cuda.max_memory_allocated(dev) - base)
        # the filter layer alone: forward + backward for h, x and b
        gf = nets['dense'].GFL[0]
        x = torch.randn(B, N, 128, device=dev, requires_grad=True)
        dy = torch.randn(B, N, 128, device=dev)
        S4 = S.unsqueeze(1)
        lists = gml.team_lists_from_dense(S4)
        lists_t = gml.team_lists_transpose(lists, B, N)

        def clear():
            gf.weight.grad = gf.bias.grad = x.grad = None

        def dense():
            clear()
            gml._LSIGFFunction.apply(gf.weight, S4, x, gf.bias, True, None, True, True, None).backward(dy)

        def on_lists():
            clear()
            gml.lsigf_team_train(gf.weight, lists, x, gf.bias, relu=True, lists_t=lists_t).backward(dy)
        row['filter_dense_us'] = round(timed(dense, args.reps)[0], 1)
        row['filter_lists_us'] = round(timed(on_lists, args.reps)[0], 1)
        row['transpose_us'] = round(timed(lambda: gml.team_lists_transpose(lists, B, N, out=lists_t), args.reps)[0], 1)
        row['lists_from_dense_us'] = round(timed(lambda: gml.team_lists_from_dense(S4, out=lists), args.reps)[0], 1)
        row['step_speedup'] = round(row['step_dense_us'] / row['step_lists_us'], 3)
        row['filter_speedup'] = round(row['filter_dense_us'] / row['filter_lists_us'], 3)
        print(json.dumps(row))
        results.append(row)
    if not args.only:
        with open(args.out, 'w') as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=args.reps, results=results), f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
