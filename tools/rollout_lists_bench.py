"""Time the hand-over of the communication graph from the simulator to the team filter, dense against lists.

    python tools/rollout_lists_bench.py [--reps 20] [--configs 64x200x64,16x512x100,8x1024x128] [--out profiles/rollout_lists.json]

The method of tools/rollout_team_bench.py: HIP events, the mean of --reps calls after warm-up, one process.  Per
(B, N, map side):
  gso_us                    gnnpp_rollout_gso                     (the dense S: N^2 floats per episode)
  lists_from_dense_us       gnnpp_team_lists_from_dense           (team_lists_kernel alone)
  rollout_lists_us          gnnpp_rollout_lists                   (the lists straight from the positions)
  fwd_dense_us              the 'lists' forward on the dense S    (list building inside the call)
  fwd_lists_us              forward_logits_lists on the block     (no list building)
  loop_dense_us             BatchedRollout(graph='dense').step with largeGraphFilter='lists'
  loop_lists_us             BatchedRollout(graph='lists').step with the same planner
and `lists_le_gso_plus_build`: rollout_lists_us <= gso_us + lists_from_dense_us (the expectation of DESIGN.md 5.5).
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

from rollout_team_bench import timed  # noqa: E402


def bench(B, N, W, reps, dev):
    from gnn_pathplanning_amd import graphML as gml
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from gnn_pathplanning_amd.rollout import BatchedRollout
    from oracle import policy_oracle as orc
    from rollout_team_cases import make_instances
    rng = np.random.default_rng(B * N)
    grids, starts, goals = make_instances(rng, B, N, W, W, 0.05)
    big = 1 << 30                                                       # no episode ends while timing
    dense = BatchedRollout(grids, starts, goals, big, dev, graph='dense')
    lists = BatchedRollout(grids, starts, goals, big, dev, graph='lists')
    for env in (dense, lists):
        env.observe()
        env.gso(0)
    block = gml.team_lists_from_dense(dense.S)

    class Cfg:
        num_agents, nGraphFilterTaps, device, largeGraphFilter = N, 3, dev, 'lists'
    net = DecentralPlannerNet(Cfg()).to(dev).eval()
    net.load_state_dict(orc.init_state_dict(3, seed=1))

    def fwd_dense():
        with torch.no_grad():
            net.addGSO(dense.S)
            net.forward_logits(dense.obs)

    def fwd_lists():
        with torch.no_grad():
            net.forward_logits_lists(lists.obs, lists.lists)
    out = {'B': B, 'N': N, 'map': W, 'reps': reps}
    out['gso_us'] = timed(lambda: dense.gso(1), reps)
    out['lists_from_dense_us'] = timed(lambda: gml.team_lists_from_dense(dense.S, out=block), reps)
    out['rollout_lists_us'] = timed(lambda: lists.gso(1), reps)
    out['fwd_dense_us'] = timed(fwd_dense, reps)
    out['fwd_lists_us'] = timed(fwd_lists, reps)
    out['mean_degree'] = float(gml.team_lists_views(lists.lists, B, N)[0].float().mean().item())
    loops = {g: BatchedRollout(grids, starts, goals, big, dev, graph=g) for g in ('dense', 'lists')}
    for g, loop in loops.items():
        def closed(loop=loop):
            with torch.no_grad():
                loop.step(net)
        out['loop_%s_us' % g] = timed(closed, reps)
    out['lists_le_gso_plus_build'] = out['rollout_lists_us'] <= out['gso_us'] + out['lists_from_dense_us']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--configs', default='64x200x64,16x512x100,8x1024x128')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    rows = []
    for c in args.configs.split(','):
        B, N, W = (int(v) for v in c.split('x'))
        rows.append({k: (round(v, 1) if isinstance(v, float) else v) for k, v in bench(B, N, W, args.reps, dev).items()})
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/rollout_lists_bench.py', 'device': torch.cuda.get_device_name(0), 'rows': rows}, f,
                      indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
