"""Time the large-team simulator launches (teams of more than 128 agents) and a whole closed-loop step.

    python tools/rollout_team_bench.py [--reps 20] [--configs 64x200x64,16x512x100,8x1024x128]

Per (B, N, map side): each simulator call (observe, gso, move, gso_observe, step) and the policy forward
(DecentralPlannerNet K = 3, eval) timed with HIP events after warm-up, mean over --reps calls; then a whole
closed-loop step (BatchedRollout.step: policy + simulator); then the CPU oracle's time for ONE episode-step
(observations + GSO + move of one episode) as the point of comparison.  One JSON line per configuration.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


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
    return t0.elapsed_time(t1) * 1e3 / reps                            # us per call


def bench(B, N, W, reps, dev):
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from gnn_pathplanning_amd.rollout import BatchedRollout
    from oracle import policy_oracle as orc
    from oracle import rollout_oracle as ro
    from rollout_team_cases import make_instances
    rng = np.random.default_rng(B * N)
    grids, starts, goals = make_instances(rng, B, N, W, W, 0.05)
    big = 1 << 30                                                       # no episode ends while timing
    env = BatchedRollout(grids, starts, goals, big, dev, tie_mode='lowest')
    env.observe()
    env.gso(0)
    acts = [torch.from_numpy(rng.integers(0, 5, size=(B, N))).to(dev) for _ in range(4)]
    k = [0]

    def move():
        k[0] += 1
        env.move(actions=acts[k[0] & 3])

    def step():
        k[0] += 1
        env.move_and_observe(actions=acts[k[0] & 3])

    class Cfg:
        num_agents, nGraphFilterTaps, device = N, 3, dev
    net = DecentralPlannerNet(Cfg()).to(dev).eval()
    net.load_state_dict(orc.init_state_dict(3, seed=1))

    def policy():
        with torch.no_grad():
            net.addGSO(env.S)
            net.forward_logits(env.obs)
    out = {'B': B, 'N': N, 'map': W}
    out['observe_us'] = timed(env.observe, reps)
    out['gso_us'] = timed(lambda: env.gso(1), reps)
    out['move_us'] = timed(move, reps)
    out['gso_observe_us'] = timed(env.gso_observe, reps)
    out['sim_step_us'] = timed(step, reps)                              # move -> gso -> observe
    out['policy_fwd_us'] = timed(policy, reps)
    loop = BatchedRollout(grids, starts, goals, big, dev, tie_mode='lowest')

    def closed():
        with torch.no_grad():
            loop.step(net)
    out['closed_loop_step_us'] = timed(closed, reps)
    out['sim_lt_policy'] = out['move_us'] + out['gso_observe_us'] < out['policy_fwd_us']
    # the CPU oracle: one episode-step
    ep = ro.EpisodeState(grids[0], goals[0], starts[0], big)
    a = rng.integers(0, 5, size=N)
    t = time.perf_counter()
    ro.build_observations(grids[0], goals[0], ep.cur)
    ro.communication_gso(ep.cur, 6.0, False)
    ro.move_step(ep, a, 1, lambda c: c[0])
    out['oracle_cpu_episode_step_us'] = (time.perf_counter() - t) * 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--configs', default='64x200x64,16x512x100,8x1024x128')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for c in args.configs.split(','):
        B, N, W = (int(v) for v in c.split('x'))
        print(json.dumps({k: (round(v, 1) if isinstance(v, float) else v)
                          for k, v in bench(B, N, W, args.reps, dev).items()}), flush=True)


if __name__ == '__main__':
    main()
