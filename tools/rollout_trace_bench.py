"""What recording a rollout costs: the same steps with and without BatchedRollout(record=...).

    python tools/rollout_trace_bench.py [--reps 20]

(a) 512 episodes of 10 agents on 20 x 20, bursts of 8 one-launch policy steps: gnnpp_rollout_policy_steps against
    gnnpp_rollout_policy_steps_traced (a record launch behind each step);
(b) one episode of 1024 agents on 64 x 64, the team kernels' simulator step (move -> graph -> observations) with and
    without the record launch behind it.
HIP events after warm-up, mean over --reps calls (the timer of tools/rollout_team_bench.py); us per STEP.  One JSON line each.
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

from rollout_team_bench import timed                                   # noqa: E402

BIG = 1 << 30                                                           # no episode ends while timing
WARMUP = 3


def policy_bursts(reps, dev, burst=8):
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from gnn_pathplanning_amd.rollout import BatchedRollout
    from oracle import policy_oracle as orc
    from rollout_team_cases import make_instances
    B, N, W = 512, 10, 20
    grids, starts, goals = make_instances(np.random.default_rng(512), B, N, W, W, 0.1)

    class Cfg:
        num_agents, nGraphFilterTaps, device = N, 3, dev
    net = DecentralPlannerNet(Cfg()).to(dev).eval()
    net.load_state_dict(orc.init_state_dict(3, seed=1))
    out = {'B': B, 'N': N, 'map': W, 'burst': burst}
    for name, record in (('plain', False), ('traced', (WARMUP + reps) * burst + 1)):
        env = BatchedRollout(grids, starts, goals, BIG, dev, tie_mode='lowest', record=record)
        with torch.no_grad():
            env.step(net)                                               # (step 0 may grow the radius)
            assert env._logits is not None                              # the one-launch step
            out[name + '_us_per_step'] = timed(lambda: env.steps(net, burst), reps, WARMUP) / burst
    out['record_us_per_step'] = out['traced_us_per_step'] - out['plain_us_per_step']
    return out


def team_steps(reps, dev):
    from gnn_pathplanning_amd.rollout import BatchedRollout
    from rollout_team_cases import make_instances
    B, N, W = 1, 1024, 64
    rng = np.random.default_rng(1024)
    grids, starts, goals = make_instances(rng, B, N, W, W, 0.05)
    acts = [torch.from_numpy(rng.integers(0, 5, size=(B, N))).to(dev) for _ in range(4)]
    out = {'B': B, 'N': N, 'map': W}
    for name, record in (('plain', False), ('traced', WARMUP + reps + 1)):
        env = BatchedRollout(grids, starts, goals, BIG, dev, tie_mode='lowest', record=record)
        env.observe()
        env.gso(0)
        k = [0]

        def step():
            k[0] += 1
            env.move_and_observe(actions=acts[k[0] & 3])
        out[name + '_us_per_step'] = timed(step, reps, WARMUP)
    out['record_us_per_step'] = out['traced_us_per_step'] - out['plain_us_per_step']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for fn in (policy_bursts, team_steps):
        print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in fn(args.reps, dev).items()}),
              flush=True)


if __name__ == '__main__':
    main()
