"""Streamed against chunked evaluation: C casegen cases of N agents on W x W, the step limit from the
goal distances (mapf.maxstep_from_distances), a randomly initialised DecentralPlannerNet (K = 3, eval) in the loop.

    stream    rollout.RolloutStream(slots=B).run
    chunked   BatchedRollout.run over chunks of B cases -- the evaluation as it was before the stream existed

Reports cases/s, the policy steps taken and the occupancy (live slot-steps / all slot-steps) of both, medians of several
warm runs interleaved in one process, into profiles/rollout_stream.json.

    python tools/rollout_stream_bench.py [--cases 4096] [--slots 512] [--agents 10] [--map 20] [--rate 3] [--runs 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', type=int, default=4096)
    ap.add_argument('--slots', type=int, default=512)
    ap.add_argument('--agents', type=int, default=10)
    ap.add_argument('--map', type=int, default=20)
    ap.add_argument('--rate', type=float, default=3.0)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--reseat-every', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rollout_stream.json'))
    a = ap.parse_args()
    from gnn_pathplanning_amd import casegen, mapf
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from gnn_pathplanning_amd.rollout import BatchedRollout, RolloutStream
    from oracle import policy_oracle as orc
    dev = torch.device('cuda:0')
    C, B, N, W = a.cases, a.slots, a.agents, a.map
    cases = casegen.generate(C, N, W, W, dev, density=0.1, seed=2024)
    assert bool(cases.ok.all())
    maxstep = mapf.maxstep_from_distances(mapf.distances(cases.grid, cases.start, cases.goal, dev).lower_makespan, a.rate)

    class Cfg:
        num_agents, nGraphFilterTaps, device = N, 3, dev
    net = DecentralPlannerNet(Cfg()).to(dev).eval()
    net.load_state_dict(orc.init_state_dict(3, seed=1))

    def stream():
        res = RolloutStream(cases.grid, cases.start, cases.goal, maxstep, dev, slots=B, reseat_every=a.reseat_every).run(net)
        return res['steps'], res['occupancy'], int(res['success'].sum()), res['lived']

    def chunked():
        steps, slot_steps, lived, ok = 0, 0, [], 0
        for lo in range(0, C, B):
            env = BatchedRollout(cases.grid[lo:lo + B], cases.start[lo:lo + B], cases.goal[lo:lo + B], maxstep[lo:lo + B], dev)
            res = env.run(net)
            steps += res['steps']
            slot_steps += res['steps'] * env.B
            lived.append(torch.minimum(res['end_step'].max(dim=1).values + 1, maxstep[lo:lo + B].cpu()))
            ok += int(res['success'].sum())
        lived = torch.cat(lived)
        return steps, float(lived.sum()) / slot_steps, ok, lived

    times = {'stream': [], 'chunked': []}
    last = {}
    with torch.no_grad():
        for run in range(a.runs + 1):                        # (run 0 warms both up)
            for name, fn in (('stream', stream), ('chunked', chunked)):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                last[name] = fn()
                torch.cuda.synchronize(dev)
                if run:
                    times[name].append(time.perf_counter() - t0)
    assert torch.equal(last['stream'][3].to(torch.int64), last['chunked'][3].to(torch.int64))     # the same episodes
    out = {'cases': C, 'slots': B, 'agents': N, 'map': W, 'rate': a.rate, 'runs': a.runs, 'reseat_every': a.reseat_every,
           'maxstep_min_median_max': [int(maxstep.min()), int(maxstep.median()), int(maxstep.max())]}
    for name in ('stream', 'chunked'):
        sec = statistics.median(times[name])
        out[name] = {'seconds_median': sec, 'seconds_min': min(times[name]), 'cases_per_s': C / sec,
                     'policy_steps': last[name][0], 'occupancy': last[name][1], 'successes': last[name][2]}
    out['stream_over_chunked_cases_per_s'] = out['stream']['cases_per_s'] / out['chunked']['cases_per_s']
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
