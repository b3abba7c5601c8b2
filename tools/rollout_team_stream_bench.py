"""Streamed against chunked evaluation of LARGE teams: casegen cases of N agents on W x W, the step limit
3 x the goal-distance bound (mapf.maxstep_from_distances), a randomly initialised DecentralPlannerNet
(largeGraphFilter='lists', K = 3, eval) in the loop, on the dense graph and on the neighbour lists.

    stream    rollout.TeamRolloutStream(slots=B, graph=..., reseat_every=1 | 4).run
    chunked   BatchedRollout(graph=...).run over chunks of B cases -- the evaluation as it was before the stream existed

Per shape: cases/s, the policy steps taken, the occupancy (live slot-steps / all slot-steps) and the seconds of every
variant, medians of `runs` warm runs interleaved in one process; the time of one reseat that seats every slot, and of the
graph + observation launches the step after a reseat runs over all slots (the redundant graph build of 5.14), from device
events.  Results go to profiles/rollout_team_stream.json.

    python tools/rollout_team_stream_bench.py [--shapes 256:64:48:16,1024:128:12:4] [--rate 3] [--runs 5]

A shape is agents:map side:cases:slots."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _event_ms(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def shape(N, W, C, B, rate, runs, dev):
    from gnn_pathplanning_amd import casegen, mapf
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from gnn_pathplanning_amd.rollout import BatchedRollout, TeamRolloutStream
    from oracle import policy_oracle as orc
    cases = casegen.generate(C, N, W, W, dev, density=0.1, seed=2024)
    assert bool(cases.ok.all())
    maxstep = mapf.maxstep_from_distances(mapf.distances(cases.grid, cases.start, cases.goal, dev).lower_makespan, rate)

    class Cfg:
        num_agents, nGraphFilterTaps, device, largeGraphFilter = N, 3, dev, 'lists'
    net = DecentralPlannerNet(Cfg()).to(dev).eval()
    net.load_state_dict(orc.init_state_dict(3, seed=1))

    def stream(graph, every):
        def run():
            res = TeamRolloutStream(cases.grid, cases.start, cases.goal, maxstep, dev, slots=B, reseat_every=every,
                                    graph=graph).run(net)
            return res['steps'], res['occupancy'], int(res['success'].sum()), res['lived']
        return run

    def chunked(graph):
        def run():
            steps, slot_steps, lived, ok = 0, 0, [], 0
            for lo in range(0, C, B):
                env = BatchedRollout(cases.grid[lo:lo + B], cases.start[lo:lo + B].clone(), cases.goal[lo:lo + B],
                                     maxstep[lo:lo + B], dev, graph=graph)
                res = env.run(net)
                steps += res['steps']
                slot_steps += res['steps'] * env.B
                lived.append(torch.minimum(res['end_step'].max(dim=1).values + 1, maxstep[lo:lo + B].cpu()))
                ok += int(res['success'].sum())
            lived = torch.cat(lived)
            return steps, float(lived.sum()) / slot_steps, ok, lived
        return run

    variants = [('stream_%s_every%d' % (g, e), stream(g, e)) for g in ('dense', 'lists') for e in (1, 4)] + \
               [('chunked_%s' % g, chunked(g)) for g in ('dense', 'lists')]
    times = {name: [] for name, _ in variants}
    last = {}
    with torch.no_grad():
        for run in range(runs + 1):                          # (round 0 warms everything up)
            for name, fn in variants:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                last[name] = fn()
                torch.cuda.synchronize(dev)
                if run:
                    times[name].append(time.perf_counter() - t0)
    lived = last['chunked_dense'][3].to(torch.int64)
    for name, _ in variants:                                 # the same episodes everywhere
        assert torch.equal(last[name][3].to(torch.int64), lived), name
    out = {'agents': N, 'map': W, 'cases': C, 'slots': B, 'rate': rate, 'runs': runs,
           'maxstep_min_median_max': [int(maxstep.min()), int(maxstep.median()), int(maxstep.max())]}
    for name, _ in variants:
        sec = statistics.median(times[name])
        out[name] = {'seconds_median': sec, 'seconds_min': min(times[name]), 'seconds_max': max(times[name]),
                     'cases_per_s': C / sec, 'policy_steps': last[name][0], 'occupancy': last[name][1],
                     'successes': last[name][2]}
    out['stream_over_chunked_cases_per_s'] = {
        '%s_every%d' % (g, e): out['stream_%s_every%d' % (g, e)]['cases_per_s'] / out['chunked_%s' % g]['cases_per_s']
        for g in ('dense', 'lists') for e in (1, 4)}
    # one reseat that seats every slot (a fresh stream's first), and the graph + observation launches over all slots that
    # the step after a reseat runs: medians of 9, device events
    for g in ('dense', 'lists'):
        reseat, rebuild = [], []
        for _ in range(10):
            st = TeamRolloutStream(cases.grid, cases.start, cases.goal, maxstep, dev, slots=B, graph=g)
            reseat.append(_event_ms(st.reseat, dev))
            rebuild.append(_event_ms(st.env.gso_observe, dev))
        out['reseat_all_slots_ms_%s' % g] = statistics.median(reseat[1:])
        out['graph_and_observations_all_slots_ms_%s' % g] = statistics.median(rebuild[1:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='256:64:48:16,1024:128:12:4')
    ap.add_argument('--rate', type=float, default=3.0)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rollout_team_stream.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'shapes': []}
    for spec in a.shapes.split(','):
        N, W, C, B = (int(v) for v in spec.split(':'))
        out['shapes'].append(shape(N, W, C, B, a.rate, a.runs, dev))
        print(json.dumps(out['shapes'][-1]), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:                          # (written after every shape: a long run keeps what it has)
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
