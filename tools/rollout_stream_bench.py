"""Streamed against chunked evaluation: C casegen cases of N agents on W x W, the step limit from the
goal distances (mapf.maxstep_from_distances), a randomly initialised DecentralPlannerNet (K = 3, eval) in the loop.

    stream    rollout.RolloutStream(slots=B).run
    chunked   BatchedRollout.run over chunks of B cases -- the evaluation as it was before the stream existed

Reports cases/s, the policy steps taken and the occupancy (live slot-steps / all slot-steps) of both, medians of several
warm runs interleaved in one process, into profiles/rollout_stream.json.

    python tools/rollout_stream_bench.py [--cases 4096] [--slots 512] [--agents 10] [--map 20] [--rate 3] [--runs 5]

--trace measures what a per-case trace costs instead: the stream untraced (the path above) and with
trace=True at reseat_every 1 and 4, and the chunked evaluation unrecorded and with record=True, all interleaved in one
process; medians and spreads go to profiles/rollout_stream_trace.json (the file above is not touched).

    python tools/rollout_stream_bench.py --trace [--runs 7]"""
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
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', action='store_true')
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'rollout_stream_trace.json' if a.trace else 'rollout_stream.json')
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

    if a.trace:
        return trace_cost(a, cases, maxstep, net, dev)

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


def trace_cost(a, cases, maxstep, net, dev):
    """--trace: six variants per round, `runs` warm rounds behind one warm-up round.  Every variant gets the same cases (a
    chunk's rollout moves its agents in the tensor it is given, so it gets a copy of the starts)."""
    from gnn_pathplanning_amd.rollout import BatchedRollout, RolloutStream
    C, B = a.cases, a.slots

    def stream(every, traced):
        def run():
            st = RolloutStream(cases.grid, cases.start, cases.goal, maxstep, dev, slots=B, reseat_every=every, trace=traced)
            res = st.run(net)
            return res['steps'], res['lived'], st.trace.steps.cpu() if traced else None
        return run

    def chunked(recorded):
        def run():
            steps, lived, rows = 0, [], []
            for lo in range(0, C, B):
                env = BatchedRollout(cases.grid[lo:lo + B], cases.start[lo:lo + B].clone(), cases.goal[lo:lo + B],
                                     maxstep[lo:lo + B], dev, record=recorded)
                res = env.run(net)
                steps += res['steps']
                lived.append(torch.minimum(res['end_step'].max(dim=1).values + 1, maxstep[lo:lo + B].cpu()))
                if recorded:
                    rows.append(env.trace.steps.cpu())
            return steps, torch.cat(lived), torch.cat(rows) if recorded else None
        return run

    variants = [('stream_every1', stream(1, False)), ('stream_every1_traced', stream(1, True)),
                ('stream_every4', stream(4, False)), ('stream_every4_traced', stream(4, True)),
                ('chunked', chunked(False)), ('chunked_recorded', chunked(True))]
    times = {name: [] for name, _ in variants}
    last = {}
    with torch.no_grad():
        for run in range(a.runs + 1):                        # (round 0 warms everything up)
            for name, fn in variants:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                last[name] = fn()
                torch.cuda.synchronize(dev)
                if run:
                    times[name].append(time.perf_counter() - t0)
    lived = last['chunked'][1].to(torch.int64)
    for name, _ in variants:                                 # the same episodes everywhere, and every trace holds them
        assert torch.equal(last[name][1].to(torch.int64), lived), name
        assert last[name][2] is None or torch.equal(last[name][2].to(torch.int64), lived), name
    out = {'cases': C, 'slots': B, 'agents': a.agents, 'map': a.map, 'rate': a.rate, 'runs': a.runs,
           'maxstep_min_median_max': [int(maxstep.min()), int(maxstep.median()), int(maxstep.max())]}
    for name, _ in variants:
        sec = statistics.median(times[name])
        out[name] = {'seconds_median': sec, 'seconds_min': min(times[name]), 'seconds_max': max(times[name]),
                     'cases_per_s': C / sec, 'policy_steps': last[name][0]}
    med = lambda name: out[name]['seconds_median']                                     # noqa: E731
    out['ratios_of_median_seconds'] = {
        'traced_over_untraced_every1': med('stream_every1_traced') / med('stream_every1'),
        'traced_over_untraced_every4': med('stream_every4_traced') / med('stream_every4'),
        'recorded_over_unrecorded_chunked': med('chunked_recorded') / med('chunked'),
        'chunked_over_stream_every1': med('chunked') / med('stream_every1'),
        'chunked_over_stream_every4': med('chunked') / med('stream_every4'),
        'chunked_recorded_over_stream_every1_traced': med('chunked_recorded') / med('stream_every1_traced'),
        'chunked_recorded_over_stream_every4_traced': med('chunked_recorded') / med('stream_every4_traced')}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
