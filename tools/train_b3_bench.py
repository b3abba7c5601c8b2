"""What trainPrecision='bf16x3' buys: the graphed training step and the convolution launches, exact fp32 against bf16x3.

    python tools/train_b3_bench.py steps  --out profiles/train_b3_steps.json
        the GraphedTrainStep of config 4 (B = 64, N = 10) and of 512 x 10, both precisions in ONE process, alternating,
        --rounds rounds of --steps replays each (device synchronise around every round); per shape and precision the median
        over the rounds and the rounds' spread (max - min), in microseconds per step
    rocprofv3 --kernel-trace --stats -d DIR -o b3 --output-format csv -- python tools/train_b3_bench.py trace
        the run to put under the profiler: eager steps of both precisions, alternating, at 64 x 10 (no timing of its own)
    python tools/train_b3_bench.py kernels DIR --out profiles/train_b3_kernels.json
        reads the kernel trace of that run: per (geometry, grid) the median duration of a conv_mfma_kernel<...> launch
        against a conv_b3_kernel<...> launch, and the spread of the fp32 launches' per-round medians

A geometry (or a step) counts as faster only if its median beats the fp32 path's by more than twice that path's spread
(DESIGN.md 9)."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PRECISIONS = ('fp32', 'bf16x3')
TRACE_ROUNDS, TRACE_STEPS = 6, 10


def _planner(dev, B, N, precision):
    import torch
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from gnn_pathplanning_amd.training import FusedAdam
    from oracle import policy_oracle as orc                   # synthetic inputs only

    class Cfg:
        num_agents, nGraphFilterTaps, device, trainPrecision = N, 3, dev, precision
    torch.manual_seed(1337)
    net = DecentralPlannerNet(Cfg()).to(dev).train()
    opt = FusedAdam(net.parameters(), lr=1e-3, weight_decay=1e-5)
    obs = orc.synth_obs(B, N, seed=1337).to(dev)
    S = torch.from_numpy(orc.synth_gso_geometric(B, N, 20, seed=1337)).float().to(dev)
    g = torch.Generator().manual_seed(0)
    tgt = torch.nn.functional.one_hot(torch.randint(0, 5, (B, N), generator=g), 5).float().to(dev)
    return net, opt, obs, tgt, S


def steps(args):
    import torch
    from gnn_pathplanning_amd.training import GraphedTrainStep
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    out = {'what': 'graphed training step, us per step: median over rounds and the rounds\' spread (max - min)',
           'rounds': args.rounds, 'steps_per_round': args.steps, 'shapes': {}}
    for B, N in ((64, 10), (512, 10)):
        graphed = {}
        for prec in PRECISIONS:
            net, opt, obs, tgt, S = _planner(dev, B, N, prec)
            graphed[prec] = (GraphedTrainStep(net, opt, obs, tgt, S), obs, tgt, S)
        times = {p: [] for p in PRECISIONS}
        for r in range(args.rounds + 1):                      # (round 0 is the warm-up of both)
            for prec in PRECISIONS:
                step, obs, tgt, S = graphed[prec]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    loss = step(obs, tgt, S)
                torch.cuda.synchronize()
                if r:
                    times[prec].append((time.perf_counter() - t0) / args.steps * 1e6)
                assert torch.isfinite(loss).item()
        rec = {p: {'median_us': statistics.median(t), 'spread_us': max(t) - min(t), 'rounds_us': t}
               for p, t in times.items()}
        gain = rec['fp32']['median_us'] - rec['bf16x3']['median_us']
        rec['gain_us'] = gain
        rec['faster'] = bool(gain > 2 * rec['fp32']['spread_us'])
        out['shapes']['%dx%d' % (B, N)] = rec
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


def trace(args):
    import torch
    from gnn_pathplanning_amd.training import train_step
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    runs = {p: _planner(dev, 64, 10, p) for p in PRECISIONS}
    for _ in range(TRACE_ROUNDS + 1):
        for prec in PRECISIONS:
            net, opt, obs, tgt, S = runs[prec]
            for _ in range(TRACE_STEPS):
                train_step(net, opt, obs, tgt, S)
            torch.cuda.synchronize()


def kernels(args):
    """Per-launch durations from the kernel trace.  A launch is keyed by (template arguments, grid): the five layers' forward
    and the four input-gradient launches fall on seven keys (layer 1's forward and layer 2's input gradient share <5, 5> on one
    grid, so do layer 3's two launches and layer 4's input gradient on <1, 1>); the fp32 and the bf16x3 kernel of a key run
    the same GEMM.  The launches of a key arrive in TRACE_ROUNDS + 1 rounds; the first is warm-up."""
    import re
    files = glob.glob(os.path.join(args.dir, '**', '*kernel_trace.csv'), recursive=True)
    assert files, 'no kernel trace under %s' % args.dir
    durs = {}
    for fn in files:
        with open(fn) as f:
            for row in csv.DictReader(f):
                m = re.search(r'(conv_mfma_kernel|conv_b3_kernel)<(\d+), ?(\d+)>', row['Kernel_Name'])
                if not m:
                    continue
                key = '<%s, %s> grid %s x %s' % (m.group(2), m.group(3), row['Grid_Size_X'], row['Grid_Size_Y'])
                start, end = int(row['Start_Timestamp']), int(row['End_Timestamp'])
                durs.setdefault(key, {}).setdefault(m.group(1), []).append((start, (end - start) / 1e3))
    out = {'what': 'conv launches of the eager 64 x 10 step (rocprofv3 --kernel-trace), us per launch: median over launches, '
                   'spread of the per-round medians (max - min)', 'rounds': TRACE_ROUNDS, 'keys': {}}
    for key in sorted(durs):
        rec = {}
        for kern, prec in (('conv_mfma_kernel', 'fp32'), ('conv_b3_kernel', 'bf16x3')):
            ds = [d for _, d in sorted(durs[key].get(kern, []))]
            per_round = len(ds) // (TRACE_ROUNDS + 1)
            rounds = [ds[i * per_round:(i + 1) * per_round] for i in range(1, TRACE_ROUNDS + 1)] if per_round else []
            meds = [statistics.median(r) for r in rounds]
            rec[prec] = {'launches': len(ds), 'median_us': statistics.median([d for r in rounds for d in r]) if meds else None,
                         'spread_us': (max(meds) - min(meds)) if meds else None}
        if rec['fp32']['median_us'] is not None and rec['bf16x3']['median_us'] is not None:
            rec['gain_us'] = rec['fp32']['median_us'] - rec['bf16x3']['median_us']
            rec['faster'] = bool(rec['gain_us'] > 2 * rec['fp32']['spread_us'])
        out['keys'][key] = rec
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['steps', 'trace', 'kernels'])
    ap.add_argument('dir', nargs='?')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--out')
    a = ap.parse_args()
    {'steps': steps, 'trace': trace, 'kernels': kernels}[a.mode](a)
