#!/usr/bin/env python3
"""Time the maze-map launch (gnnpp_casegen_maze) on the MI355X -> profiles/casegen_maze.json.

    python tools/casegen_maze_bench.py [--out profiles/casegen_maze.json]

Per shape: the launch alone on preallocated outputs, HIP events around windows of `--window` launches after `--warmup`
launches, the median window (with the fastest and the slowest) divided by the window's launches -> ms per launch and maps
per second; the same for the gnnpp_casegen launch that takes those maps as its caller maps (closure, starts, goals), so the
two stand next to each other; and as context the plain restatement of the walk (tests/casegen_maze_cases.maze_map, pure
Python) on one core of the same machine's host, on a few maps of the shape.  The maps the device drew for those few are
compared with the restatement's before anything is timed.  There is no CPU fallback: without a device the tool fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SHAPES = (dict(C=4096, H=20, W=20, N=10, density=0.1, complexity=0.01, host_maps=256),
          dict(C=256, H=128, W=128, N=64, density=0.1, complexity=0.01, host_maps=4))


def windows(fn, warmup, window, repeats):
    """ms per call of fn(): [median, min, max] over `repeats` windows of `window` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(window):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / window)
    return [statistics.median(ms), min(ms), max(ms)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'casegen_maze.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--window', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=21)
    ap.add_argument('--seed', type=int, default=1337)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X (no CPU fallback)'
    import casegen_maze_cases as mz
    from gnn_pathplanning_amd import _native, casegen
    _native.lib()
    dev = 'cuda:0'
    rows = []
    for sh in SHAPES:
        C, H, W, N = sh['C'], sh['H'], sh['W'], sh['N']
        raw = torch.empty((C, H, W), dtype=torch.uint8, device=dev)
        words = torch.empty((C,), dtype=torch.int32, device=dev)
        cases = casegen.empty_cases(C, N, H, W, dev)

        def maze():
            casegen.enqueue_maze_maps(raw, sh['density'], sh['complexity'], seed=args.seed, words=words)

        def closure():
            casegen.enqueue_generate(cases, seed=args.seed, grids=raw)

        maze()
        torch.cuda.synchronize()
        walls, steps = mz.counts_of(H, W, sh['density'], sh['complexity'])
        t0 = time.perf_counter()
        host = [mz.maze_map(H, W, walls, steps, (args.seed + c) % 2 ** 32) for c in range(sh['host_maps'])]
        host_s = time.perf_counter() - t0
        got, got_words = raw[:sh['host_maps']].cpu().numpy(), words[:sh['host_maps']].cpu().numpy()
        for c, (m, w) in enumerate(host):
            assert (got[c] == m).all() and got_words[c] == w, ('device and restatement differ', H, W, c)
        t_maze = windows(maze, args.warmup, args.window, args.repeats)
        t_closure = windows(closure, args.warmup, args.window, args.repeats)
        row = dict(C=C, H=H, W=W, density=sh['density'], complexity=sh['complexity'], walls=walls, steps=steps,
                   words_mean=float(words.float().mean()), words_max=int(words.max()),
                   maze_ms_median_min_max=t_maze, maze_maps_per_s=C / (t_maze[0] * 1e-3),
                   casegen_agents=N, casegen_ms_median_min_max=t_closure,
                   host_restatement_maps=sh['host_maps'], host_restatement_maps_per_s=sh['host_maps'] / host_s,
                   ok_cases=int(cases.ok.sum()))
        print(json.dumps(row))
        rows.append(row)
    doc = dict(tool='tools/casegen_maze_bench.py', device=torch.cuda.get_device_name(0), warmup=args.warmup,
               window=args.window, repeats=args.repeats, seed=args.seed,
               note='HIP events around windows of launches, outputs preallocated; host = the pure-Python restatement on '
                    'one core of the same machine, as context only', shapes=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
