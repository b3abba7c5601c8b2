"""Time the summary of a rollout's result tables at the reference's test set, C = 4500 cases x N = 10 agents, on cuda:0:

    device   one gnnpp_rollout_summary launch (device events around `--iters` launches, after a warm-up)
    host     what a caller did before: ten per-case tensors copied to the host as results() copies them, then the numpy
             restatement of the record (tests/rollout_summary_cases.py), by a host clock that starts behind a synchronise

The two are timed alternately, `--rounds` times, and each round's figures are printed; DESIGN.md 5.15 quotes the medians.
Needs the GPU: there is no fallback."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', type=int, default=4500)
    ap.add_argument('--agents', type=int, default=10)
    ap.add_argument('--iters', type=int, default=5000)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    import rollout_summary_cases as rc
    from gnn_pathplanning_amd import _native
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    lib = _native.lib()
    C, N = args.cases, args.agents
    x = rc.inputs(C, N, 1, True, 'one')
    keep = {}

    def ptr(a):
        return keep.setdefault(id(a), torch.from_numpy(np.ascontiguousarray(a)).to(dev)).data_ptr()
    s = rc.fill_struct(_native.RolloutSummaryIn(), x, ptr)
    out = torch.empty(lib.gnnpp_rollout_summary_out_bytes(N, 1), dtype=torch.uint8, device=dev)
    # the tensors results() copies: reached, makespan, flowtime, end_step, start_step, positions, radius, done + slot, t0, lived
    i32 = dict(dtype=torch.int32, device=dev)
    tables = [keep[id(x['reached'])], keep[id(x['stats'])][:, 0], keep[id(x['stats'])][:, 1], torch.zeros(C, N, **i32),
              torch.zeros(C, N, **i32), torch.zeros(C, N, 2, **i32), torch.zeros(C, dtype=torch.float64, device=dev),
              torch.zeros(C, **i32), torch.zeros(C, **i32), torch.zeros(C, **i32)]
    stream = _native.stream_ptr(dev)

    def launches(n):
        for _ in range(n):
            assert lib.gnnpp_rollout_summary(ctypes.byref(s), out.data_ptr(), stream) == 0

    launches(50)
    torch.cuda.synchronize(dev)
    device_us, host_us = [], []
    for r in range(args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launches(args.iters)
        b.record()
        torch.cuda.synchronize(dev)
        device_us.append(a.elapsed_time(b) * 1e3 / args.iters)
        reps = 20
        t0 = time.perf_counter()
        for _ in range(reps):
            host = [t.cpu() for t in tables]
            rc.restate(dict(x, reached=host[0].numpy()))
        host_us.append((time.perf_counter() - t0) * 1e6 / reps)
        print('round %d: device %.2f us per launch (%d launches back to back), host path %.0f us per summary'
              % (r, device_us[-1], args.iters, host_us[-1]))
    print('C = %d, N = %d: median device %.2f us, median host %.0f us' % (C, N, statistics.median(device_us),
                                                                          statistics.median(host_us)))


if __name__ == '__main__':
    main()
