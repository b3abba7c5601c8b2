"""Time one gnnpp_schedule_samples call: agent-samples per second and achieved write bandwidth.

    python tools/expert_bench.py [--agents 10] [--side 20] [--steps 1000,32000,256000] [--reps 10] [--out FILE]
    python tools/expert_bench.py --team [--lists] [--only 0,2] [--reps 10] [--out FILE]

Synthetic solved cases (tests/expert_cases.py: ~25 steps each, 64 distinct ones tiled up to the requested number of
steps) are transformed in ONE call, outputs preallocated, timed with HIP events after warm-up, mean over --reps calls.
The rate is set against the bytes the call MUST write, T_total * N * (3 * 121 * 4 + 4 * N + 5 * 4) (observations, fp32
GSO, targets), over the HBM peak bench.py's roofline uses.  One JSON record per size; --out collects them in a file.

--team times gnnpp_schedule_team_samples (5 launches) on its own fixed sizes (TEAM_SIZES): synthetic walks -- every
agent takes a random legal move or waits, the goal is where it ends -- because the call's time does not depend on whose
schedule it is.  The 1024-agent sizes are also run with S starting 4 bytes past a 16-byte boundary (the 4-byte store
path), and the 128-agent size through BOTH entry points.  --lists adds, per size and in the same process, the route that
keeps the graphs as capped neighbour lists: gnnpp_schedule_team_plan + gnnpp_schedule_team_fill_lists (6 launches) with
cap = the largest degree rounded up to 4, read from an untimed plan; its bytes are observations, targets and the lists.
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

HBM_PEAK_TBPS = 8.0                     # bench.py::HBM_PEAK_TBPS


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
    return t0.elapsed_time(t1) * 1e-3 / reps                           # seconds per call


# (label, agents, map side, cases, steps per case)
TEAM_SIZES = (('8 x 1024 agents, 128 x 128', 1024, 128, 8, 100),
              ('64 x 256 agents, 100 x 100', 256, 100, 64, 50),
              ('1 x 1024 agents, 3 steps (the few-steps corner)', 1024, 128, 1, 3),
              ('64 x 128 agents, 40 x 40', 128, 40, 64, 50))


def synthetic_walks(rng, N, side, steps):
    """(grid, goal [N,2], schedule [steps,N,2]): random legal moves on a random map (agents ignore each other)."""
    grid = (rng.random((side, side)) < 0.1).astype(np.uint8)
    free = np.argwhere(grid == 0)
    pos = free[rng.choice(len(free), size=N, replace=False)]
    delta = np.array([[-1, 0], [0, -1], [1, 0], [0, 1], [0, 0]])
    sched = [pos]
    for _ in range(steps):                              # one more state than steps: the last one is the goal
        nxt = sched[-1] + delta[rng.integers(0, 5, N)]
        inside = ((nxt >= 0) & (nxt < side)).all(-1)
        ok = inside & (grid[np.clip(nxt[:, 0], 0, side - 1), np.clip(nxt[:, 1], 0, side - 1)] == 0)
        sched.append(np.where(ok[:, None], nxt, sched[-1]))
    return grid, sched[-1].astype(np.int32), np.stack(sched[:-1]).astype(np.int32)


def team_main(a):
    from gnn_pathplanning_amd import _native, expert
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(7)
    only = None if a.only is None else {int(i) for i in a.only.split(',')}
    records = []
    for si, (label, N, side, C, steps) in enumerate(TEAM_SIZES):
        if only is not None and si not in only:
            continue
        made = [synthetic_walks(rng, N, side, steps) for _ in range(C)]
        T = C * steps
        bounds = list(range(0, T + 1, steps))
        grid = torch.from_numpy(np.stack([m[0] for m in made])).to(dev)
        goal = torch.from_numpy(np.stack([m[1] for m in made])).to(dev)
        pos = torch.from_numpy(np.concatenate([m[2] for m in made])).to(dev)
        start = torch.tensor(bounds, dtype=torch.int32, device=dev)
        flat = torch.empty(T * N * N + 4, device=dev)   # (S at a 16-byte boundary, or one float past it)
        nws = _native.lib().gnnpp_schedule_team_workspace_bytes(N, T)

        def outputs(shift):
            return expert.ScheduleSamples(
                input=torch.empty(T, N, 3, 11, 11, device=dev), GSO=flat[shift:shift + T * N * N].view(T, N, N), GSO64=None,
                target=torch.empty(T, N, 5, device=dev), radius=torch.empty(C, dtype=torch.float64, device=dev),
                growth=torch.empty(C, dtype=torch.int32, device=dev), status=torch.empty(C, dtype=torch.int32, device=dev),
                step_growth=torch.empty(T, dtype=torch.int32, device=dev), bounds=bounds,
                workspace=torch.empty(nws, dtype=torch.uint8, device=dev))
        runs = [('gnnpp_schedule_team_samples (5 launches), 16-byte S stores', expert.enqueue_schedule_team_samples, 0)]
        if N == 1024:
            runs.append(('gnnpp_schedule_team_samples (5 launches), S off the 16-byte boundary: 4-byte stores',
                         expert.enqueue_schedule_team_samples, 1))
        if N <= expert.MAX_AGENTS:
            runs.append(('gnnpp_schedule_samples (3 launches)', expert.enqueue_schedule_samples, 0))
        for what, fn, shift in runs:
            out = outputs(shift)
            sec = timed(lambda: fn(grid, goal, pos, start, out), a.reps)
            assert int(out.status.abs().sum().item()) == 0
            nbytes = expert.team_output_bytes(T, N)
            rec = {'what': '%s, one call, HIP events, mean of %d calls after 3' % (what, a.reps), 'size': label,
                   'agents': N, 'map': '%dx%d' % (side, side), 'cases': C, 'steps': T,
                   'growths': sorted(set(out.growth.tolist())), 'ms_per_call': round(sec * 1e3, 4),
                   'agent_samples_per_s': round(T * N / sec), 'steps_per_s': round(T / sec),
                   'bytes_written_min': nbytes, 'write_GBps': round(nbytes / sec / 1e9, 1),
                   'frac_of_hbm_peak_%gTBps' % HBM_PEAK_TBPS: round(nbytes / sec / (HBM_PEAK_TBPS * 1e12), 4)}
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del out
        if a.lists:
            out = outputs(0)
            out.GSO = None
            out.step_deg = torch.empty(T, dtype=torch.int32, device=dev)
            expert.enqueue_schedule_team_plan(grid, goal, pos, start, out)
            out.cap = cap = max(4, (int(out.step_deg.max().item()) + 3) & ~3)
            out.cnt = torch.empty(T, N, dtype=torch.int32, device=dev)
            out.idx = torch.empty(T, N, cap, dtype=torch.int16, device=dev)
            out.val = torch.empty(T, N, cap, device=dev)

            def lists_route():
                expert.enqueue_schedule_team_plan(grid, goal, pos, start, out)
                expert.enqueue_schedule_team_fill_lists(grid, goal, pos, start, out)
            sec = timed(lists_route, a.reps)
            assert int(out.status.abs().sum().item()) == 0 and int(out.cnt.max().item()) <= cap
            nbytes = expert.team_lists_output_bytes(T, N, cap)
            rec = {'what': 'gnnpp_schedule_team_plan + gnnpp_schedule_team_fill_lists (6 launches), both calls, HIP events, '
                           'mean of %d calls after 3' % a.reps, 'size': label, 'agents': N, 'map': '%dx%d' % (side, side),
                   'cases': C, 'steps': T, 'cap': cap, 'ms_per_call': round(sec * 1e3, 4),
                   'agent_samples_per_s': round(T * N / sec), 'steps_per_s': round(T / sec), 'bytes_written_min': nbytes,
                   'graph_bytes': T * N * (4 + 6 * cap), 'dense_graph_bytes': 4 * T * N * N,
                   'write_GBps': round(nbytes / sec / 1e9, 1)}
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del out
        del flat, grid, goal, pos
        torch.cuda.empty_cache()
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--team', action='store_true', help='gnnpp_schedule_team_samples on TEAM_SIZES')
    ap.add_argument('--lists', action='store_true', help='--team: also time the capped-lists route (plan + fill_lists)')
    ap.add_argument('--only', default=None, help='--team: indices into TEAM_SIZES, comma separated')
    ap.add_argument('--agents', type=int, default=10)
    ap.add_argument('--side', type=int, default=20)
    ap.add_argument('--steps', default='1000,32000,256000')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X: a CPU run measures nothing'
    import expert_cases as ec
    from gnn_pathplanning_amd import expert
    if a.team:
        records = team_main(a)
        if a.out:
            with open(a.out, 'w') as f:
                json.dump({'device': torch.cuda.get_device_name(0), 'records': records}, f, indent=1)
                f.write('\n')
        return
    dev, N = torch.device('cuda:0'), a.agents
    rng = np.random.default_rng(7)
    made = [ec.random_case(rng, N, a.side, a.side, density=0.1, wait=0.1, max_steps=25) for _ in range(64)]
    sched = [ec.schedule_of(paths, goal) for _, goal, paths in made]
    records = []
    for want in (int(s) for s in a.steps.split(',')):
        grids, goals, parts, T = [], [], [], 0
        while T < want:
            c = len(parts) % len(made)
            part = sched[c][:want - T]
            # (a schedule cut short is a schedule whose goal is the state that followed)
            goals.append(made[c][1] if len(part) == len(sched[c]) else sched[c][len(part)])
            grids.append(made[c][0])
            parts.append(part)
            T += len(part)
        C = len(parts)
        bounds = np.cumsum([0] + [len(p) for p in parts]).tolist()
        grid = torch.from_numpy(np.stack(grids)).to(dev)
        goal = torch.from_numpy(np.stack(goals).astype(np.int32)).to(dev)
        pos = torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(dev)
        start = torch.tensor(bounds, dtype=torch.int32, device=dev)
        out = expert.ScheduleSamples(
            input=torch.empty(T, N, 3, 11, 11, device=dev), GSO=torch.empty(T, N, N, device=dev), GSO64=None,
            target=torch.empty(T, N, 5, device=dev), radius=torch.empty(C, dtype=torch.float64, device=dev),
            growth=torch.empty(C, dtype=torch.int32, device=dev), status=torch.empty(C, dtype=torch.int32, device=dev),
            step_growth=torch.empty(T, dtype=torch.int32, device=dev), bounds=bounds)
        sec = timed(lambda: expert.enqueue_schedule_samples(grid, goal, pos, start, out), a.reps)
        assert int(out.status.abs().sum().item()) == 0
        nbytes = T * N * (3 * 121 * 4 + 4 * N + 5 * 4)
        rec = {'what': 'gnnpp_schedule_samples, one call (3 launches), HIP events, mean of %d calls after 3' % a.reps,
               'agents': N, 'map': '%dx%d' % (a.side, a.side), 'cases': C, 'steps': T, 'ms_per_call': round(sec * 1e3, 4),
               'agent_samples_per_s': round(T * N / sec), 'steps_per_s': round(T / sec),
               'bytes_written_min': nbytes, 'write_GBps': round(nbytes / sec / 1e9, 1),
               'frac_of_hbm_peak_%gTBps' % HBM_PEAK_TBPS: round(nbytes / sec / (HBM_PEAK_TBPS * 1e12), 4)}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del out, grid, goal, pos
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'records': records}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
