"""Time one gnnpp_mapf_solve / gnnpp_mapf_team_solve call: cases per second and agent-plans per second.

    python tools/mapf_bench.py [--reps 10] [--out profiles/mapf_solve.json] [--only NAME] [--cpu-cases 16]
    python tools/mapf_bench.py --team [--reps 10] [--out profiles/mapf_team_solve.json] [--only NAME] [--cpu-cases 2]
    python tools/mapf_bench.py --priorities [--reps 10] [--out profiles/mapf_distance.json] [--only NAME]
    python tools/mapf_bench.py --generated [--reps 10] [--out profiles/casegen.json] [--only NAME] [--cpu-cases 2]
    python tools/mapf_bench.py --audit [--reps 10] [--out profiles/mapf_audit.json] [--only NAME] [--cpu-cases 2]

Configurations (random maps of tests/expert_cases.random_map at density 0.1, horizon 4 (H + W)): 512 cases x 10 agents
on 20 x 20 with R = 1 and R = 4 orders, 256 x 20 on 20 x 20, 128 x 64 on 40 x 40.  Outputs and workspace are
preallocated; the call is timed with HIP events after 3 warm-up calls, mean over --reps calls.  An agent-plan is one
agent planned in one restart (C * R * N per call, whether or not the case is solved).  Beside each GPU rate: the
sequential numpy restatement (tests/mapf_cases.py) on the first --cpu-cases cases of the same inputs, on the host, as
context (it is the yardstick, not a tuned CPU solver).  --only NAME runs one configuration (for a profiler run).

--team: mapf.solve_team's call (one workgroup per case) at the B x N shapes of the large-team rollouts -- 64 cases x 160
agents on 64 x 64 (R = 1 and R = 4), 16 x 512 on 100 x 100, 8 x 1024 on 128 x 128 -- and, for comparison with the
one-wave call on inputs both accept, 128 x 64 on 40 x 40 (timed through BOTH calls, outputs compared).  A case is planned
by one workgroup from its first agent to its last, so a call lasts as long as its slowest case: us_per_step_or_hop = call
time / (2 x the largest flowtime), the time of one forward search step or one walk-back hop (a flowtime of F means F steps
forward and F hops back; commit, t_min scan and the per-case set-up are inside this figure, so it is an upper bound).

--priorities: the planning orders ranked on the device from true goal distances (csrc/mapf_distance_kernels.hip) on the
inputs of both lists above (each set of inputs once, through the call its list times it with).  Per configuration and
per choice of orders -- None with R = 1 (the index order), None with R = 4 (the index order and three host-drawn
permutations, mapf.default_orders), 'longest_first' (R = 1), 'mixed' with R = 4 -- the solved count and the time of the
whole call (for the string forms: the distance, bounds and order launches and the solve, enqueued back to back), and
the distance + bounds launches and the order launch timed on their own, with their share of the whole call.

--generated: the configurations of --priorities on cases GENERATED on the device (casegen.generate, csrc/casegen_kernels.hip)
at the same density, next to the host-drawn cases of the same configuration: the time of one gnnpp_casegen call (HIP
events, outputs preallocated), the agents with dist < 0 (0 by construction on generated cases: asserted), and the solved
counts under None (the index order), 'longest_first' and 'mixed' with R = 4 for both kinds of cases.  Beside the call's
time: the numpy / queue yardstick (tests/casegen_cases.py) on the first --cpu-cases cases, on one host core, as context.

--audit: the schedule audit (mapf.enqueue_audit, csrc/mapf_audit_kernels.hip) on the schedules the solver produced for the
configurations of --priorities on GENERATED cases (so that the cases are solvable), index order, steps = the solver's
makespan: the time of one gnnpp_mapf_audit call (HIP events, outputs and workspace preallocated) next to the time of the
solve call it checks, measured in the same process, the audit as a share of it, and the bytes of schedule the audit reads
per second (rows 0 .. makespan of the solved cases, once).  Every solved case must audit clean with the solver's arrivals
and costs (asserted: a condition, not a measurement).  Beside it the solve time the profiles record for the configuration
on host-drawn cases (profiles/mapf_solve.json, profiles/mapf_team_solve.json), and the sequential restatement
(tests/mapf_audit_cases.py) on the first --cpu-cases cases as context.
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

CONFIGS = (('c512_n10_20x20_r1', 512, 10, 20, 1), ('c512_n10_20x20_r4', 512, 10, 20, 4),
           ('c256_n20_20x20_r1', 256, 20, 20, 1), ('c128_n64_40x40_r1', 128, 64, 40, 1))
TEAM_CONFIGS = (('team_c128_n64_40x40_r1', 128, 64, 40, 1), ('team_c64_n160_64x64_r1', 64, 160, 64, 1),
                ('team_c64_n160_64x64_r4', 64, 160, 64, 4), ('team_c16_n512_100x100_r1', 16, 512, 100, 1),
                ('team_c8_n1024_128x128_r1', 8, 1024, 128, 1))


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


def priorities_records(a, mc, mapf, dev):
    """--priorities: one record per distinct set of inputs of CONFIGS and TEAM_CONFIGS."""
    records, seen = [], set()
    for team, (name, C, N, side, _) in [(False, c) for c in CONFIGS] + [(True, c) for c in TEAM_CONFIGS]:
        name = name.rsplit('_r', 1)[0]
        if (a.only and name != a.only) or name in seen:
            continue
        seen.add(name)
        rng = np.random.default_rng(C * N + side)
        cases = mc.random_cases(rng, C, N, side, density=0.1)
        T = mc.default_horizon(side, side)
        grid = torch.from_numpy(np.stack([c[0] for c in cases])).to(dev)
        start = torch.from_numpy(np.stack([c[1] for c in cases]).astype(np.int32)).to(dev)
        goal = torch.from_numpy(np.stack([c[2] for c in cases]).astype(np.int32)).to(dev)
        enqueue = mapf.enqueue_solve_team if team else mapf.enqueue_solve
        dist = mapf.Distances(*(torch.empty(shape, dtype=torch.int32, device=dev) for shape in ((C, N), (C,), (C,))))
        rec = {'config': name, 'call': 'gnnpp_mapf_team_solve' if team else 'gnnpp_mapf_solve', 'cases': C, 'agents': N,
               'map': '%dx%d' % (side, side), 'T_max': T,
               'what': 'HIP events, mean of %d calls after 3; outputs and orders preallocated' % a.reps}
        rec['distances_ms'] = round(timed(lambda: mapf.enqueue_distances(grid, start, goal, dist), a.reps) * 1e3, 4)
        torch.cuda.synchronize()
        rec['unreachable_agents'] = int((dist.dist < 0).sum().item())
        rec['lower_makespan_max'] = int(dist.lower_makespan.max().item())
        for label, prio, R in (('none_r1', None, 1), ('none_r4', None, 4), ('longest_first', 'longest_first', 1),
                               ('mixed_r4', 'mixed', 4)):
            out = (mapf.empty_solutions(C, N, side, T, dev, R, W=side, team=True) if team
                   else mapf.empty_solutions(C, N, side, T, dev, R))
            if prio is None:
                order = (torch.from_numpy(mapf.default_orders(C, N, R, 0).astype(np.int32)).to(dev) if R > 1 else None)
                sec = timed(lambda: enqueue(grid, start, goal, order, out), a.reps)
            else:
                rules = [mapf.ORDER_RULES[r] for r in (['index', 'longest_first', 'shortest_first', 'hashed']
                                                       if prio == 'mixed' else [prio])]
                order = torch.empty((C, R, N), dtype=torch.int32, device=dev)
                rec[label + '_orders_ms'] = round(timed(lambda: mapf.enqueue_orders(dist.dist, rules, 0, order),
                                                        a.reps) * 1e3, 4)

                def chain():
                    mapf.enqueue_distances(grid, start, goal, dist)
                    mapf.enqueue_orders(dist.dist, rules, 0, order)
                    enqueue(grid, start, goal, order, out)
                sec = timed(chain, a.reps)
                rec[label + '_distance_and_order_share'] = round(
                    (rec['distances_ms'] + rec[label + '_orders_ms']) / (sec * 1e3), 4)
            rec[label + '_ms_per_call'] = round(sec * 1e3, 4)
            rec[label + '_solved'] = int((out.status == 0).sum().item())
            flow = out.flowtime[out.status == 0]
            rec[label + '_flowtime_mean_of_solved'] = round(float(flow.double().mean().item()), 1) if flow.numel() else None
            del out, order
            torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)
        records.append(rec)
    return records


def generated_records(a, mc, mapf, dev):
    """--generated: one record per distinct set of inputs of CONFIGS and TEAM_CONFIGS."""
    import casegen_cases as cc
    from gnn_pathplanning_amd import casegen
    records, seen = [], set()
    for team, (name, C, N, side, _) in [(False, c) for c in CONFIGS] + [(True, c) for c in TEAM_CONFIGS]:
        name = name.rsplit('_r', 1)[0]
        if (a.only and name != a.only) or name in seen:
            continue
        seen.add(name)
        seed = C * N + side
        cases = mc.random_cases(np.random.default_rng(seed), C, N, side, density=0.1)
        drawn = tuple(torch.from_numpy(np.stack([c[k] for c in cases]).astype(np.uint8 if k == 0 else np.int32)).to(dev)
                      for k in range(3))
        out = casegen.empty_cases(C, N, side, side, dev)
        sec = timed(lambda: casegen.enqueue_generate(out, density=0.1, seed=seed), a.reps)
        torch.cuda.synchronize()
        rec = {'config': name, 'call': 'gnnpp_casegen', 'cases': C, 'agents': N, 'map': '%dx%d' % (side, side),
               'density': 0.1, 'seed': seed,
               'what': 'HIP events, mean of %d calls after 3; outputs preallocated' % a.reps,
               'casegen_ms_per_call': round(sec * 1e3, 4), 'casegen_cases_per_s': round(C / sec),
               'too_small_cases': int((out.status != 0).sum().item()),
               'cells_min': int(out.cells.min().item()), 'cells_mean': round(float(out.cells.double().mean().item()), 1),
               'obstacles_mean': round(float(out.grid.sum((1, 2)).double().mean().item()), 1)}
        k = min(a.cpu_cases, C)
        t0 = time.perf_counter()
        want = cc.generate(k, N, side, side, casegen.threshold_of(0.1), seed) if k else None
        rec['cpu_yardstick_cases_per_s'] = round(k / (time.perf_counter() - t0), 2) if k else None
        rec['cpu_yardstick_cases_timed'] = k
        rec['cpu_yardstick_agrees'] = all(np.array_equal(getattr(out, key)[:k].cpu().numpy(), want[key])
                                          for key in cc.OUTPUTS) if k else None
        solve = mapf.solve_team if team else mapf.solve
        for kind, (grid, start, goal) in (('generated', (out.grid, out.start, out.goal)), ('host_drawn', drawn)):
            d = mapf.distances(grid, start, goal, dev)
            rec[kind + '_agents_without_path'] = int((d.dist < 0).sum().item())
            rec[kind + '_cases_with_such_an_agent'] = int((d.dist < 0).any(1).sum().item())
            for label, prio, R in (('none_r1', None, 1), ('longest_first', 'longest_first', 1), ('mixed_r4', 'mixed', 4)):
                sol = solve(grid, start, goal, dev, restarts=R, priorities=prio)
                rec['%s_%s_solved' % (kind, label)] = int((sol.status == 0).sum().item())
                del sol
                torch.cuda.empty_cache()
        assert rec['generated_agents_without_path'] == 0, rec        # a condition of the contract, not a measurement
        print(json.dumps(rec), flush=True)
        records.append(rec)
    return records


def audit_records(a, mc, mapf, dev):
    """--audit: one record per distinct set of inputs of CONFIGS and TEAM_CONFIGS."""
    import mapf_audit_cases as ac
    from gnn_pathplanning_amd import casegen
    recorded = {}
    for path in ('mapf_solve.json', 'mapf_team_solve.json'):
        try:
            with open(os.path.join(ROOT, 'profiles', path)) as f:
                recorded.update({r['config']: r['ms_per_call'] for r in json.load(f)['records']})
        except (OSError, KeyError, ValueError):
            pass
    records, seen = [], set()
    for team, (full, C, N, side, _) in [(False, c) for c in CONFIGS] + [(True, c) for c in TEAM_CONFIGS]:
        name = full.rsplit('_r', 1)[0]
        if (a.only and name != a.only) or name in seen:
            continue
        seen.add(name)
        seed = C * N + side
        T = mc.default_horizon(side, side)
        cases = casegen.generate(C, N, side, side, dev, density=0.1, seed=seed)
        out = (mapf.empty_solutions(C, N, side, T, dev, 1, W=side, team=True) if team
               else mapf.empty_solutions(C, N, side, T, dev, 1))
        enqueue = mapf.enqueue_solve_team if team else mapf.enqueue_solve
        solve_sec = timed(lambda: enqueue(cases.grid, cases.start, cases.goal, None, out), a.reps)
        found = mapf.empty_audit(C, N, T, dev)
        sec = timed(lambda: mapf.enqueue_audit(cases.grid, cases.start, cases.goal, out.schedules, out.makespan, found),
                    a.reps)
        torch.cuda.synchronize()
        solved = out.status == 0
        assert bool((found.status[solved] == 0).all()) and bool((found.status[~solved] == mapf.AUDIT_SKIPPED).all())
        assert torch.equal(found.arrival[solved], out.arrival[solved])
        assert torch.equal(found.flowtime[solved], out.flowtime[solved])
        rows = int((out.makespan[solved] + 1).sum().item())
        rec = {'config': name, 'call': 'gnnpp_mapf_audit', 'cases': C, 'agents': N, 'map': '%dx%d' % (side, side),
               'T_max': T, 'chunk': mapf.AUDIT_CHUNK,
               'what': 'HIP events, mean of %d calls after 3; outputs and workspace preallocated; generated cases '
                       '(density 0.1, seed %d), index order, steps = makespan' % (a.reps, seed),
               'solved': int(solved.sum().item()), 'makespan_max': int(out.makespan.max().item()), 'rows_audited': rows,
               'audit_ms_per_call': round(sec * 1e3, 4),
               'solve_call': 'gnnpp_mapf_team_solve' if team else 'gnnpp_mapf_solve',
               'solve_ms_per_call_same_process': round(solve_sec * 1e3, 4),
               'audit_share_of_solve': round(sec / solve_sec, 5),
               'solve_ms_per_call_recorded_host_drawn': recorded.get(full),
               'schedule_GB_read_per_s': round(rows * N * 8 / sec / 1e9, 3),
               'workspace_MB': round(found.workspace.numel() / 2 ** 20, 3)}
        k = min(a.cpu_cases, C, 0 if N >= 160 else C)       # (the restatement looks for swaps in O(N^2) per step)
        if k:
            case = ac.make_case(name, cases.grid[:k].cpu().numpy(), cases.goal[:k].cpu().numpy(),
                                out.schedules[:k].cpu().numpy(), start=cases.start[:k].cpu().numpy(),
                                steps=out.makespan[:k].cpu().numpy())
            t0 = time.perf_counter()
            want = ac.audit(case)
            rec['cpu_restatement_cases_per_s'] = round(k / (time.perf_counter() - t0), 2)
            rec['cpu_restatement_agrees'] = all(np.array_equal(getattr(found, key)[:k].cpu().numpy(), want[key])
                                                for key in ac.OUTPUTS)
        rec['cpu_restatement_cases_timed'] = k
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del out, found, cases
        torch.cuda.empty_cache()
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--only', default=None)
    ap.add_argument('--cpu-cases', type=int, default=None)
    ap.add_argument('--team', action='store_true')
    ap.add_argument('--priorities', action='store_true',
                    help='compare the planning orders: None, longest_first, mixed (see the module docstring)')
    ap.add_argument('--generated', action='store_true',
                    help='the --priorities configurations on cases generated on the device (see the module docstring)')
    ap.add_argument('--audit', action='store_true',
                    help='time the schedule audit next to the solve it checks (see the module docstring)')
    a = ap.parse_args()
    if a.cpu_cases is None:
        a.cpu_cases = 2 if a.team or a.generated or a.audit else 16
    assert torch.cuda.is_available(), 'needs the MI355X: a CPU run measures nothing'
    import mapf_cases as mc
    from gnn_pathplanning_amd import mapf
    dev = torch.device('cuda:0')
    records = (priorities_records(a, mc, mapf, dev) if a.priorities else
               generated_records(a, mc, mapf, dev) if a.generated else
               audit_records(a, mc, mapf, dev) if a.audit else [])
    for name, C, N, side, R in (() if a.priorities or a.generated or a.audit else TEAM_CONFIGS if a.team else CONFIGS):
        if a.only and name != a.only:
            continue
        rng = np.random.default_rng(C * N + side)
        cases = mc.random_cases(rng, C, N, side, density=0.1)
        T = mc.default_horizon(side, side)
        grid = torch.from_numpy(np.stack([c[0] for c in cases])).to(dev)
        start = torch.from_numpy(np.stack([c[1] for c in cases]).astype(np.int32)).to(dev)
        goal = torch.from_numpy(np.stack([c[2] for c in cases]).astype(np.int32)).to(dev)
        orders = np.stack([np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(R - 1)]) for _ in cases])
        order = torch.from_numpy(orders.astype(np.int32)).to(dev) if R > 1 else None
        extra = {}
        if a.team:
            out = mapf.empty_solutions(C, N, side, T, dev, R, W=side, team=True)
            sec = timed(lambda: mapf.enqueue_solve_team(grid, start, goal, order, out), a.reps)
            flow = out.flowtime.clamp(min=0)
            extra = {'flowtime_sum': int(flow.sum().item()), 'flowtime_max': int(flow.max().item()),
                     'us_per_step_or_hop': round(sec * 1e6 / max(1, 2 * int(flow.max().item())), 4)}
            if N <= mapf.MAX_AGENTS and side <= mapf.MAX_SIDE:          # the one-wave call on the same inputs
                small = mapf.empty_solutions(C, N, side, T, dev, R)
                sec_small = timed(lambda: mapf.enqueue_solve(grid, start, goal, order, small), a.reps)
                extra['one_wave_call_ms'] = round(sec_small * 1e3, 4)
                extra['one_wave_call_same_outputs'] = all(
                    torch.equal(getattr(out, k), getattr(small, k))
                    for k in ('schedules', 'arrival', 'makespan', 'flowtime', 'status', 'failing', 'restart'))
                del small
        else:
            out = mapf.empty_solutions(C, N, side, T, dev, R)
            sec = timed(lambda: mapf.enqueue_solve(grid, start, goal, order, out), a.reps)
        solved = int((out.status == 0).sum().item())
        k = min(a.cpu_cases, C, 1 if N >= 512 else C)        # (--cpu-cases 0: a profiler run, no yardstick)
        t0 = time.perf_counter()
        cpu = [mc.solve_case(g, s, gl, T, None if R == 1 else list(orders[c])) for c, (g, s, gl) in enumerate(cases[:k])]
        cpu_sec = (time.perf_counter() - t0) / max(k, 1)
        same = all(int(out.status[c]) == w['status'] and int(out.flowtime[c]) == w['flowtime'] for c, w in enumerate(cpu))
        rec = {'config': name, 'what': '%s, one call, HIP events, mean of %d calls after 3' % (
               'gnnpp_mapf_team_solve' if a.team else 'gnnpp_mapf_solve', a.reps),
               'cases': C, 'agents': N, 'map': '%dx%d' % (side, side), 'restarts': R, 'T_max': T,
               'ms_per_call': round(sec * 1e3, 4), 'cases_per_s': round(C / sec),
               'agent_plans_per_s': round(C * R * N / sec), 'solved': solved,
               'makespan_max': int(out.makespan.max().item()),
               'workspace_MB': round(out.workspace.numel() / 2 ** 20, 1),
               'cpu_yardstick_cases_per_s': round(1 / cpu_sec, 2) if k else None, 'cpu_yardstick_cases_timed': k,
               'cpu_yardstick_agrees': same}
        rec.update(extra)
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del out
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'records': records}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
