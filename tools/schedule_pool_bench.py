"""Time a draw from expert.SchedulePool (gnnpp_schedule_draw: the batch is built from the stored schedules) against the
same draw from the materialised pools (expert.SamplePool / SampleListPool: an index gather), and an append to each.

    python tools/schedule_pool_bench.py [--reps 200] [--append-cases 10000,1000] [--out FILE]

Per shape -- 64 x 10 agents dense, 16 x 100 agents dense, 4 x 1024 agents lists -- both pools hold the same synthetic
walks (tools/expert_bench.py::synthetic_walks), the two gathers are checked equal, then timed ALTERNATELY, each call on a
host clock that ends in a device synchronise (a gather allocates its outputs: that is part of what a caller pays); the
figure is the median of --reps warm calls.  The append figures are one call each: a batch of cases appended to a pool
that already holds the first number of --append-cases cases (10-agent teams, 20 steps a case), for SamplePool split into
building the samples (samples_from_schedules) and SamplePool.append itself.  One JSON record per line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from expert_bench import synthetic_walks  # noqa: E402

# (label, agents, map side, cases, steps per case, batch, graph)
SHAPES = (('64 x 10 agents, 20 x 20, dense', 10, 20, 64, 25, 64, 'dense'),
          ('16 x 100 agents, 50 x 50, dense', 100, 50, 16, 25, 16, 'dense'),
          ('4 x 1024 agents, 128 x 128, lists', 1024, 128, 4, 10, 4, 'lists'))


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def walks(rng, N, side, cases, steps):
    made = [synthetic_walks(rng, N, side, steps) for _ in range(cases)]
    return np.stack([m[0] for m in made]), np.stack([m[1] for m in made]), [m[2] for m in made]


def draw_records(expert, reps):
    dev = 'cuda:0'
    rng = np.random.default_rng(7)
    for label, N, side, C, steps, B, graph in SHAPES:
        grids, goals, sched = walks(rng, N, side, C, steps)
        old = expert.SamplePool() if graph == 'dense' else expert.SampleListPool()
        old.append(expert.samples_from_schedules_team(grids, goals, sched, dev, graph=graph))
        new = expert.SchedulePool(dev)
        new.append(grids, goals, sched)
        gen = torch.Generator(device=dev).manual_seed(1)
        picks = [torch.randperm(len(old), generator=gen, device=dev)[:B] for _ in range(reps + 20)]
        a, b = old.gather(picks[0]), new.gather(picks[0], graph)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and (graph == 'lists' or torch.equal(a[2], b[2]))
        ms = {'old': [], 'new': []}
        for i, idx in enumerate(picks):
            t_old = clocked(lambda: old.gather(idx))
            t_new = clocked(lambda: new.gather(idx, graph))
            if i >= 20:
                ms['old'].append(t_old)
                ms['new'].append(t_new)
        held = sum(t.numel() * t.element_size() for t in vars(old).values() if torch.is_tensor(t))
        yield {'what': 'gather of one batch, host clock to a device synchronise, median of %d warm calls, alternating' % reps,
               'shape': label, 'steps_held': len(old), 'batch': B, 'graph': graph,
               'materialised_pool_ms': round(float(np.median(ms['old'])), 4),
               'schedule_pool_ms': round(float(np.median(ms['new'])), 4),
               'materialised_pool_ms_p10_p90': [round(float(np.percentile(ms['old'], q)), 4) for q in (10, 90)],
               'schedule_pool_ms_p10_p90': [round(float(np.percentile(ms['new'], q)), 4) for q in (10, 90)],
               'materialised_pool_bytes': held, 'schedule_pool_bytes': new.nbytes}
        del old, new
        torch.cuda.empty_cache()


def append_record(expert, held_cases, batch_cases):
    dev, N, side, steps = 'cuda:0', 10, 20, 20
    rng = np.random.default_rng(11)
    distinct = walks(rng, N, side, 250, steps)

    def tiled(cases):
        k = [i % 250 for i in range(cases)]
        return distinct[0][k], distinct[1][k], [distinct[2][i] for i in k]
    first, batch = tiled(held_cases), tiled(batch_cases)
    old, new = expert.SamplePool(), expert.SchedulePool(dev)
    old.append(expert.samples_from_schedules(*first, dev))
    new.append(*first)
    built = []
    t_build = clocked(lambda: built.append(expert.samples_from_schedules(*batch, dev)))
    t_old = clocked(lambda: old.append(built[0]))
    t_new = clocked(lambda: new.append(*batch))
    assert len(old) == len(new) == (held_cases + batch_cases) * steps
    return {'what': 'one append of %d cases (%d agents, %d steps each) to a pool that holds %d cases, host clock to a device '
                    'synchronise, one call each' % (batch_cases, N, steps, held_cases),
            'samples_from_schedules_ms': round(t_build, 3), 'sample_pool_append_ms': round(t_old, 3),
            'schedule_pool_append_ms': round(t_new, 3),
            'sample_pool_bytes': sum(t.numel() * t.element_size() for t in (old.input, old.target, old.GSO)),
            'schedule_pool_bytes': new.nbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--append-cases', default='10000,1000', help='cases held, cases appended')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X: a CPU run measures nothing'
    from gnn_pathplanning_amd import expert
    records = []
    for rec in draw_records(expert, a.reps):
        print(json.dumps(rec), flush=True)
        records.append(rec)
    held, batch = (int(v) for v in a.append_cases.split(','))
    records.append(append_record(expert, held, batch))
    print(json.dumps(records[-1]), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'records': records}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
