"""Write tests/golden/metrics_summary.npz: 40 hand-sized cases of 4 agents fed through the REFERENCE's own
MonitoringMultiAgentPerformance.update() / summary() (utils/metrics.py of a checkout of the reference, imported from
--reference), with the inputs and the numbers the reference reports.  Recorded data only: per-case tables in the layout of
include/gnnpp_rollout_summary.h, the reference's rates, its per-case list of agents that reached, and the tags and values
its summary() handed to a writer for the label 'valid'.

    python tools/gen_metrics_golden.py --reference /path/to/reference [--out tests/golden/metrics_summary.npz]

The per-case flags of update()'s log_result are formed here from the tables, by the definitions of the header: every agent
reached; not every agent reached and one that did not was shielded; every agent reached at no more than the expert's costs;
audit_ok; some agent was shielded.  The reference only counts them.  Needs the reference's imports (torch, numpy, scipy).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tables(C=40, N=4, seed=20240611):
    rng = np.random.RandomState(seed)
    i32 = np.int32
    reached = (rng.rand(C, N) < 0.85).astype(i32)
    reached[:3] = 1                                           # (some cases reach for sure, one is optimal for sure)
    makespan = rng.randint(4, 40, C)
    stats = np.stack([makespan, makespan * N - rng.randint(0, 2 * N, C)], 1).astype(i32)
    targets = np.stack([np.maximum(makespan - rng.randint(0, 6, C), 2), rng.randint(6, 30 * N, C)], 1).astype(i32)
    targets[0] = stats[0]
    shielded = (rng.rand(C, N) < 0.25).astype(i32) * rng.randint(1, 6, (C, N)).astype(i32)
    audit_ok = (rng.rand(C) < 0.7).astype(i32)
    return reached, stats, targets, shielded, audit_ok


class Recorder:
    def __init__(self):
        self.tags, self.values, self.steps = [], [], []

    def add_scalar(self, tag, value, step):
        self.tags.append(tag)
        self.values.append(float(value))
        self.steps.append(int(step))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='a checkout of the reference (the directory that holds utils/)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'metrics_summary.npz'))
    args = ap.parse_args()
    # utils/metrics.py is loaded as a file of its own: the package's __init__ imports every module of utils/, the
    # plotting ones and their dependencies included, and the class needs none of them
    import importlib.util
    spec = importlib.util.spec_from_file_location('reference_metrics',
                                                  os.path.join(os.path.abspath(args.reference), 'utils', 'metrics.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    MonitoringMultiAgentPerformance = mod.MonitoringMultiAgentPerformance

    reached, stats, targets, shielded, audit_ok = tables()
    C, N = reached.shape
    mon = MonitoringMultiAgentPerformance(None)
    mon.reset()
    for c in range(C):
        r, s = reached[c] > 0, shielded[c] > 0
        all_reach = bool(r.all())
        mp, ft, tm, tf = int(stats[c, 0]), int(stats[c, 1]), int(targets[c, 0]), int(targets[c, 1])
        mon.update(0, [all_reach, bool(not all_reach and (s & ~r).any()), bool(all_reach and mp <= tm and ft <= tf),
                       bool(audit_ok[c]), bool(s.any()), [mp, tm], [ft, tf], int(r.sum()), None, None, 0.0, []])
    rec = Recorder()
    mon.summary('valid', rec, 7)
    np.savez(args.out, reached=reached, stats=stats, targets=targets, shielded=shielded, audit_ok=audit_ok,
             rateReachGoal=mon.rateReachGoal, rateFailedReachGoalSH=mon.rateFailedReachGoalSH,
             ratefindOptimalSolution=mon.ratefindOptimalSolution, rateCollsionFreeSol=mon.rateCollsionFreeSol,
             rateCollisionPredictedinLoop=mon.rateCollisionPredictedinLoop,
             avg_rate_deltaMP=mon.avg_rate_deltaMP, std_rate_deltaMP=mon.std_rate_deltaMP,
             avg_rate_deltaFT=mon.avg_rate_deltaFT, std_rate_deltaFT=mon.std_rate_deltaFT,
             list_numAgentReachGoal=np.array(mon.list_numAgentReachGoal, np.int64),
             hist_numAgentReachGoal=np.array([mon.list_numAgentReachGoal.count(i) for i in range(N + 1)], np.int64),
             list_rate_deltaMP=np.array(mon.list_rate_deltaMP), list_rate_deltaFT=np.array(mon.list_rate_deltaFT),
             scalar_tags=np.array(rec.tags), scalar_values=np.array(rec.values), scalar_epoch=np.array(rec.steps))
    print('wrote', args.out, 'reach rate %.3f' % mon.rateReachGoal)


if __name__ == '__main__':
    main()
