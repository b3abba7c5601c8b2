"""The numbers an evaluation ends at, reduced on the device: what the reference's MonitoringMultiAgentPerformance
(utils/metrics.py) reports for every validation and test run, from a rollout's per-case tables as they lie in HBM.

    summarise(run, targets)  ->  Summary        one launch of gnnpp_rollout_summary (include/gnnpp_rollout_summary.h,
                                                csrc/rollout_summary_kernels.hip), no host synchronisation

`run` is a BatchedRollout, a RolloutStream or a TeamRolloutStream; `targets` the expert's costs.  A Summary holds the
record on the device and copies it to the host when it is first read: host() is the reference's summary under the
reference's names, per_group(g) the same of one group, write_scalars() the reference's tensorboard tags, and
Summary.merge() joins the summaries of the shards of one evaluation exactly (counts, means and the sums of squared
differences, by Chan's formula).  There is no CPU fallback.

Not covered: the reference's time records, its GSO / communication-radius logs and the .mat statistics file.
"""
import ctypes
import math

import numpy as np
import torch

from . import _native

MAX_GROUPS = _native.SUMMARY_MAX_GROUPS
# the reference's five tags of a validation run (utils/metrics.py:186-199) and the key of host() each one carries
SCALAR_TAGS = (('Accuracy_reachGoalNoCollision', 'rateReachGoal'), ('DeteriorationRate_MakeSpan', 'avg_rate_deltaMP'),
               ('DeteriorationRate_FlowTime', 'avg_rate_deltaFT'),
               ('Rate_CollisionPredictedinLoop', 'rateCollisionPredictedinLoop'),
               ('Rate_FailedReachGoalSH', 'rateFailedReachGoalSH'))
# the words of out_i64 by name (GNNPP_SUMMARY_<NAME>)
_I = {k: getattr(_native, 'SUMMARY_' + k.upper()) for k in (
    'n', 'n_reach_all', 'n_optimal', 'agents_reached', 'n_degenerate', 'n_bad_group', 'sum_mp_pred', 'sum_mp_target',
    'sum_ft_pred', 'sum_ft_target', 'min_reached', 'max_reached', 'n_fail_shielded', 'n_collision_free', 'n_shielded')}
_OPTIONAL = ('n_fail_shielded', 'n_collision_free', 'n_shielded')     # -1: the table they are counted from was not given


def _rate(count, n):
    return float(count) / float(n) if n > 0 and count >= 0 else float('nan')


class Summary:
    """The record of one summarise() call: `i64` [G,16] int64, `f64` [G,8] float64 and `hist` [G,N+1] int32 (the layout
    of include/gnnpp_rollout_summary.h), device tensors filled by a launch on the stream summarise() was called on.
    Nothing is copied until host(), per_group() or write_scalars() reads it; that first read synchronises.  A merged
    Summary holds the same three arrays on the host."""

    def __init__(self, i64, f64, hist, keep=()):
        self.i64, self.f64, self.hist = i64, f64, hist
        self.G, self.N = int(i64.shape[0]), int(hist.shape[1]) - 1
        self._keep = keep                                     # the launch's inputs
        self._host = None

    def _read(self):
        """(i64, f64, hist) as numpy arrays."""
        if self._host is None:
            if torch.is_tensor(self.i64):
                torch.cuda.synchronize(self.i64.device)
                self._host = tuple(t.cpu().numpy() for t in (self.i64, self.f64, self.hist))
            else:
                self._host = (self.i64, self.f64, self.hist)
            self._keep = ()
        return self._host

    def per_group(self, g):
        """Group g's summary under the reference's names, plus the counts behind them (`n`, `n_reach_all`, `n_optimal`,
        `n_degenerate`, `n_bad_group`, the cost sums, `min_reached`, `max_reached`, `mean_agents_reached`).  A rate whose
        table was not given (no trace: rateFailedReachGoalSH, rateCollisionPredictedinLoop; no audit: rateCollsionFreeSol)
        is NaN, as is every rate of an empty group."""
        if not 0 <= int(g) < self.G:
            raise _native.GnnppError('Summary.per_group: group %r of %d' % (g, self.G))
        i64, f64, hist = (a[int(g)] for a in self._read())
        out = {k: int(i64[v]) for k, v in _I.items()}
        n = out['n']
        out.update({
            'rateReachGoal': float(f64[_native.SUMMARY_RATE_REACH]),
            'avg_rate_deltaMP': float(f64[_native.SUMMARY_AVG_DMP]), 'std_rate_deltaMP': float(f64[_native.SUMMARY_STD_DMP]),
            'avg_rate_deltaFT': float(f64[_native.SUMMARY_AVG_DFT]), 'std_rate_deltaFT': float(f64[_native.SUMMARY_STD_DFT]),
            'rateFailedReachGoalSH': _rate(out['n_fail_shielded'], n),
            'ratefindOptimalSolution': _rate(out['n_optimal'], n),
            'rateCollsionFreeSol': _rate(out['n_collision_free'], n),
            'rateCollisionPredictedinLoop': _rate(out['n_shielded'], n),
            'list_numAgentReachGoal': [int(v) for v in hist],
            'mean_agents_reached': float(f64[_native.SUMMARY_MEAN_REACHED]),
        })
        return out

    def host(self):
        """The whole evaluation's summary: group 0 of a one-group record as the kernel wrote it, else the groups merged."""
        if self.G == 1:
            return self.per_group(0)
        return Summary.merge([Summary(*(a[g:g + 1] for a in self._read())) for g in range(self.G)]).per_group(0)

    def write_scalars(self, writer, label, epoch):
        """The reference's five `epoch/{label}_set_*` scalars of a validation run, to anything that has add_scalar(tag,
        value, step); returns the writer, as the reference's summary() does."""
        res = self.host()
        for tag, key in SCALAR_TAGS:
            writer.add_scalar('epoch/{}_set_{}'.format(label, tag), res[key], epoch)
        return writer

    @staticmethod
    def merge(parts):
        """One Summary (on the host) of the shards of one evaluation: `parts` are Summaries of the same N and G, such as
        one per rank of sharding.py.  Group by group the counts, cost sums and histograms add, the extremes combine, and
        the deterioration rates are joined from each part's count m = n - n_degenerate, mean and sum of squared
        differences M2 by Chan's formula -- mean = mean_a + d m_b / m, M2 = M2_a + M2_b + d^2 m_a m_b / m with d = mean_b
        - mean_a -- so the result is the summary of the unsplit evaluation up to rounding.  An optional count (shielded,
        audit) is kept only when every part has it."""
        parts = list(parts)
        if not parts:
            raise _native.GnnppError('Summary.merge: no parts')
        G, N = parts[0].G, parts[0].N
        for p in parts:
            if (p.G, p.N) != (G, N):
                raise _native.GnnppError('Summary.merge: parts of G = %d, N = %d and of G = %d, N = %d' % (G, N, p.G, p.N))
        nat = _native
        i64 = np.zeros((G, nat.SUMMARY_I64), np.int64)
        f64 = np.zeros((G, nat.SUMMARY_F64), np.float64)
        hist = np.zeros((G, N + 1), np.int32)
        adds = [v for k, v in _I.items() if k not in ('min_reached', 'max_reached') + _OPTIONAL]
        for g in range(G):
            m, mean, m2 = 0, [0.0, 0.0], [0.0, 0.0]
            lo, hi = None, None
            optional = {k: 0 for k in _OPTIONAL}
            for p in parts:
                pi, pf, ph = (a[g] for a in p._read())
                i64[g, adds] += pi[adds]
                hist[g] += ph
                for k in _OPTIONAL:
                    v = int(pi[_I[k]])
                    optional[k] = -1 if v < 0 or optional[k] < 0 else optional[k] + v
                if pi[nat.SUMMARY_N] == 0:
                    continue
                lo = int(pi[nat.SUMMARY_MIN_REACHED]) if lo is None else min(lo, int(pi[nat.SUMMARY_MIN_REACHED]))
                hi = int(pi[nat.SUMMARY_MAX_REACHED]) if hi is None else max(hi, int(pi[nat.SUMMARY_MAX_REACHED]))
                mb = int(pi[nat.SUMMARY_N] - pi[nat.SUMMARY_N_DEGENERATE])
                if mb == 0:
                    continue
                for j, (avg, sq) in enumerate(((nat.SUMMARY_AVG_DMP, nat.SUMMARY_M2_DMP),
                                               (nat.SUMMARY_AVG_DFT, nat.SUMMARY_M2_DFT))):
                    if m == 0:
                        mean[j], m2[j] = float(pf[avg]), float(pf[sq])
                    else:
                        d = float(pf[avg]) - mean[j]
                        mean[j] += d * mb / (m + mb)
                        m2[j] += float(pf[sq]) + d * d * m * mb / (m + mb)
                m += mb
            n = int(i64[g, nat.SUMMARY_N])
            i64[g, nat.SUMMARY_MIN_REACHED] = -1 if lo is None else lo
            i64[g, nat.SUMMARY_MAX_REACHED] = -1 if hi is None else hi
            for k in _OPTIONAL:
                i64[g, _I[k]] = optional[k]
            nan = float('nan')
            f64[g, nat.SUMMARY_RATE_REACH] = _rate(i64[g, nat.SUMMARY_N_REACH_ALL], n)
            f64[g, nat.SUMMARY_MEAN_REACHED] = _rate(i64[g, nat.SUMMARY_AGENTS_REACHED], n)
            for j, (avg, std, sq) in enumerate(((nat.SUMMARY_AVG_DMP, nat.SUMMARY_STD_DMP, nat.SUMMARY_M2_DMP),
                                                (nat.SUMMARY_AVG_DFT, nat.SUMMARY_STD_DFT, nat.SUMMARY_M2_DFT))):
                f64[g, avg] = mean[j] if m > 0 else nan
                f64[g, std] = math.sqrt(m2[j] / (m - 1)) if m > 1 else nan
                f64[g, sq] = m2[j]
        return Summary(i64, f64, hist)


def _targets(targets, C, N):
    """-> (target_makespan, target_flowtime, stride, valid or None, tensors to keep): views of `targets` where they lie."""
    if torch.is_tensor(targets):
        if targets.dim() != 2 or tuple(targets.shape) != (C, 2):
            raise _native.GnnppError('summarise: targets must be an int32 [C,2] = [%d,2] tensor of (makespan, flowtime) '
                                     '(got %s)' % (C, tuple(targets.shape)))
        if targets.dtype.is_floating_point or targets.dtype is torch.bool:
            raise _native.GnnppError('summarise: targets must hold integers (got %s)' % targets.dtype)
        t = targets.to(torch.int32).contiguous()
        return t, t[:, 1], 2, None, (t,)
    if hasattr(targets, 'status') and hasattr(targets, 'makespan') and hasattr(targets, 'arrival'):     # mapf.Solutions
        what, shape = 'Solutions', tuple(targets.arrival.shape)
        mp, ft, valid = targets.makespan, targets.flowtime, targets.status == 0
    elif hasattr(targets, 'lower_makespan') and hasattr(targets, 'dist'):                                 # mapf.Distances
        what, shape = 'Distances', tuple(targets.dist.shape)
        mp, ft, valid = targets.lower_makespan, targets.lower_flowtime, None
    else:
        raise _native.GnnppError('summarise: targets must be an int32 [C,2] tensor, a mapf.Solutions or a mapf.Distances '
                                 '(got %s)' % type(targets).__name__)
    if shape != (C, N):
        raise _native.GnnppError('summarise: the %s are of C = %d cases of N = %d agents, the run of C = %d, N = %d'
                                 % ((what,) + shape + (C, N)))
    mp, ft = mp.to(torch.int32).contiguous(), ft.to(torch.int32).contiguous()
    return mp, ft, 1, valid, (mp, ft)


def _per_case(x, C, what):
    if not torch.is_tensor(x) or tuple(x.shape) != (C,):
        raise _native.GnnppError('summarise: %s must be an int32 [C] = [%d] tensor (got %s)'
                                 % (what, C, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
    return x.to(torch.int32).contiguous()


def summarise(run, targets, group=None, groups=1, audit=None):
    """The summary of a rollout against the expert's costs: one launch on the current stream, nothing synchronised.

    run      BatchedRollout, RolloutStream or TeamRolloutStream.  Only its device tensors `reached` and `stats` are read,
             of a stream also `lived` (a case that has not ended takes no part; finished slots are harvested first by
             reseat(), as results() does) and, where the run keeps a trace, `trace.shielded`.  results() is not called.
    targets  int32 [C,2] tensor of (makespan, flowtime); or a mapf.Solutions (its costs; an unsolved case takes no part);
             or a mapf.Distances (its lower bounds).
    group    int32 [C] device tensor of group ids 0 .. groups - 1, or None for one group.  groups <= MAX_GROUPS.
    audit    a mapf.Audit of the run's schedules, or an int32 [C] tensor, 1 where a case's schedule has no offence."""
    reached, stats = run.reached, run.stats
    C, N = int(reached.shape[0]), int(reached.shape[1])
    if tuple(stats.shape) != (C, 2):
        raise _native.GnnppError('summarise: run.stats must be [C,2] = [%d,2] (got %s)' % (C, tuple(stats.shape)))
    groups = int(groups)
    if not 1 <= groups <= MAX_GROUPS:
        raise _native.GnnppError('summarise: 1 <= groups <= %d (got %d)' % (MAX_GROUPS, groups))
    if group is None and groups != 1:
        raise _native.GnnppError('summarise: groups = %d needs `group`, the group id of every case' % groups)
    t_mp, t_ft, stride, valid, keep = _targets(targets, C, N)
    if group is not None:
        group = _per_case(group, C, 'group')
    ok = None
    if audit is not None:
        ok = _per_case(audit, C, 'audit') if torch.is_tensor(audit) else _per_case((audit.status == 0), C, 'audit.status')
    dev = _native.require_gpu(reached, stats, t_mp, t_ft, valid, group, ok)
    if hasattr(run, 'lived'):                                 # a stream: harvest, then only the cases that have ended
        run.reseat()
        ended = run.lived >= 0
        valid = ended if valid is None else valid & ended
    if valid is not None:
        valid = valid.to(torch.int32).contiguous()
    trace = getattr(run, 'trace', None)
    shielded = trace.shielded if trace is not None else None
    L = _native.lib()
    nbytes = L.gnnpp_rollout_summary_out_bytes(N, groups)
    out = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    n_i, n_f = groups * _native.SUMMARY_I64, groups * _native.SUMMARY_F64
    i64 = out[:n_i].view(groups, _native.SUMMARY_I64)
    f64 = out[n_i:n_i + n_f].view(torch.float64).view(groups, _native.SUMMARY_F64)
    hist = out[n_i + n_f:].view(torch.int32)[:groups * (N + 1)].view(groups, N + 1)
    s = _native.RolloutSummaryIn()
    s.reached, s.stats, s.target_makespan, s.target_flowtime = (reached.data_ptr(), stats.data_ptr(), t_mp.data_ptr(),
                                                                t_ft.data_ptr())
    for name, t in (('valid', valid), ('group', group), ('shielded', shielded), ('audit_ok', ok)):
        setattr(s, name, t.data_ptr() if t is not None else None)
    s.C, s.N, s.G, s.target_stride = C, N, groups, stride
    with _native.device_guard(dev):
        _native.check(L.gnnpp_rollout_summary(ctypes.byref(s), out.data_ptr(), _native.stream_ptr(dev)),
                      'gnnpp_rollout_summary')
    return Summary(i64, f64, hist, keep=(run, out, valid, group, shielded, ok) + keep)
