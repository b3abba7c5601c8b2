"""Shared by the CPU emulation test and the GPU test of gnnpp_rollout_summary (include/gnnpp_rollout_summary.h): the table of
shapes, deterministic inputs for each of its entries, a float64 numpy restatement of the record, and the comparison.

The table: C = 1, 2, 255, 256, 257, 600 (below, at and beyond one round of 256 cases, and a last round that is part full)
x N = 1, 3 x G = 1, 3; each entry in four variants: `valid` given or NULL x one degenerate case or all cases degenerate.
With G = 3 the groups are uneven, group 1 is empty and case C // 2 carries an id outside 0 .. G - 1.  The variants with
`valid` given also pass `shielded` and `audit_ok` and read the targets as the two columns of one [C,2] table (stride 2);
the others pass neither table (the record says -1) and read two target arrays (stride 1).

Tolerance of the doubles.  The kernel and numpy differ in the order of summation only (strided partials, a butterfly and
four waves against numpy's pairwise sum).  The largest relative difference measured over this table is MEASURED_REL; the
tests' bound is 16 x that."""
import ctypes

import numpy as np

SHAPES = [(C, N, G) for C in (1, 2, 255, 256, 257, 600) for N in (1, 3) for G in (1, 3)]
# the histogram's other paths: a thread that owns two bins (N + 1 > 256), and bins counted in global memory (N + 1 > 4096)
HIST_SHAPES = [(5, 300, 1), (258, 300, 3), (3, 4096, 2)]
VARIANTS = [(with_valid, degenerate) for with_valid in (True, False) for degenerate in ('one', 'all')]
MEASURED_REL = 4.4e-16                # 4.38e-16: the largest seen over the table, on the emulation and on the MI355X alike
TOL = 16 * MEASURED_REL
assert TOL <= 1e-12

I64, F64 = 16, 8
(I_N, I_REACH_ALL, I_OPTIMAL, I_AGENTS, I_DEGENERATE, I_BAD_GROUP, I_MP_PRED, I_MP_TARGET, I_FT_PRED, I_FT_TARGET, I_MIN,
 I_MAX, I_FAIL_SHIELDED, I_COLLISION_FREE, I_SHIELDED) = range(15)
F_RATE_REACH, F_AVG_DMP, F_STD_DMP, F_AVG_DFT, F_STD_DFT, F_MEAN_REACHED, F_M2_DMP, F_M2_DFT = range(8)


def inputs(C, N, G, with_valid, degenerate, seed=0):
    """Deterministic tables of one entry: dict of int32 arrays (None = the pointer is NULL) plus C, N, G."""
    rng = np.random.RandomState(1000 * C + 100 * N + 10 * G + 2 * int(with_valid) + (degenerate == 'all') + 7919 * seed)
    i32 = np.int32
    reached = (rng.rand(C, N) < 0.8).astype(i32)
    makespan = rng.randint(3, 60, C)
    stats = np.stack([makespan, makespan * N - rng.randint(0, 3, C) * (N - 1)], 1).astype(i32)
    targets = np.stack([rng.randint(3, 50, C), rng.randint(3, 50 * N, C)], 1).astype(i32)
    if degenerate == 'all':
        targets[::2, 0] = -1                                 # (either cost, zero or negative)
        targets[1::2, 1] = 0
    else:
        targets[C - 1, 0] = 0
    out = {'C': C, 'N': N, 'G': G, 'reached': reached, 'stats': stats, 'valid': None, 'group': None, 'shielded': None,
           'audit_ok': None}
    if with_valid:
        out['valid'] = (rng.rand(C) < 0.85).astype(i32) * rng.randint(1, 4, C).astype(i32)
        out['shielded'] = (rng.rand(C, N) < 0.3).astype(i32) * rng.randint(1, 9, (C, N)).astype(i32)
        out['audit_ok'] = (rng.rand(C) < 0.6).astype(i32)
        out['targets'], out['target_stride'] = targets, 2
    else:
        out['targets'] = (np.ascontiguousarray(targets[:, 0]), np.ascontiguousarray(targets[:, 1]))
        out['target_stride'] = 1
    if G > 1:
        group = np.where(rng.rand(C) < 0.7, 0, G - 1).astype(i32)            # uneven; the groups between stay empty
        group[C // 2] = G + 2 if C % 2 else -1                                # one id outside 0 .. G - 1
        out['group'] = group
    return out


def shard(x, lo, hi):
    """Cases lo .. hi - 1 of an entry as an entry of its own (contiguous copies)."""
    out = dict(x, C=hi - lo)
    for k in ('reached', 'stats', 'valid', 'group', 'shielded', 'audit_ok'):
        out[k] = None if x[k] is None else np.ascontiguousarray(x[k][lo:hi])
    t = x['targets']
    out['targets'] = np.ascontiguousarray(t[lo:hi]) if x['target_stride'] == 2 else tuple(
        np.ascontiguousarray(a[lo:hi]) for a in t)
    return out


def target_columns(x):
    t = x['targets']
    return (t[:, 0], t[:, 1]) if x['target_stride'] == 2 else t


def restate(x):
    """(i64 [G,16], f64 [G,8], hist [G,N+1]) of include/gnnpp_rollout_summary.h in numpy: int64 counts, float64 rates with
    np.mean and np.std(ddof=1) as the reference's summary() computes them."""
    C, N, G = x['C'], x['N'], x['G']
    tm, tf = (np.asarray(t, np.int64) for t in target_columns(x))
    mp, ft = x['stats'][:, 0].astype(np.int64), x['stats'][:, 1].astype(np.int64)
    valid = np.ones(C, bool) if x['valid'] is None else x['valid'] != 0
    group = np.zeros(C, np.int64) if x['group'] is None else x['group'].astype(np.int64)
    bad = valid & ((group < 0) | (group >= G))
    r = x['reached'] > 0
    k = r.sum(1)
    i64, f64, hist = np.zeros((G, I64), np.int64), np.zeros((G, F64), np.float64), np.zeros((G, N + 1), np.int32)
    for g in range(G):
        sel = valid & (group == g)
        n = int(sel.sum())
        all_ = sel & (k == N)
        degenerate = sel & ((tm <= 0) | (tf <= 0))
        rated = sel & ~degenerate
        row = i64[g]
        row[I_N], row[I_REACH_ALL], row[I_AGENTS] = n, all_.sum(), k[sel].sum()
        row[I_OPTIMAL] = (all_ & (mp <= tm) & (ft <= tf)).sum()
        row[I_DEGENERATE] = degenerate.sum()
        row[I_BAD_GROUP] = bad.sum() if g == 0 else 0
        row[I_MP_PRED], row[I_MP_TARGET] = mp[rated].sum(), tm[rated].sum()
        row[I_FT_PRED], row[I_FT_TARGET] = ft[rated].sum(), tf[rated].sum()
        row[I_MIN], row[I_MAX] = (k[sel].min(), k[sel].max()) if n else (-1, -1)
        if x['shielded'] is None:
            row[I_FAIL_SHIELDED] = row[I_SHIELDED] = -1
        else:
            s = x['shielded'] > 0
            row[I_FAIL_SHIELDED] = (sel & (k < N) & (s & ~r).any(1)).sum()
            row[I_SHIELDED] = (sel & s.any(1)).sum()
        row[I_COLLISION_FREE] = -1 if x['audit_ok'] is None else (sel & (x['audit_ok'] != 0)).sum()
        hist[g] = np.bincount(k[sel], minlength=N + 1)
        nan = float('nan')
        d_mp = np.abs(mp[rated] - tm[rated]).astype(np.float64) / tm[rated].astype(np.float64)
        d_ft = np.abs(ft[rated] - tf[rated]).astype(np.float64) / tf[rated].astype(np.float64)
        m = int(rated.sum())
        out = f64[g]
        out[F_RATE_REACH] = row[I_REACH_ALL] / n if n else nan
        out[F_MEAN_REACHED] = row[I_AGENTS] / n if n else nan
        for d, avg, std, m2 in ((d_mp, F_AVG_DMP, F_STD_DMP, F_M2_DMP), (d_ft, F_AVG_DFT, F_STD_DFT, F_M2_DFT)):
            out[avg] = np.mean(d) if m else nan
            out[std] = np.std(d, ddof=1) if m > 1 else nan
            out[m2] = np.sum((d - np.mean(d)) ** 2) if m else 0.0
    return i64, f64, hist


def rel_diff(got, want):
    """Largest relative difference of two float64 arrays; NaN must meet NaN and 0 must meet 0 (else inf)."""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    worst = 0.0
    for a, b in zip(got, want):
        if np.isnan(a) or np.isnan(b):
            d = 0.0 if np.isnan(a) and np.isnan(b) else float('inf')
        elif b == 0.0:
            d = 0.0 if a == 0.0 else float('inf')
        else:
            d = abs(a - b) / abs(b)
        worst = max(worst, d)
    return worst


def check(got, want, what):
    """Integers and hist exact, doubles within TOL; -> the largest relative difference of the doubles."""
    assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
    assert np.array_equal(got[2], want[2]), (what, got[2], want[2])
    d = rel_diff(got[1], want[1])
    assert d <= TOL, (what, d, got[1], want[1])
    return d


def out_views(buf, N, G):
    """The three arrays of a record held in a byte buffer (a numpy uint8 array, 8-byte aligned)."""
    a, b = G * I64 * 8, G * (I64 + F64) * 8
    return (buf[:a].view(np.int64).reshape(G, I64), buf[a:b].view(np.float64).reshape(G, F64),
            buf[b:b + G * (N + 1) * 4].view(np.int32).reshape(G, N + 1))


def fill_struct(s, x, ptr):
    """struct gnnpp_rollout_summary_in over the tables of `x`; ptr(array) -> its address."""
    tm, tf = target_columns(x)
    s.reached, s.stats = ptr(x['reached']), ptr(x['stats'])
    s.target_makespan = ptr(tm) if x['target_stride'] == 1 else ptr(x['targets'])
    s.target_flowtime = ptr(tf) if x['target_stride'] == 1 else ptr(x['targets']) + 4
    for k in ('valid', 'group', 'shielded', 'audit_ok'):
        setattr(s, k, ptr(x[k]) if x[k] is not None else None)
    s.C, s.N, s.G, s.target_stride = x['C'], x['N'], x['G'], x['target_stride']
    return s


def run_host(lib, x, poison=0x5a):
    """The call on numpy arrays (the emulated library); the buffer is poisoned first and carries 16 guard bytes."""
    from gnn_pathplanning_amd._native import RolloutSummaryIn
    N, G = x['N'], x['G']
    nbytes = lib.gnnpp_rollout_summary_out_bytes(N, G)
    assert nbytes == G * (I64 + F64) * 8 + G * (N + 1) * 4
    raw = np.full(nbytes + 24, poison, np.uint8)
    off = (-raw.ctypes.data) % 8
    buf = raw[off:off + nbytes + 16]
    s = fill_struct(RolloutSummaryIn(), x, lambda a: a.ctypes.data)
    assert lib.gnnpp_rollout_summary(ctypes.byref(s), buf.ctypes.data, None) == 0
    assert (buf[nbytes:] == poison).all(), 'a write behind the record'
    return tuple(v.copy() for v in out_views(buf[:nbytes], N, G))
