// The summary of a rollout's per-case result tables (include/gnnpp_rollout_summary.h): the reference's
// validation / test metrics, one launch, one workgroup of 256 threads per group, no atomics, nothing read on the host, one
// writer per word, capturable.
//
// rollout_summary_kernel, workgroup g = group g:
//   pass 1  rounds of 256 cases: thread tid looks at case round * 256 + tid.  A case that takes part (valid, of this
//           group) is counted into the thread's integer partials and, unless degenerate, its two rates are added to the
//           thread's double partials.  The case's number of agents that reached goes to LDS; behind a barrier the owner
//           of a histogram bin (bin k: thread k % 256) scans the round's 256 words in order and counts its bins, which
//           it alone reads and writes: in LDS while N + 1 <= kSummaryLdsBins (copied to hist at the end), else in hist
//           itself -- the same code on another pointer.  A thread that owns no bin (tid > N) skips the scan.
//   reduce  every partial over the wave (xor butterfly: every lane ends with the same bits), the four waves' results
//           through LDS, added in wave order by every thread: all of them hold n, n_degenerate and the two means.
//   pass 2  the same cases in the same order: squared differences from the means, reduced the same way.
//   thread 0 writes the record.
// A 64-bit word crosses lanes as two 32-bit halves, moved as float BITS by __shfl_xor (a move, not a conversion).
// Included from gnnpp_api.hip; needs nothing of the other kernel files.
#include "../../include/gnnpp_rollout_summary.h"

namespace gnnpp {

constexpr int kSummaryThreads = 256, kSummaryWaves = kSummaryThreads / 64;
// integer partials of a thread, in this order (the first 13 are sums)
enum {
    kSumN, kSumReachAll, kSumOptimal, kSumAgents, kSumDegenerate, kSumBadGroup, kSumMpPred, kSumMpTarget, kSumFtPred,
    kSumFtTarget, kSumFailShielded, kSumCollisionFree, kSumShielded, kSummarySums, kSumMin = kSummarySums, kSumMax,
    kSummaryInts
};
// histograms of up to this many bins are counted in LDS (a read-modify-write per hit: in global memory that chain of
// round trips was 90 % of the launch at C = 4500, N = 10)
constexpr int kSummaryLdsBins = 4096;
// LDS: the round's reach counts, then one slot per (wave, integer partial), then one per (wave, double partial), then the
// histogram's bins when they fit
__host__ __device__ inline size_t summary_smem(int N) {
    return kSummaryThreads * sizeof(int) + (size_t)kSummaryWaves * (kSummaryInts + 2) * 8 +
           (N + 1 <= kSummaryLdsBins ? ((size_t)N + 1) * sizeof(int) : 0);
}
struct alignas(16) SummaryInt4 { int x, y, z, w; };

struct SummaryArgs {
    const int* reached; const int* stats; const int* target_mp; const int* target_ft; const int* valid; const int* group;
    const int* shielded; const int* audit_ok;
    long long* out_i64; double* out_f64; int* hist;
    int C, N, G, target_stride;
};

__device__ __forceinline__ unsigned long long summary_shfl_xor(unsigned long long v, int m) {
    const int lo = __float_as_int(__shfl_xor(__int_as_float((int)(unsigned)(v & 0xffffffffull)), m));
    const int hi = __float_as_int(__shfl_xor(__int_as_float((int)(unsigned)(v >> 32)), m));
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
}
__device__ __forceinline__ long long summary_shfl_xor(long long v, int m) {
    return (long long)summary_shfl_xor((unsigned long long)v, m);
}
__device__ __forceinline__ double summary_shfl_xor(double v, int m) {
    return __builtin_bit_cast(double, summary_shfl_xor(__builtin_bit_cast(unsigned long long, v), m));
}

// Does case c take part in group g?  -> 1: yes; 0: no; -1: a valid case with a group id outside 0 .. G - 1
__device__ __forceinline__ int summary_member(const SummaryArgs& p, long long c, int g) {
    if (c >= p.C || (p.valid && p.valid[c] == 0)) return 0;
    const int gc = p.group ? p.group[c] : 0;
    if (gc < 0 || gc >= p.G) return -1;
    return gc == g;
}

__global__ __launch_bounds__(256) void rollout_summary_kernel(const SummaryArgs p) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    int* round_k = reinterpret_cast<int*>(gnnpp_smem);                                 // [256]
    long long* wave_i = reinterpret_cast<long long*>(gnnpp_smem + kSummaryThreads * sizeof(int));   // [4][kSummaryInts]
    double* wave_d = reinterpret_cast<double*>(wave_i + kSummaryWaves * kSummaryInts);  // [4][2]
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = p.N;
    int* hist = p.hist + (size_t)g * (N + 1);
    const bool lds_bins = N + 1 <= kSummaryLdsBins;
    int* bins = lds_bins ? reinterpret_cast<int*>(wave_d + 2 * kSummaryWaves) : hist;  // [N + 1]
    for (int k = tid; k <= N; k += kSummaryThreads) bins[k] = 0;                       // (its owner: the only writer)

    long long acc[kSummaryInts];
#pragma unroll
    for (int i = 0; i < kSummarySums; ++i) acc[i] = 0;
    acc[kSumMin] = (long long)N + 1;
    acc[kSumMax] = -1;
    double sum_mp = 0.0, sum_ft = 0.0;

    // ---- pass 1
    for (long long base = 0; base < p.C; base += kSummaryThreads) {
        const long long c = base + tid;
        const int member = summary_member(p, c, g);
        int k = -1;                                          // agents that reached, of a case that takes part
        if (member < 0 && g == 0) acc[kSumBadGroup] += 1;
        if (member > 0) {
            const int* reached = p.reached + (size_t)c * N;
            const int* shielded = p.shielded ? p.shielded + (size_t)c * N : nullptr;
            int any_shielded = 0, late_shielded = 0;
            k = 0;
            for (int a = 0; a < N; ++a) {
                const int r = reached[a] > 0;
                k += r;
                if (shielded) {
                    const int s = shielded[a] > 0;
                    any_shielded |= s;
                    late_shielded |= s & (r ^ 1);
                }
            }
            const int all = k == N;
            const long long mp = p.stats[2 * c], ft = p.stats[2 * c + 1];
            const long long tm = p.target_mp[(size_t)c * p.target_stride], tf = p.target_ft[(size_t)c * p.target_stride];
            acc[kSumN] += 1;
            acc[kSumReachAll] += all;
            acc[kSumOptimal] += all && mp <= tm && ft <= tf;
            acc[kSumAgents] += k;
            acc[kSumMin] = k < acc[kSumMin] ? k : acc[kSumMin];
            acc[kSumMax] = k > acc[kSumMax] ? k : acc[kSumMax];
            acc[kSumFailShielded] += !all && late_shielded;
            acc[kSumShielded] += any_shielded;
            if (p.audit_ok) acc[kSumCollisionFree] += p.audit_ok[c] != 0;
            if (tm <= 0 || tf <= 0) {
                acc[kSumDegenerate] += 1;
            } else {
                acc[kSumMpPred] += mp; acc[kSumMpTarget] += tm; acc[kSumFtPred] += ft; acc[kSumFtTarget] += tf;
                sum_mp += fabs((double)mp - (double)tm) / (double)tm;
                sum_ft += fabs((double)ft - (double)tf) / (double)tf;
            }
        }
        round_k[tid] = k;
        __syncthreads();
        if (tid <= N) {                                      // (LDS broadcast reads; the owner of bin k counts it)
            const SummaryInt4* round_k4 = reinterpret_cast<const SummaryInt4*>(round_k);
#pragma unroll 4
            for (int j = 0; j < kSummaryThreads / 4; ++j) {
                const SummaryInt4 v = round_k4[j];
                if (v.x >= 0 && (v.x & (kSummaryThreads - 1)) == tid) bins[v.x] += 1;
                if (v.y >= 0 && (v.y & (kSummaryThreads - 1)) == tid) bins[v.y] += 1;
                if (v.z >= 0 && (v.z & (kSummaryThreads - 1)) == tid) bins[v.z] += 1;
                if (v.w >= 0 && (v.w & (kSummaryThreads - 1)) == tid) bins[v.w] += 1;
            }
        }
        __syncthreads();                                     // the next round overwrites round_k
    }

    // ---- reduce: wave butterfly, then the four waves in order
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int i = 0; i < kSummarySums; ++i) acc[i] += summary_shfl_xor(acc[i], m);
        const long long lo = summary_shfl_xor(acc[kSumMin], m), hi = summary_shfl_xor(acc[kSumMax], m);
        acc[kSumMin] = lo < acc[kSumMin] ? lo : acc[kSumMin];
        acc[kSumMax] = hi > acc[kSumMax] ? hi : acc[kSumMax];
        sum_mp += summary_shfl_xor(sum_mp, m);
        sum_ft += summary_shfl_xor(sum_ft, m);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kSummaryInts; ++i) wave_i[wave * kSummaryInts + i] = acc[i];
        wave_d[2 * wave] = sum_mp;
        wave_d[2 * wave + 1] = sum_ft;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kSummaryInts; ++i) acc[i] = wave_i[i];
    sum_mp = wave_d[0];
    sum_ft = wave_d[1];
    for (int w = 1; w < kSummaryWaves; ++w) {
#pragma unroll
        for (int i = 0; i < kSummarySums; ++i) acc[i] += wave_i[w * kSummaryInts + i];
        const long long lo = wave_i[w * kSummaryInts + kSumMin], hi = wave_i[w * kSummaryInts + kSumMax];
        acc[kSumMin] = lo < acc[kSumMin] ? lo : acc[kSumMin];
        acc[kSumMax] = hi > acc[kSumMax] ? hi : acc[kSumMax];
        sum_mp += wave_d[2 * w];
        sum_ft += wave_d[2 * w + 1];
    }
    if (lds_bins)
        for (int k = tid; k <= N; k += kSummaryThreads) hist[k] = bins[k];
    const long long n = acc[kSumN], m_rates = n - acc[kSumDegenerate];
    const double nan = __builtin_nan("");
    const double avg_mp = m_rates > 0 ? sum_mp / (double)m_rates : nan;
    const double avg_ft = m_rates > 0 ? sum_ft / (double)m_rates : nan;
    __syncthreads();                                         // every thread has read the slots pass 2 writes again

    // ---- pass 2: squared differences from the means, the same cases in the same order
    double m2_mp = 0.0, m2_ft = 0.0;
    if (m_rates > 0) {                                       // (workgroup-uniform)
        for (long long c = tid; c < p.C; c += kSummaryThreads) {
            if (summary_member(p, c, g) <= 0) continue;
            const long long tm = p.target_mp[(size_t)c * p.target_stride], tf = p.target_ft[(size_t)c * p.target_stride];
            if (tm <= 0 || tf <= 0) continue;
            const double d_mp = fabs((double)p.stats[2 * c] - (double)tm) / (double)tm - avg_mp;
            const double d_ft = fabs((double)p.stats[2 * c + 1] - (double)tf) / (double)tf - avg_ft;
            m2_mp += d_mp * d_mp;
            m2_ft += d_ft * d_ft;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        m2_mp += summary_shfl_xor(m2_mp, m);
        m2_ft += summary_shfl_xor(m2_ft, m);
    }
    if (lane == 0) {
        wave_d[2 * wave] = m2_mp;
        wave_d[2 * wave + 1] = m2_ft;
    }
    __syncthreads();
    if (tid != 0) return;
    m2_mp = wave_d[0];
    m2_ft = wave_d[1];
    for (int w = 1; w < kSummaryWaves; ++w) {
        m2_mp += wave_d[2 * w];
        m2_ft += wave_d[2 * w + 1];
    }

    long long* oi = p.out_i64 + (size_t)g * GNNPP_SUMMARY_I64;
    double* od = p.out_f64 + (size_t)g * GNNPP_SUMMARY_F64;
    oi[GNNPP_SUMMARY_N] = n;
    oi[GNNPP_SUMMARY_N_REACH_ALL] = acc[kSumReachAll];
    oi[GNNPP_SUMMARY_N_OPTIMAL] = acc[kSumOptimal];
    oi[GNNPP_SUMMARY_AGENTS_REACHED] = acc[kSumAgents];
    oi[GNNPP_SUMMARY_N_DEGENERATE] = acc[kSumDegenerate];
    oi[GNNPP_SUMMARY_N_BAD_GROUP] = acc[kSumBadGroup];
    oi[GNNPP_SUMMARY_SUM_MP_PRED] = acc[kSumMpPred];
    oi[GNNPP_SUMMARY_SUM_MP_TARGET] = acc[kSumMpTarget];
    oi[GNNPP_SUMMARY_SUM_FT_PRED] = acc[kSumFtPred];
    oi[GNNPP_SUMMARY_SUM_FT_TARGET] = acc[kSumFtTarget];
    oi[GNNPP_SUMMARY_MIN_REACHED] = n > 0 ? acc[kSumMin] : -1;
    oi[GNNPP_SUMMARY_MAX_REACHED] = n > 0 ? acc[kSumMax] : -1;
    oi[GNNPP_SUMMARY_N_FAIL_SHIELDED] = p.shielded ? acc[kSumFailShielded] : -1;
    oi[GNNPP_SUMMARY_N_COLLISION_FREE] = p.audit_ok ? acc[kSumCollisionFree] : -1;
    oi[GNNPP_SUMMARY_N_SHIELDED] = p.shielded ? acc[kSumShielded] : -1;
    oi[15] = 0;
    od[GNNPP_SUMMARY_RATE_REACH] = n > 0 ? (double)acc[kSumReachAll] / (double)n : nan;
    od[GNNPP_SUMMARY_AVG_DMP] = avg_mp;
    od[GNNPP_SUMMARY_STD_DMP] = m_rates > 1 ? sqrt(m2_mp / (double)(m_rates - 1)) : nan;
    od[GNNPP_SUMMARY_AVG_DFT] = avg_ft;
    od[GNNPP_SUMMARY_STD_DFT] = m_rates > 1 ? sqrt(m2_ft / (double)(m_rates - 1)) : nan;
    od[GNNPP_SUMMARY_MEAN_REACHED] = n > 0 ? (double)acc[kSumAgents] / (double)n : nan;
    od[GNNPP_SUMMARY_M2_DMP] = m2_mp;
    od[GNNPP_SUMMARY_M2_DFT] = m2_ft;
}

inline size_t summary_out_bytes(int N, int G) {
    return (size_t)G * (GNNPP_SUMMARY_I64 + GNNPP_SUMMARY_F64) * 8 + (size_t)G * ((size_t)N + 1) * sizeof(int);
}

// GNNPP_OK or GNNPP_ERR_LAUNCH (arguments checked by the entry point)
int rollout_summary_launch(const gnnpp_rollout_summary_in& in, void* out, hipStream_t st) {
    SummaryArgs p;
    p.reached = in.reached; p.stats = in.stats; p.target_mp = in.target_makespan; p.target_ft = in.target_flowtime;
    p.valid = in.valid; p.group = in.group; p.shielded = in.shielded; p.audit_ok = in.audit_ok;
    char* base = static_cast<char*>(out);
    p.out_i64 = reinterpret_cast<long long*>(base);
    p.out_f64 = reinterpret_cast<double*>(base + (size_t)in.G * GNNPP_SUMMARY_I64 * 8);
    p.hist = reinterpret_cast<int*>(base + (size_t)in.G * (GNNPP_SUMMARY_I64 + GNNPP_SUMMARY_F64) * 8);
    p.C = in.C; p.N = in.N; p.G = in.G; p.target_stride = in.target_stride;
    hipLaunchKernelGGL(rollout_summary_kernel, dim3(in.G), dim3(kSummaryThreads), summary_smem(in.N), st, p);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

static_assert(GNNPP_SUMMARY_N_SHIELDED < GNNPP_SUMMARY_I64 - 1 && GNNPP_SUMMARY_M2_DFT == GNNPP_SUMMARY_F64 - 1, "record");

}  // namespace gnnpp
