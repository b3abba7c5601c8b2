// The communication graphs of gnnpp_schedule_team_samples as CAPPED neighbour lists (include/gnnpp.h: cnt [graphs][N] |
// idx [graphs][N][cap] | val [graphs][N][cap], graphs = T_total), and the draw that expands chosen graphs into the
// standard block the team filter takes.  The graph of a step is symmetric bit for bit -- the weight is
// (float)(inv[i] * inv[j]) in fp64 -- so column n is row n and one set of lists serves both directions.
//
//   expert_team_step_deg_kernel   one workgroup per step, thread = agent: the largest degree of the step under the
//                                 case's final radius, recovered from the workspace's s = sqrt(1 / deg) -> step_deg
//                                 [T_total] (0 for a flagged case): what the caller sizes `cap` with
//   expert_team_lists_kernel      grid = steps x column tiles of kListCols columns, thread = column: the positions and
//                                 s = sqrt(1 / deg) of the whole step go to LDS, the thread scans the rows in ascending
//                                 order (every lane reads the same cell: an LDS broadcast) and stores its entries four at
//                                 a time, the indices in one 8-byte and the weights in one 16-byte store, as
//                                 rollout_team_lists_kernel does.  cnt is the true degree; entries from `cap` on are
//                                 dropped, nothing is written outside the column.
//   team_lists_gather_kernel      thread = (column, group of four entries) of one drawn graph: cnt and the first
//                                 roundup4(cnt) entries of every column go from the capped set to the block of stride Np
//
// No atomics, one writer per element: two calls give the same bytes.  Included from gnnpp_api.hip after
// expert_team_kernels.hip and rollout_team_lists_kernel.hip and uses their helpers.

namespace gnnpp {

constexpr int kListCols = 64;                 // columns per workgroup of expert_team_lists_kernel: one wave

// Largest degree of step t with the case's radius, from what expert_team_degree_kernel left in the workspace instead of
// a second count over the positions: s = sqrt(1.0 / deg) with 1 <= deg < N <= 1024 (0.0 for deg = 0), both operations
// correctly rounded, so 1.0 / (s * s) lies within a few ulp of deg and rounds to it exactly.  LDS: max(N, 64) ints.
__global__ __launch_bounds__(1024) void expert_team_step_deg_kernel(const ScheduleArgs p, const double* inv_ws,
                                                                    int* step_deg) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int N = p.N, t = blockIdx.x, a = threadIdx.x;
    const int c = schedule_case_of(p.case_start, p.C, t);
    if (p.status[c] != 0) {                                      // (workgroup-uniform; its workspace rows are unwritten)
        if (a == 0) step_deg[t] = 0;
        return;
    }
    int* dg = reinterpret_cast<int*>(gnnpp_smem);
    if (a < N) {
        const double s = inv_ws[(size_t)t * N + a];
        dg[a] = s > 0.0 ? (int)(1.0 / (s * s) + 0.5) : 0;
    }
    __syncthreads();
    if (a < 64) {                                                // the first wave folds the N degrees to 64 ...
        int m = 0;
        for (int j = a; j < N; j += 64) m = max(m, dg[j]);
        dg[a] = m;                                               // (lane a read only the entries = a mod 64)
    }
    __syncthreads();
    if (a == 0) {                                                // ... and its first lane those
        int m = 0;
        for (int j = 0; j < 64; ++j) m = max(m, dg[j]);
        step_deg[t] = m;
    }
}

// Column n of the lists of step t of case c (lane = the thread's index in its workgroup of kListCols, which calls this
// as a whole) -> il / wl, the column's cap entries in the caller's arrays (il 8-byte, wl 16-byte aligned, cap % 4 == 0);
// returns cnt, the true degree (unspecified for n >= N, which stores nothing).  LDS: (row, col) [N] | s [N] (fp64).
__device__ __forceinline__ int schedule_team_list_column(const ScheduleArgs& p, int t, int c, int n, int lane,
                                                         const double* inv_g, unsigned short* il, float* wl, int cap,
                                                         char* smem) {
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    typedef int v2i __attribute__((ext_vector_type(2)));
    const int N = p.N;
    v2i* pl = reinterpret_cast<v2i*>(smem);                                         // [N]
    double* inv = reinterpret_cast<double*>(smem + round16((size_t)8 * N));         // [N]
    const int* pos = p.pos + (size_t)t * N * 2;
    for (int i = lane; i < N; i += kListCols) {
        v2i q; q[0] = pos[2 * i]; q[1] = pos[2 * i + 1];
        pl[i] = q;
        inv[i] = inv_g[i];
    }
    __syncthreads();
    if (n >= N) return 0;
    const unsigned Tu = dist2_bound(p.radius[c]);
    const v2i me = pl[n];
    const double sn = inv[n];
    int cnt = 0;
    unsigned long long pk = 0ull;                                // the last four entries, the newest on top ...
    v4f w = {0.f, 0.f, 0.f, 0.f};                                // ... and their weights, the newest in w[3]
#pragma unroll 4
    for (int i = 0; i < N; ++i) {
        const v2i q = pl[i];
        if (i != n && dist2(q[0], q[1], me[0], me[1]) <= Tu) {
            pk = (pk >> 16) | ((unsigned long long)i << 48);
            const v4f s = {w[1], w[2], w[3], (float)(inv[i] * sn)};
            w = s;
            ++cnt;
            if ((cnt & 3) == 0 && cnt <= cap) {
                v2u o; o[0] = (unsigned)pk; o[1] = (unsigned)(pk >> 32);
                *reinterpret_cast<v2u*>(il + cnt - 4) = o;
                *reinterpret_cast<v4f*>(wl + cnt - 4) = w;
            }
        }
    }
    const int r = cnt & 3;
    if (r && (cnt & ~3) < cap) {                                 // the tail and, behind it, the zeros of the padding
        pk >>= 16 * (4 - r);
        v2u o; o[0] = (unsigned)pk; o[1] = (unsigned)(pk >> 32);
        *reinterpret_cast<v2u*>(il + (cnt & ~3)) = o;
        const v4f z = {r == 1 ? w[3] : r == 2 ? w[2] : w[1], r == 1 ? 0.f : r == 2 ? w[3] : w[2], r == 3 ? w[3] : 0.f, 0.f};
        *reinterpret_cast<v4f*>(wl + (cnt & ~3)) = z;
    }
    return cnt;
}

// Columns [tile * kListCols, ...) of step t.
__global__ __launch_bounds__(kListCols) void expert_team_lists_kernel(const ScheduleArgs p, const double* inv_ws, int tiles,
                                                                      int* cnt_out, unsigned short* idx_out,
                                                                      float* val_out, int cap) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int N = p.N, lane = threadIdx.x;
    const int t = blockIdx.x / tiles, n = (blockIdx.x - t * tiles) * kListCols + lane;
    const int c = schedule_case_of(p.case_start, p.C, t);
    if (p.status[c] != 0) return;                                // (workgroup-uniform)
    const size_t col = (size_t)t * N + n;
    const int cnt = schedule_team_list_column(p, t, c, n, lane, inv_ws + (size_t)t * N, idx_out + col * cap,
                                              val_out + col * cap, cap, gnnpp_smem);
    if (n < N) cnt_out[col] = cnt;
}

struct TeamGatherArgs {
    const int* cnt; const unsigned short* idx; const float* val;      // the capped set
    const int* index;                                                  // [B] graph of the set for graph b of the block
    int* cnt_o; unsigned short* idx_o; float* val_o;                   // the regions of the standard block
    int graphs_src, cap, N, Np, per_graph;                             // per_graph: workgroups per drawn graph
};

// item = (column, group of four entries) of drawn graph b, column-major: consecutive threads read consecutive groups of
// the set.  An index outside [0, graphs_src) is CLAMPED into it.  Copies min(roundup4(cnt), cap) entries.
__global__ __launch_bounds__(256) void team_lists_gather_kernel(const TeamGatherArgs p) {
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    const int b = blockIdx.x / p.per_graph;
    const int quads = p.cap >> 2;
    const int item = (blockIdx.x - b * p.per_graph) * 256 + threadIdx.x;
    const int n = item / quads, d = 4 * (item - n * quads);
    if (n >= p.N) return;
    int g = p.index[b];
    g = g < 0 ? 0 : g >= p.graphs_src ? p.graphs_src - 1 : g;
    const size_t src = (size_t)g * p.N + n, dst = (size_t)b * p.N + n;
    const int cnt = p.cnt[src];
    if (d == 0) p.cnt_o[dst] = cnt;
    if (d >= cnt) return;                                        // (d < cap <= Np: inside both columns)
    *reinterpret_cast<v2u*>(p.idx_o + dst * p.Np + d) = *reinterpret_cast<const v2u*>(p.idx + src * p.cap + d);
    *reinterpret_cast<v4f*>(p.val_o + dst * p.Np + d) = *reinterpret_cast<const v4f*>(p.val + src * p.cap + d);
}

// scan, case and degree of schedule_team_samples_launch, then the steps' largest degrees
int schedule_team_plan_launch(const ScheduleArgs& a, double* inv_ws, int* step_deg, hipStream_t st) {
    if (!schedule_team_fits(a)) return GNNPP_ERR_UNSUPPORTED;
    const int nt = team_threads(a.N);
    hipLaunchKernelGGL(expert_team_scan_kernel, dim3(a.T_total), dim3(nt), expert_team_scan_smem(a.N), st, a);
    hipLaunchKernelGGL(expert_case_kernel, dim3(a.C), dim3(64), 0, st, a);
    hipLaunchKernelGGL(expert_team_degree_kernel, dim3(a.T_total), dim3(nt), (size_t)8 * a.N, st, a, inv_ws);
    hipLaunchKernelGGL(expert_team_step_deg_kernel, dim3(a.T_total), dim3(nt),
                       (size_t)4 * (a.N > 64 ? a.N : 64), st, a, static_cast<const double*>(inv_ws), step_deg);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

int schedule_team_fill_lists_launch(const ScheduleArgs& a, const double* inv_ws, int* cnt, unsigned short* idx,
                                    float* val, int cap, hipStream_t st) {
    if (!schedule_team_fits(a)) return GNNPP_ERR_UNSUPPORTED;
    const int tiles = (a.N + kListCols - 1) / kListCols;
    const int groups = (a.N + kObsAgentsPerWg - 1) / kObsAgentsPerWg;
    hipLaunchKernelGGL(expert_team_lists_kernel, dim3(a.T_total * tiles), dim3(kListCols),
                       round16((size_t)8 * a.N) + (size_t)8 * a.N, st, a, inv_ws, tiles, cnt, idx, val, cap);
    schedule_team_observe_launch(a, groups, st);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

// `lists`: a block of team_lists_bytes(B, N) bytes, 16-byte aligned (validated by the caller, like cap and the set)
int team_lists_gather_launch(const int* cnt, const unsigned short* idx, const float* val, int graphs_src, int cap,
                             const int* index, int B, void* lists, int N, hipStream_t st) {
    const TeamLayout L = team_layout(B, N, 1, 2, 1, 1);
    char* base = static_cast<char*>(lists);
    TeamGatherArgs a;
    a.cnt = cnt; a.idx = idx; a.val = val; a.index = index;
    a.cnt_o = reinterpret_cast<int*>(base + L.cnt);
    a.idx_o = reinterpret_cast<unsigned short*>(base + L.idx);
    a.val_o = reinterpret_cast<float*>(base + L.val);
    a.graphs_src = graphs_src; a.cap = cap; a.N = N; a.Np = L.Np;
    a.per_graph = (N * (cap >> 2) + 255) / 256;
    if ((long long)B * a.per_graph > 0x7fffffffLL) return GNNPP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(team_lists_gather_kernel, dim3(B * a.per_graph), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

}  // namespace gnnpp
