// A training batch straight from expert schedules (include/gnnpp_schedule_draw.h): B picked steps of a schedule set
// become the observations, one-hot targets and graphs that gnnpp_schedule_team_samples (dense S) or
// gnnpp_schedule_team_fill_lists + gnnpp_team_lists_gather (a standard lists block) would have produced for those steps,
// byte for byte, without the tensors of any other step ever existing.  radius[c] and status[c] are INPUTS here: the
// plan call (gnnpp_schedule_team_plan) left them when the cases were appended.
//
// The device functions are those of the sample calls -- schedule_team_degree_step / schedule_team_graph_tile /
// schedule_team_observe_group (expert_team_kernels.hip) and schedule_team_list_column (expert_team_lists_kernel.hip) --
// called with "row b of the batch" where the sample kernels say "row t of the set".  The only new data movement is
// pick -> step -> case: t = index[b] clamped into [0, T_total), c by the binary search of case_start every schedule
// kernel uses (log2 C reads of a cached array per workgroup; a per-step table would cost 4 more bytes per stored step).
// One route for every team size 2 .. GNNPP_ROLLOUT_MAX_TEAM.  Three launches on one stream:
//
//   schedule_draw_degree_kernel    one workgroup per pick, thread = agent: s = sqrt(1.0 / deg) in fp64 under the case's
//                                  radius -> workspace [B, N]; the agent's one-hot target
//   schedule_draw_graph_kernel     grid = row tiles x picks: kTeamGraphRows rows of S[b], 16-byte stores when N % 4 == 0
//     or schedule_draw_lists_kernel  and S is 16-byte aligned;  grid = column tiles x picks, thread = column: cnt and the
//                                  first roundup4(cnt) entries of the column at the block's stride
//   schedule_draw_observe_kernel   grid = 16-agent groups x picks: the case's occupancy grid in LDS, the group's rows
//
// A pick whose case is flagged (status != 0) writes zeros: target, S or cnt, obs.  No atomics, one writer per element,
// no hand-off between workgroups of a launch.  Included from gnnpp_api.hip after expert_team_lists_kernel.hip.
#include "../../include/gnnpp_schedule_draw.h"

namespace gnnpp {

// the step of pick b: an index outside [0, T_total) is clamped into it, as team_lists_gather_kernel does
__device__ __forceinline__ int schedule_draw_step(const ScheduleArgs& p, const int* index, int b) {
    const int t = index[b];
    return t < 0 ? 0 : t >= p.T_total ? p.T_total - 1 : t;
}

// p.target: the batch's [B,N,5].  LDS: px | py [N].
__global__ __launch_bounds__(1024) void schedule_draw_degree_kernel(const ScheduleArgs p, const int* index,
                                                                    double* inv_ws) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int N = p.N, b = blockIdx.x, a = threadIdx.x;
    const int t = schedule_draw_step(p, index, b);
    const int c = schedule_case_of(p.case_start, p.C, t);
    float* tgt = p.target + (size_t)b * N * 5;
    if (p.status[c] != 0) {                                      // (workgroup-uniform; the workspace row stays unread)
        if (a < N) {
#pragma unroll
            for (int j = 0; j < 5; ++j) tgt[(size_t)a * 5 + j] = 0.f;
        }
        return;
    }
    int* px = reinterpret_cast<int*>(gnnpp_smem);
    schedule_team_degree_step(p, t, c, a, px, px + N, inv_ws + (size_t)b * N, tgt);
}

// p.S: the batch's [B,N,N].  LDS as expert_team_graph_kernel.
__global__ __launch_bounds__(256) void schedule_draw_graph_kernel(const ScheduleArgs p, const int* index,
                                                                  const double* inv_ws, int tiles, int vec) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int N = p.N;
    const int b = blockIdx.x / tiles, i0 = (blockIdx.x - b * tiles) * kTeamGraphRows;
    const int t = schedule_draw_step(p, index, b);
    const int c = schedule_case_of(p.case_start, p.C, t);
    float* S = p.S + ((size_t)b * N + i0) * N;
    if (p.status[c] != 0) {                                      // (workgroup-uniform) the tile's rows are contiguous
        const int cells = (min(N, i0 + kTeamGraphRows) - i0) * N;
        for (int i = threadIdx.x; i < cells; i += 256) S[i] = 0.f;
        return;
    }
    schedule_team_graph_tile(p, t, c, i0, inv_ws + (size_t)b * N, S, nullptr, vec, gnnpp_smem);
}

// cnt_o / idx_o / val_o: the regions of the batch's standard block of stride Np = roundup4(N).  A column never holds more
// than N - 1 < Np entries, so schedule_team_list_column at cap = Np stores exactly cnt and the first roundup4(cnt)
// entries: what the gather copies out of a capped set.  LDS as expert_team_lists_kernel.
__global__ __launch_bounds__(kListCols) void schedule_draw_lists_kernel(const ScheduleArgs p, const int* index,
                                                                        const double* inv_ws, int tiles, int* cnt_o,
                                                                        unsigned short* idx_o, float* val_o, int Np) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int N = p.N, lane = threadIdx.x;
    const int b = blockIdx.x / tiles, n = (blockIdx.x - b * tiles) * kListCols + lane;
    const int t = schedule_draw_step(p, index, b);
    const int c = schedule_case_of(p.case_start, p.C, t);
    const size_t col = (size_t)b * N + n;
    if (p.status[c] != 0) {                                      // (workgroup-uniform)
        if (n < N) cnt_o[col] = 0;
        return;
    }
    const int cnt = schedule_team_list_column(p, t, c, n, lane, inv_ws + (size_t)b * N, idx_o + col * Np, val_o + col * Np,
                                              Np, gnnpp_smem);
    if (n < N) cnt_o[col] = cnt;
}

// p.obs: the batch's [B,N,3,11,11].  LDS as expert_team_observe_kernel.
__global__ __launch_bounds__(256) void schedule_draw_observe_kernel(const ScheduleArgs p, const int* index, int groups) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int b = blockIdx.x / groups, n0 = (blockIdx.x - b * groups) * kObsAgentsPerWg;
    const int t = schedule_draw_step(p, index, b);
    const int c = schedule_case_of(p.case_start, p.C, t);
    if (p.status[c] != 0) {                                      // (workgroup-uniform; its states may be off the map)
        float* out = p.obs + ((size_t)b * p.N + n0) * 363;
        const int cells = (min(p.N, n0 + kObsAgentsPerWg) - n0) * 363;
        for (int i = threadIdx.x; i < cells; i += 256) out[i] = 0.f;
        return;
    }
    schedule_team_observe_group(p, t, c, b, n0, gnnpp_smem);
}

inline size_t schedule_draw_workspace_bytes(int N, int B) { return round16((size_t)B * N * sizeof(double)); }

// the map fits the LDS occupancy grid and every launch a grid dimension
inline bool schedule_draw_fits(int N, int H, int W, int B) {
    const int most = (N + kObsAgentsPerWg - 1) / kObsAgentsPerWg;           // (the launch with the most workgroups per pick)
    return (long long)H * W <= kTeamMaxCells && (long long)B * most <= 0x7fffffffLL;
}

// a: the schedule set with obs / target / S replaced by the batch's tensors (S NULL: the lists block is written).
// `lists`: a block of team_lists_bytes(B, a.N) bytes, 16-byte aligned (validated by the caller, like everything else).
int schedule_draw_launch(const ScheduleArgs& a, const int* index, int B, void* lists, double* inv_ws, hipStream_t st) {
    const int N = a.N, nt = team_threads(N);
    const int groups = (N + kObsAgentsPerWg - 1) / kObsAgentsPerWg;
    hipLaunchKernelGGL(schedule_draw_degree_kernel, dim3(B), dim3(nt), (size_t)8 * N, st, a, index, inv_ws);
    if (a.S) {
        const int tiles = (N + kTeamGraphRows - 1) / kTeamGraphRows;
        const int vec = (N & 3) == 0 && (reinterpret_cast<size_t>(a.S) & 15) == 0;
        hipLaunchKernelGGL(schedule_draw_graph_kernel, dim3(B * tiles), dim3(256), (size_t)16 * ((N + 3) & ~3), st, a, index,
                           static_cast<const double*>(inv_ws), tiles, vec);
    } else {
        const TeamLayout L = team_layout(B, N, 1, 2, 1, 1);
        char* base = static_cast<char*>(lists);
        const int tiles = (N + kListCols - 1) / kListCols;
        hipLaunchKernelGGL(schedule_draw_lists_kernel, dim3(B * tiles), dim3(kListCols),
                           round16((size_t)8 * N) + (size_t)8 * N, st, a, index, static_cast<const double*>(inv_ws), tiles,
                           reinterpret_cast<int*>(base + L.cnt), reinterpret_cast<unsigned short*>(base + L.idx),
                           reinterpret_cast<float*>(base + L.val), L.Np);
    }
    static LdsAttrOnce once;
    set_lds_attr_once(once, reinterpret_cast<const void*>(&schedule_draw_observe_kernel), kTeamLdsBytes);
    hipLaunchKernelGGL(schedule_draw_observe_kernel, dim3(B * groups), dim3(256), team_observe_smem(N, a.H, a.W), st, a,
                       index, groups);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

}  // namespace gnnpp
