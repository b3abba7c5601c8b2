// Training samples from expert schedules for teams of up to GNNPP_ROLLOUT_MAX_TEAM agents: the statement of
// expert_kernels.hip (targets, observations, the radius that grows until every step of a case is connected, the
// final radius rebuilding every step), the same bytes wherever both apply, in the layout of rollout_team_kernels.hip
// instead of one wave per step (two agents per lane, 128-bit agent masks).  Five launches on one stream, no atomics
// and no hand-off between workgroups of a launch (a case can have more steps than the chip holds workgroups), every
// output element has one writer:
//
//   expert_team_scan_kernel     one workgroup per step, thread = agent: legality of the step's states and moves, k_t
//                               by the level-synchronous search over N-bit frontier sets     -> step_info [T_total]
//   expert_case_kernel          (expert_kernels.hip, as it is) growth, status, radius per case
//   expert_team_degree_kernel   one workgroup per step, thread = agent: deg, s = sqrt(1.0 / deg) in fp64 with the
//                               case's radius -> workspace [T_total, N]; the agent's one-hot target
//   expert_team_graph_kernel    grid = row tiles x steps: kTeamGraphRows rows of S (and S64) per workgroup, the
//                               adjacency recomputed from the positions (no N^2 bits stored anywhere)
//   expert_team_observe_kernel  grid = 16-agent groups x steps: rollout_team_observe_kernel with step -> case
//
// The degrees go through memory because the tiles of a step all need every agent's s: one workgroup per step for the
// whole of S would leave a call of a few steps on a handful of compute units.
// Squared distances are unsigned (dist2_bound, dist2 of comm_graph.hip): a map of GNNPP_ROLLOUT_TEAM_MAX_CELLS
// cells can be 1 x 65536, (H-1)^2 + (W-1)^2 < 2^32.
// This file is included from gnnpp_api.hip after expert_kernels.hip and rollout_team_kernels.hip and uses their helpers.

namespace gnnpp {

constexpr int kTeamGraphRows = 32;            // rows of S per workgroup of expert_team_graph_kernel

typedef int v4i __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

__host__ __device__ inline size_t expert_team_scan_smem(int N) { return round16((size_t)8 * N) + 3 * kTeamWords * 8; }

// Pass 1.  step_info[t] = k_t | status << 16, the word expert_scan_kernel writes.  A step with a state off the map
// gets no graph search (k_t = 0): its case is flagged and not built.
__global__ __launch_bounds__(1024) void expert_team_scan_kernel(const ScheduleArgs p) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int N = p.N, t = blockIdx.x, a = threadIdx.x, nw = blockDim.x >> 6;
    int* px = reinterpret_cast<int*>(gnnpp_smem);                                   // [N]
    int* py = px + N;                                                               // [N]
    unsigned long long* fr[2] = {reinterpret_cast<unsigned long long*>(gnnpp_smem + round16((size_t)8 * N)), nullptr};
    fr[1] = fr[0] + kTeamWords;
    unsigned long long* words = fr[1] + kTeamWords;                                 // [kTeamWords]
    const int c = schedule_case_of(p.case_start, p.C, t);
    const int* pos = p.pos + (size_t)t * N * 2;
    const int* nxt = schedule_next_state(p, c, t, pos);
    const unsigned char* grid = p.grid + (p.grid_batched ? (size_t)c * p.H * p.W : 0);
    const bool live = a < N;
    bool bad_move = false, off_map = false, on_obstacle = false;
    int mx = 0, my = 0;
    if (live) {
        const int x = pos[2 * a], y = pos[2 * a + 1];
        schedule_agent_flags(p, grid, x, y, nxt[2 * a], nxt[2 * a + 1], bad_move, off_map, on_obstacle);
        mx = x; my = y;
        px[a] = x; py[a] = y;
    }
    int status = 0;
    if (team_any(bad_move, words, a, nw)) status |= GNNPP_SCHEDULE_BAD_MOVE;        // (its barriers publish px, py)
    const bool any_off = team_any(off_map, words, a, nw);
    if (any_off || team_any(on_obstacle, words, a, nw)) status |= GNNPP_SCHEDULE_BAD_STATE;
    int k = 0;
    if (!any_off) {                                              // (workgroup-uniform, like everything below)
        double r = p.radius0;
        unsigned built = 0;
        bool have = false;
        for (;;) {
            const unsigned Tu = dist2_bound(r);
            if (!have || Tu != built) {                          // same threshold = same graph: still disconnected
                have = true;
                built = Tu;
                bool in_r = a == 0;                              // reached set; the frontier starts as {0}
                int cur = 0;
                {
                    const unsigned long long m = __ballot(in_r);
                    if ((a & 63) == 0) fr[0][a >> 6] = m;
                }
                __syncthreads();
                for (;;) {
                    bool join = false;
                    if (live && !in_r) {
                        for (int w = 0; w < nw && !join; ++w) {
                            for (unsigned long long f = fr[cur][w]; f; f &= f - 1) {
                                const int j = w * 64 + __ffsll((long long)f) - 1;
                                if (dist2(px[j], py[j], mx, my) <= Tu) { join = true; break; }
                            }
                        }
                    }
                    in_r |= join;
                    const unsigned long long m = __ballot(join);
                    if ((a & 63) == 0) fr[cur ^ 1][a >> 6] = m;
                    __syncthreads();
                    bool any = false;
                    for (int w = 0; w < nw; ++w) any |= fr[cur ^ 1][w] != 0ull;
                    cur ^= 1;                                    // (the old frontier is rewritten only after a barrier)
                    if (!any) break;
                }
                if (!team_any(live && !in_r, words, a, nw)) break;          // connected
            }
            if (k == kGrowthCap) { status |= GNNPP_SCHEDULE_NO_RADIUS; break; }
            r = r * 1.1;
            ++k;
        }
    }
    if (a == 0) p.step_info[t] = k | (status << 16);
}

// The degree pass of step t of case c for agent a (a thread per agent, the whole workgroup calls it; LDS px | py [N]):
// inv[n] = sqrt(1.0 / deg) (fp64) under the case's final radius and tgt[n, 0..4] = the expert action, the one-hot of
// next - current in the order [-1,0] [0,-1] [1,0] [0,1] [0,0] (legal: pass 1).  inv / tgt: the step's rows of the
// caller's arrays -- row t of the sample calls, row b of a draw (schedule_draw_kernels.hip).
__device__ __forceinline__ void schedule_team_degree_step(const ScheduleArgs& p, int t, int c, int a, int* px, int* py,
                                                          double* inv, float* tgt) {
    const int N = p.N;
    const int* pos = p.pos + (size_t)t * N * 2;
    const bool live = a < N;
    int mx = 0, my = 0;
    if (live) { mx = pos[2 * a]; my = pos[2 * a + 1]; px[a] = mx; py[a] = my; }
    __syncthreads();
    if (!live) return;
    const unsigned Tu = dist2_bound(p.radius[c]);
    int deg = 0;
    for (int j = 0; j < N; ++j) deg += j != a && dist2(px[j], py[j], mx, my) <= Tu;
    inv[a] = inv_sqrt_degree(deg);
    const int* nxt = schedule_next_state(p, c, t, pos);
    const int dx = nxt[2 * a] - mx, dy = nxt[2 * a + 1] - my;
    expert_target_store(tgt + (size_t)a * 5, dx, dy);
}

// Pass 3: degrees with the case's final radius -> inv_ws[t, n] = sqrt(1.0 / deg) (fp64), and the expert action.  A
// flagged case is left unwritten (here and in the two kernels below).
__global__ __launch_bounds__(1024) void expert_team_degree_kernel(const ScheduleArgs p, double* inv_ws) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int N = p.N, t = blockIdx.x;
    const int c = schedule_case_of(p.case_start, p.C, t);
    if (p.status[c] != 0) return;                                // (workgroup-uniform)
    int* px = reinterpret_cast<int*>(gnnpp_smem);
    schedule_team_degree_step(p, t, c, threadIdx.x, px, px + N, inv_ws + (size_t)t * N, p.target + (size_t)t * N * 5);
}

// Rows [i0, i0 + kTeamGraphRows) of the S of step t of case c -> S (and S64 unless NULL), pointers to row i0 of the
// caller's matrix: S64 = s_i * s_j where d2 <= threshold and i != j, else 0; S = (float)S64.  inv_g [N]: the step's s.
// Consecutive threads store consecutive floats of a row; vec: four columns per thread and 16-byte stores (the launcher
// sets it when N % 4 == 0 and the outputs are 16-byte aligned).  256 threads; LDS: px | py | s of all N agents.
__device__ __forceinline__ void schedule_team_graph_tile(const ScheduleArgs& p, int t, int c, int i0, const double* inv_g,
                                                         float* S, double* S64, int vec, char* smem) {
    const int N = p.N, tid = threadIdx.x;
    const int np = (N + 3) & ~3;                                 // (the vector reads stay inside their array)
    int* px = reinterpret_cast<int*>(smem);                      // [np]
    int* py = px + np;                                           // [np]
    double* inv = reinterpret_cast<double*>(py + np);            // [np]
    const int* pos = p.pos + (size_t)t * N * 2;
    for (int n = tid; n < N; n += 256) { px[n] = pos[2 * n]; py[n] = pos[2 * n + 1]; inv[n] = inv_g[n]; }
    __syncthreads();
    const unsigned Tu = dist2_bound(p.radius[c]);
    const int rows = min(N, i0 + kTeamGraphRows) - i0;
    // item = (row r, column unit u) in row-major order, 256 items per pass: stepped without a division
    const int units = vec ? N >> 2 : N;
    const int dr = 256 / units, du = 256 - dr * units;
    int r = tid / units, u = tid - r * units;
    if (vec) {
        for (; r < rows; r += dr) {
            const int i = i0 + r, j = 4 * u;
            const int ix = px[i], iy = py[i];
            const double ii = inv[i];
            const v4i jx = *reinterpret_cast<const v4i*>(px + j), jy = *reinterpret_cast<const v4i*>(py + j);
            const v2d ja = *reinterpret_cast<const v2d*>(inv + j), jb = *reinterpret_cast<const v2d*>(inv + j + 2);
            const double ij[4] = {ja[0], ja[1], jb[0], jb[1]};
            double v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                v[e] = (i != j + e && dist2(jx[e], jy[e], ix, iy) <= Tu) ? ii * ij[e] : 0.0;
            const v4f o = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
            *reinterpret_cast<v4f*>(S + (size_t)r * N + j) = o;
            if (S64) {
                const v2d lo = {v[0], v[1]}, hi = {v[2], v[3]};
                v2d* o64 = reinterpret_cast<v2d*>(S64 + (size_t)r * N + j);
                o64[0] = lo; o64[1] = hi;
            }
            u += du;
            if (u >= units) { u -= units; ++r; }
        }
    } else {
        for (; r < rows; r += dr) {
            const int i = i0 + r;
            const double v = (i != u && dist2(px[u], py[u], px[i], py[i]) <= Tu) ? inv[i] * inv[u] : 0.0;
            S[(size_t)r * N + u] = (float)v;
            if (S64) S64[(size_t)r * N + u] = v;
            u += du;
            if (u >= units) { u -= units; ++r; }
        }
    }
}

// Pass 4: rows [tile * kTeamGraphRows, ...) of S[t] (and S64[t]).
__global__ __launch_bounds__(256) void expert_team_graph_kernel(const ScheduleArgs p, const double* inv_ws, int tiles,
                                                                 int vec) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int N = p.N;
    const int t = blockIdx.x / tiles, tile = blockIdx.x - t * tiles;
    const int c = schedule_case_of(p.case_start, p.C, t);
    if (p.status[c] != 0) return;                                // (workgroup-uniform)
    const int i0 = tile * kTeamGraphRows;
    schedule_team_graph_tile(p, t, c, i0, inv_ws + (size_t)t * N, p.S + ((size_t)t * N + i0) * N,
                             p.S64 ? p.S64 + ((size_t)t * N + i0) * N : nullptr, vec, gnnpp_smem);
}

// Observations of agents [n0, n0 + 16) of step t of case c -> row `out` of p.obs (the step itself in the sample calls,
// the pick of a draw).  256 threads; LDS as rollout_team_observe_kernel: goal_l [2N] | occupancy [H * W] | the stage of
// the output rows.
__device__ __forceinline__ void schedule_team_observe_group(const ScheduleArgs& p, int t, int c, int out, int n0,
                                                            char* smem) {
    int* goal_l = reinterpret_cast<int*>(smem);                              // [2N]
    unsigned char* cell = reinterpret_cast<unsigned char*>(smem + round16((size_t)8 * p.N));
    float* stage = reinterpret_cast<float*>(cell + round16((size_t)p.H * p.W));
    const RolloutArgs q = schedule_as_rollout(p);
    const int* pos = p.pos + (size_t)t * p.N * 2;
    observe_stage(q, c, cell, goal_l, threadIdx.x, 256);
    __syncthreads();
    observe_prep(q, pos, cell, goal_l, threadIdx.x, 256);
    __syncthreads();
    const int n1 = min(p.N, n0 + kObsAgentsPerWg);
    observe_rows(q, out, pos, n0, n1, cell, goal_l, threadIdx.x, 256, stage);
    __syncthreads();
    observe_flush(q, out, n0, n1, stage, threadIdx.x, 256);
}

// Pass 5: observations of 16 agents of one step; grid = groups x steps in one dimension.
__global__ __launch_bounds__(256) void expert_team_observe_kernel(const ScheduleArgs p, int groups) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int t = blockIdx.x / groups, n0 = (blockIdx.x - t * groups) * kObsAgentsPerWg;
    const int c = schedule_case_of(p.case_start, p.C, t);
    if (p.status[c] != 0) return;                                // (workgroup-uniform; its states may be off the map)
    schedule_team_observe_group(p, t, c, t, n0, gnnpp_smem);
}

inline size_t schedule_team_workspace_bytes(int N, int T_total) { return round16((size_t)T_total * N * sizeof(double)); }

// the observation launch of gnnpp_schedule_team_samples and gnnpp_schedule_team_fill_lists (expert_team_lists_kernel.hip)
inline void schedule_team_observe_launch(const ScheduleArgs& a, int groups, hipStream_t st) {
    static LdsAttrOnce once;
    set_lds_attr_once(once, reinterpret_cast<const void*>(&expert_team_observe_kernel), kTeamLdsBytes);
    hipLaunchKernelGGL(expert_team_observe_kernel, dim3(a.T_total * groups), dim3(256),
                       team_observe_smem(a.N, a.H, a.W), st, a, groups);
}

// the map fits the LDS occupancy grid and the workgroups a grid dimension
inline bool schedule_team_fits(const ScheduleArgs& a) {
    const int groups = (a.N + kObsAgentsPerWg - 1) / kObsAgentsPerWg;
    return (long long)a.H * a.W <= kTeamMaxCells && (long long)a.T_total * groups <= 0x7fffffffLL;
}

// GNNPP_OK, or GNNPP_ERR_UNSUPPORTED (the map does not fit the LDS occupancy grid, or more workgroups than a grid
// dimension holds) with nothing enqueued
int schedule_team_samples_launch(const ScheduleArgs& a, double* inv_ws, hipStream_t st) {
    const int nt = team_threads(a.N);
    const int tiles = (a.N + kTeamGraphRows - 1) / kTeamGraphRows;
    const int groups = (a.N + kObsAgentsPerWg - 1) / kObsAgentsPerWg;
    if (!schedule_team_fits(a)) return GNNPP_ERR_UNSUPPORTED;
    const size_t align = reinterpret_cast<size_t>(a.S) | reinterpret_cast<size_t>(a.S64);
    const int vec = (a.N & 3) == 0 && (align & 15) == 0;
    hipLaunchKernelGGL(expert_team_scan_kernel, dim3(a.T_total), dim3(nt), expert_team_scan_smem(a.N), st, a);
    hipLaunchKernelGGL(expert_case_kernel, dim3(a.C), dim3(64), 0, st, a);
    hipLaunchKernelGGL(expert_team_degree_kernel, dim3(a.T_total), dim3(nt), (size_t)8 * a.N, st, a, inv_ws);
    hipLaunchKernelGGL(expert_team_graph_kernel, dim3(a.T_total * tiles), dim3(256), (size_t)16 * ((a.N + 3) & ~3), st, a,
                       static_cast<const double*>(inv_ws), tiles, vec);
    schedule_team_observe_launch(a, groups, st);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

}  // namespace gnnpp
