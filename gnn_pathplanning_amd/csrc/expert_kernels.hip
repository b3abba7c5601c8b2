// Training samples from expert schedules: what the reference's two transformers
//
//   offlineExpert/DataGen_Transformer.py:295-371, 466-515
//   onlineExpert/DataTransformer_local_onlineExpert.py (pathtransformer_RelativeCoordinate, computeAdjacencyMatrix)
//
// compute on the host, per solved case, in python loops: for every step t of a schedule (positions of N agents over
// T steps, map, goals) the observation tensor [N,3,11,11], the normalised communication graph [N,N] and the one-hot
// expert action [N,5].  Here C cases with T_total steps in all are one call.
//
// The schedule's graph rule is NOT the rollout's: the radius starts at radius0, is multiplied by 1.1 until the graph
// of a step is connected, is carried from step to step, and after the last step the FINAL radius rebuilds every step.
// The radius only grows and connectivity is monotone in it, so the sequential scan equals: every step t finds, on
// its own, the smallest k_t with the graph at radius0 * 1.1^k connected; growth = max_t k_t; radius = radius0
// multiplied growth times by 1.1 (repeated fp64 multiplication: the reference's bits); every step is rebuilt with it.
// Three launches on one stream, no atomics and no hand-off between workgroups (so nothing depends on which
// workgroups are resident and every output has one writer):
//
//   expert_scan_kernel     one WAVE per step: legality of the step's states and moves, k_t       -> step_info [T_total]
//   expert_case_kernel     one wave per case: max / OR over the case's steps -> growth, status, radius [C]
//   expert_samples_kernel  one workgroup per step: target, S (+ fp64 S), observations with the case's radius
//
// A single launch would need the per-case maximum before any step's graph: a spin-wait on the other steps'
// workgroups, i.e. a co-residency assumption (a case may have more steps than the chip holds workgroups).  The two
// extra launches cost microseconds against a call that writes ~14.5 KB per step.
//
// Observations are AgentState.toSeqInputTensor == toInputTensor per step: rollout_kernels.hip's observe_stage /
// observe_prep / observe_rows / observe_flush, called with step -> case indirection for map and goal.
#include "../../include/gnnpp.h"
#include "gnnpp_common.h"

namespace gnnpp {

typedef ::gnnpp_schedules ScheduleArgs;

constexpr int kScanStepsPerWg = 4;            // expert_scan_kernel: 256 threads = 4 waves = 4 steps

// largest c with case_start[c] <= t (case_start [C + 1] ascending, case_start[0] = 0): wave-uniform
__device__ __forceinline__ int schedule_case_of(const int* case_start, int C, int t) {
    int lo = 0, hi = C - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (case_start[mid] <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the observation builders read their sizes and pointers from a gnnpp_rollout: B = steps, one map / goal set per CASE
__device__ __forceinline__ RolloutArgs schedule_as_rollout(const ScheduleArgs& p) {
    RolloutArgs q = {};
    q.grid = p.grid; q.grid_batched = p.grid_batched; q.goal = p.goal;
    q.B = p.T_total; q.N = p.N; q.H = p.H; q.W = p.W;
    q.obs = p.obs;
    return q;
}

// ---- per-agent pieces shared with expert_team_kernels.hip -------------------------------------------------------
// the states step t moves to: the next step's, after a case's last state the goal
__device__ __forceinline__ const int* schedule_next_state(const ScheduleArgs& p, int c, int t, const int* pos) {
    const bool last = t + 1 >= p.case_start[c + 1] || t + 1 >= p.T_total;
    return last ? p.goal + (size_t)c * p.N * 2 : pos + 2 * p.N;
}

// legality of one agent's state (x, y) and of its move to (nx, ny)
__device__ __forceinline__ void schedule_agent_flags(const ScheduleArgs& p, const unsigned char* grid, int x, int y,
                                                     int nx, int ny, bool& bad_move, bool& off_map, bool& on_obstacle) {
    // one of [-1,0] [0,-1] [1,0] [0,1] [0,0] (compared, not subtracted: no overflow on wild input)
    const bool legal = (nx == x && (ny == y || ny == y - 1 || ny == y + 1)) ||
                       (ny == y && (nx == x - 1 || nx == x + 1));
    bad_move = !legal;
    off_map = x < 0 || x >= p.H || y < 0 || y >= p.W;
    on_obstacle = !off_map && grid[(size_t)x * p.W + y] != 0;
}

// expert action: one-hot of next - current = (dx, dy) in the order [-1,0] [0,-1] [1,0] [0,1] [0,0] (legal: pass 1)
__device__ __forceinline__ void expert_target_store(float* o, int dx, int dy) {
    const int a = dx == -1 ? 0 : dy == -1 ? 1 : dx == 1 ? 2 : dy == 1 ? 3 : 4;
#pragma unroll
    for (int j = 0; j < 5; ++j) o[j] = j == a ? 1.f : 0.f;
}

// Pass 1.  Lane l of the step's wave holds agents l and l + 64 (the one-wave form of comm_graph.hip).  step_info[t] =
// k_t | status << 16.  A step with a state off the map gets no graph search (k_t = 0): its case is flagged and not built.
__global__ __launch_bounds__(256) void expert_scan_kernel(const ScheduleArgs p) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * kScanStepsPerWg + (threadIdx.x >> 6);
    if (t >= p.T_total) return;                                  // (whole wave; the kernel has no workgroup barrier)
    const int N = p.N;
    const bool two = N > 64;
    const int c = schedule_case_of(p.case_start, p.C, t);
    const int* pos = p.pos + (size_t)t * N * 2;
    const int* nxt = schedule_next_state(p, c, t, pos);
    const unsigned char* grid = p.grid + (p.grid_batched ? (size_t)c * p.H * p.W : 0);
    const WaveAgents A = wave_agents_load(pos, N, lane);
    bool bad_move[2], off_map[2], on_obstacle[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int n = lane + 64 * h;
        bad_move[h] = off_map[h] = on_obstacle[h] = false;
        if (A.live[h]) {
            schedule_agent_flags(p, grid, A.px[h], A.py[h], nxt[2 * n], nxt[2 * n + 1], bad_move[h], off_map[h],
                                 on_obstacle[h]);
        }
    }
    const MaskPair m_move = ballot2(bad_move[0], two && bad_move[1]);
    const MaskPair m_off = ballot2(off_map[0], two && off_map[1]);
    const MaskPair m_obs = ballot2(on_obstacle[0], two && on_obstacle[1]);
    int status = 0;
    if (m_move.lo | m_move.hi) status |= GNNPP_SCHEDULE_BAD_MOVE;
    if (m_off.lo | m_off.hi | m_obs.lo | m_obs.hi) status |= GNNPP_SCHEDULE_BAD_STATE;
    int k = 0;
    // A.px / A.py hold the states as given, wild ones included: this guard alone keeps them out of dist2 (a step with a
    // state off the map gets no search), so below every coordinate is a cell of the map
    if (!(m_off.lo | m_off.hi)) {                                // (wave-uniform)
        WaveRows rows = {{0ull, 0ull}, {0ull, 0ull}};
        // The launcher accepts H, W <= 16384 and the API radius0 > 0 only: d2 < 2^29 and thresholds >= 0, where the unsigned
        // dist2 <= dist2_bound and the signed test with a 2^31 - 1 clamp it replaces agree on every pair: the same k_t.
        k = expert_radius_search(p.radius0, status, [&](unsigned Tu) {
            wave_adjacency_rows(A, N, lane, Tu, rows);
            return wave_connected(rows, A.live, N);
        });
    }
    if (lane == 0) p.step_info[t] = k | (status << 16);
}

// Pass 2: one wave per case.  growth = max k_t, status = OR, radius = radius0 * 1.1 * 1.1 ... (growth times).
__global__ __launch_bounds__(64) void expert_case_kernel(const ScheduleArgs p) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int t0 = p.case_start[c], t1 = min(p.case_start[c + 1], p.T_total);
    int kmax = 0, st = 0;
    for (int t = t0 + lane; t < t1; t += 64) {
        const int v = p.step_info[t];
        kmax = max(kmax, v & 0xffff);
        st |= v >> 16;
    }
    for (int l = 1; l < 64; ++l) {                               // (every lane ends with lane 0's view of the wave)
        kmax = max(kmax, __builtin_amdgcn_readlane(kmax, l));
        st |= __builtin_amdgcn_readlane(st, l);
    }
    if (lane == 0) {
        double r = p.radius0;
        for (int i = 0; i < kmax; ++i) r = r * 1.1;
        p.growth[c] = kmax;
        p.status[c] = st;
        p.radius[c] = r;
    }
}

// Pass 3: one workgroup per step.  LDS: goal_l [2 kMaxAgents] ints | graph [kGsoSmemBytes] | occupancy [H * W] |
// (staged) kObsStageBytes of observation rows.  A flagged case is left unwritten (its states may be off the map).
__global__ __launch_bounds__(256) void expert_samples_kernel(const ScheduleArgs p, int staged) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int t = blockIdx.x, tid = threadIdx.x, N = p.N;
    const int c = schedule_case_of(p.case_start, p.C, t);
    if (p.status[c] != 0) return;                                // (workgroup-uniform)
    int* goal_l = reinterpret_cast<int*>(gnnpp_smem);
    char* gso_smem = gnnpp_smem + 2 * kMaxAgents * sizeof(int);
    unsigned char* cell = reinterpret_cast<unsigned char*>(gso_smem + kGsoSmemBytes);
    const size_t occ_bytes = ((size_t)p.H * p.W + 15) & ~(size_t)15;
    float* stage = staged ? reinterpret_cast<float*>(cell + occ_bytes) : nullptr;
    const RolloutArgs q = schedule_as_rollout(p);
    const int* pos = p.pos + (size_t)t * N * 2;
    const double radius = p.radius[c];

    const int* nxt = schedule_next_state(p, c, t, pos);
    for (int n = tid; n < N; n += 256) {
        expert_target_store(p.target + ((size_t)t * N + n) * 5, nxt[2 * n] - pos[2 * n], nxt[2 * n + 1] - pos[2 * n + 1]);
    }

    observe_stage(q, c, cell, goal_l, tid, 256);
    __syncthreads();
    if (tid < 64) gso_wave0(q, pos, false, radius, gso_smem, tid);
    else observe_prep(q, pos, cell, goal_l, tid - 64, 256 - 64);
    __syncthreads();

    gso_store_S(gso_layout(gso_smem), N, p.S + (size_t)t * N * N, p.S64 ? p.S64 + (size_t)t * N * N : nullptr, tid, 256);

    for (int n0 = 0; n0 < N; n0 += kObsAgentsPerWg) {            // 16 agents' rows at a time through the LDS stage
        const int n1 = min(N, n0 + kObsAgentsPerWg);
        observe_rows(q, t, pos, n0, n1, cell, goal_l, tid, 256, stage);
        if (stage) {                                             // (workgroup-uniform)
            __syncthreads();
            observe_flush(q, t, n0, n1, stage, tid, 256);
            __syncthreads();
        }
    }
}

// GNNPP_OK, or GNNPP_ERR_UNSUPPORTED (map too large for the LDS occupancy grid) with nothing enqueued
int schedule_samples_launch(const ScheduleArgs& a, hipStream_t st) {
    const size_t occ = ((size_t)a.H * a.W + 15) & ~(size_t)15;
    size_t smem = 2 * kMaxAgents * sizeof(int) + kGsoSmemBytes + occ;
    if (smem > 64 * 1024 || a.H > 16384 || a.W > 16384) return GNNPP_ERR_UNSUPPORTED;
    const int staged = smem + kObsStageBytes <= 64 * 1024;      // the output stage, while the default LDS limit allows
    if (staged) smem += kObsStageBytes;
    hipLaunchKernelGGL(expert_scan_kernel, dim3((a.T_total + kScanStepsPerWg - 1) / kScanStepsPerWg), dim3(256), 0, st, a);
    hipLaunchKernelGGL(expert_case_kernel, dim3(a.C), dim3(64), 0, st, a);
    hipLaunchKernelGGL(expert_samples_kernel, dim3(a.T_total), dim3(256), smem, st, a, staged);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

}  // namespace gnnpp
