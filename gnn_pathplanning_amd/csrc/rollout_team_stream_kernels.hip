// Streamed rollouts of teams of GNNPP_ROLLOUT_MAX_AGENTS < N <= GNNPP_ROLLOUT_MAX_TEAM agents
// (include/gnnpp_rollout_team_stream.h): the reseat of rollout_stream_kernels.hip for the large-team
// kernels, on the dense graph or on the neighbour lists.  Three launches per reseat, no atomics, nothing read on the host,
// one writer per word, all capturable.
//
// 1. rollout_stream_assign_kernel (rollout_stream_kernels.hip, as it is: it has no team-size limit).
// 2. rollout_team_stream_harvest_seat_kernel<lists>  one workgroup of team_threads(N) threads per slot, thread t = agent t.
//     done[b], slot_case[b] and assign[b] are read by every thread at entry and decide every branch that holds a barrier;
//     thread 0 rewrites them only behind a barrier.  Harvest: the table writes of rollout_stream_harvest_seat_kernel; the
//     fold of the relative records into makespan, flowtime and lived goes over up to 1024 agents, so wave 0 folds 64 strided
//     partial results and thread 0 folds those (integers: any order gives the same words).  Seat: the case's map, starts and
//     goals are copied into the slot and the episode's words are reset, then -- behind a barrier -- team_gso_body or
//     team_lists_body with grow = 1 builds the graph, radius and connected from the slot's own memory, as gnnpp_rollout_gso
//     and gnnpp_rollout_lists do at step 0.
// 3. rollout_team_stream_seat_observe_kernel  rollout_team_observe_kernel's grid; a workgroup whose slot this reseat did
//     not seat (assign[b] < 0, written by launch 1 alone) leaves at once, the others run team_observe_body.
// Included from gnnpp_api.hip after rollout_team_lists_kernel.hip and rollout_stream_kernels.hip.
#include "../../include/gnnpp_rollout_team_stream.h"

namespace gnnpp {

// harvest scratch: relative end and relative start (missing: 0) per agent, then 3 x 64 partial results
__host__ __device__ inline size_t team_stream_harvest_smem(int N) { return (size_t)8 * N + 3 * 64 * sizeof(int); }

inline size_t team_stream_seat_smem(int N) {
    const size_t h = team_stream_harvest_smem(N), g = team_gso_smem(N);
    return h > g ? h : g;
}

template <bool kLists>
__global__ __launch_bounds__(1024) void rollout_team_stream_harvest_seat_kernel(const RolloutArgs p, const RolloutStreamArgs s,
                                                                                int now, int* cnt_out,
                                                                                unsigned short* idx_out, float* val_out,
                                                                                int Np) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, N = p.N;
    const int c_old = s.slot_case[b], c_new = s.assign[b];
    if (p.done[b] == 0 || (c_old < 0 && c_new < 0)) return;  // (workgroup-uniform) a live slot, or an empty one that stays so
    int* pos = p.pos + (size_t)b * N * 2;
    int* reached = p.reached + (size_t)b * N;
    int* start_step = p.start_step + (size_t)b * N;
    int* end_step = p.end_step + (size_t)b * N;

    if (c_old >= 0) {                                        // ---- harvest
        int* red = reinterpret_cast<int*>(gnnpp_smem);       // [2][N]: relative end, relative start (missing: 0)
        int* part = red + 2 * N;                             // [3][64]: flow, max end, min start of agents l, l + 64, ...
        const int t0 = s.slot_t0[b];
        if (tid < N) {
            const int st = start_step[tid], e = end_step[tid];
            const int rs = st >= t0 ? st - t0 : (st < 0 ? -1 : 0);
            const int re = e < 0 ? -1 : e - t0;
            const size_t o = (size_t)c_old * N + tid;
            s.reached[o] = reached[tid];
            s.start_step[o] = rs;
            s.end_step[o] = re;
            s.pos[2 * o] = pos[2 * tid];
            s.pos[2 * o + 1] = pos[2 * tid + 1];
            red[tid] = re;
            red[N + tid] = rs < 0 ? 0 : rs;
        }
        __syncthreads();
        if (tid < 64) {
            int flow = 0, emax = -(1 << 30), smin = 1 << 30;
            for (int n = tid; n < N; n += 64) {
                const int e = red[n], st = red[N + n];
                flow += e - st;
                emax = e > emax ? e : emax;
                smin = st < smin ? st : smin;
            }
            part[tid] = flow; part[64 + tid] = emax; part[128 + tid] = smin;
        }
        __syncthreads();
        if (tid == 0) {
            int flow = 0, emax = -(1 << 30), smin = 1 << 30;
            for (int l = 0; l < 64; ++l) {
                flow += part[l];
                emax = part[64 + l] > emax ? part[64 + l] : emax;
                smin = part[128 + l] < smin ? part[128 + l] : smin;
            }
            const int limit = s.case_maxstep[c_old];
            s.stats[2 * c_old] = emax - smin;
            s.stats[2 * c_old + 1] = flow;
            s.lived[c_old] = emax + 1 < limit ? emax + 1 : limit;
            s.radius[c_old] = p.radius[b];
            s.slot[c_old] = b;
            s.t0[c_old] = t0;
        }
    }
    __syncthreads();                                         // every read of the old episode precedes the writes below
    if (c_new < 0) {
        if (tid == 0) s.slot_case[b] = -1;                   // harvested, nothing left to seat: empty, done stays set
        return;
    }

    // ---- seat
    const int HW = p.H * p.W;
    if (s.case_grid_batched) {
        const unsigned char* src = s.case_grid + (size_t)c_new * HW;
        unsigned char* dst = s.slot_grid + (size_t)b * HW;
        if ((HW & 3) == 0 && ((reinterpret_cast<size_t>(src) | reinterpret_cast<size_t>(dst)) & 3) == 0) {
            const unsigned* s4 = reinterpret_cast<const unsigned*>(src);
            unsigned* d4 = reinterpret_cast<unsigned*>(dst);
            for (int i = tid; i < (HW >> 2); i += nt) d4[i] = s4[i];
        } else {
            for (int i = tid; i < HW; i += nt) dst[i] = src[i];
        }
    }
    const int* cstart = s.case_start + (size_t)c_new * N * 2;
    const int* cgoal = s.case_goal + (size_t)c_new * N * 2;
    int* goal = s.goal + (size_t)b * N * 2;
    for (int i = tid; i < 2 * N; i += nt) {
        pos[i] = cstart[i];
        goal[i] = cgoal[i];
    }
    if (tid < N) {
        reached[tid] = 0;
        start_step[tid] = -1;
        end_step[tid] = -1;
    }
    if (tid == 0) {
        p.flags[3 * b] = 0; p.flags[3 * b + 1] = 0; p.flags[3 * b + 2] = 0;
        p.stats[2 * b] = 0; p.stats[2 * b + 1] = 0;
        if (p.choice_count) p.choice_count[b] = 0;
        s.maxstep[b] = now + s.case_maxstep[c_new];
        p.radius[b] = s.commR;
        p.done[b] = 0;
        s.slot_case[b] = c_new;
        s.slot_t0[b] = now;
    }
    __syncthreads();                                         // the slot's memory is the case: build its step-0 graph from it
    if (kLists) team_lists_body(p, b, tid, nt, 1, gnnpp_smem, cnt_out, idx_out, val_out, Np);
    else team_gso_body(p, b, tid, nt, 1, gnnpp_smem);
}

__global__ __launch_bounds__(256) void rollout_team_stream_seat_observe_kernel(const RolloutArgs p, const RolloutStreamArgs s) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int b = blockIdx.y;
    if (s.assign[b] < 0) return;                             // (workgroup-uniform) not seated by this reseat
    team_observe_body(p, b, blockIdx.x * kObsAgentsPerWg, threadIdx.x, gnnpp_smem);
}

// GNNPP_OK or GNNPP_ERR_LAUNCH (arguments checked by the entry point).  lists: NULL = the dense form, else a block of
// team_lists_bytes(r.B, r.N) bytes, 16-byte aligned
int rollout_team_stream_reseat_launch(const RolloutArgs& r, const RolloutStreamArgs& s, int now, void* lists, hipStream_t st) {
    static LdsAttrOnce once;
    set_lds_attr_once(once, reinterpret_cast<const void*>(&rollout_team_stream_seat_observe_kernel), kTeamLdsBytes);
    hipLaunchKernelGGL(rollout_stream_assign_kernel, dim3(1), dim3(kStreamThreads), kStreamThreads * sizeof(int), st, r, s);
    if (hipGetLastError() != hipSuccess) return GNNPP_ERR_LAUNCH;
    const dim3 grid(r.B), block(team_threads(r.N));
    const size_t smem = team_stream_seat_smem(r.N);
    if (lists) {
        const TeamLayout L = team_layout(r.B, r.N, 1, 2, 1, 1);
        char* base = static_cast<char*>(lists);
        hipLaunchKernelGGL(rollout_team_stream_harvest_seat_kernel<true>, grid, block, smem, st, r, s, now,
                           reinterpret_cast<int*>(base + L.cnt), reinterpret_cast<unsigned short*>(base + L.idx),
                           reinterpret_cast<float*>(base + L.val), L.Np);
    } else {
        hipLaunchKernelGGL(rollout_team_stream_harvest_seat_kernel<false>, grid, block, smem, st, r, s, now,
                           static_cast<int*>(nullptr), static_cast<unsigned short*>(nullptr), static_cast<float*>(nullptr), 0);
    }
    if (hipGetLastError() != hipSuccess) return GNNPP_ERR_LAUNCH;
    hipLaunchKernelGGL(rollout_team_stream_seat_observe_kernel, dim3((r.N + kObsAgentsPerWg - 1) / kObsAgentsPerWg, r.B),
                       dim3(256), team_observe_smem(r.N, r.H, r.W), st, r, s);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

static_assert(8 * kMaxTeam + 3 * 64 * 4 <= 64 * 1024 && 8 * kMaxTeam + 8 + 8 * kMaxTeam + 3 * kTeamWords * 8 + 16 <= 64 * 1024,
              "team stream seat kernel LDS: below the default limit");

}  // namespace gnnpp
