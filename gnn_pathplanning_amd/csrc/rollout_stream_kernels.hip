// Streamed rollouts (include/gnnpp_rollout_stream.h): B episode slots stay resident, and between two
// steps a slot whose episode has ended hands its result to a per-case table and takes the next case of a queue.  Two
// launches per reseat, no atomics, nothing read on the host, both capturable.
//
// rollout_stream_assign_kernel        ONE workgroup.  Thread t owns the contiguous slots [t * per, (t + 1) * per); it counts
//     its done slots, an inclusive scan over the 256 counts in LDS (8 rounds) turns the counts into each thread's rank of
//     its first done slot, and the k-th done slot in slot order gets case cursor + k while that is < C.  Thread 0 advances
//     the cursor behind a barrier that every thread's read of it precedes.
// rollout_stream_harvest_seat_kernel  one workgroup of 256 threads per slot.  done[b], slot_case[b] and assign[b] are
//     read by every thread at entry and decide everything workgroup-uniformly; thread 0 rewrites them only behind a
//     barrier.  Harvest: thread n owns agent n's row elements, thread 0 folds the relative records into makespan and
//     flowtime in the move kernel's own order of operations (integers: any order gives the same words).  Seat: the case's
//     map, starts and goals are copied into the slot and the episode's words are reset, then -- behind a barrier, so the
//     copies are visible to the workgroup -- gso_body(grow = 1) and the observe_* stages of rollout_kernels.hip build S,
//     radius, connected and the observations from the slot's own memory, exactly as gnnpp_rollout_gso and
//     gnnpp_rollout_observe do at step 0.  The graph scratch and the observation scratch share one LDS block (the graph is
//     stored before the map is staged), so the request is that of gnnpp_rollout_gso_observe.
#include "../../include/gnnpp_rollout_stream.h"
#include "gnnpp_common.h"

namespace gnnpp {

constexpr int kStreamThreads = 256;

typedef ::gnnpp_rollout_stream RolloutStreamArgs;

__global__ __launch_bounds__(kStreamThreads) void rollout_stream_begin_kernel(const RolloutArgs p, const RolloutStreamArgs s) {
    const long long i = (long long)blockIdx.x * kStreamThreads + threadIdx.x;
    const long long CN = (long long)s.C * p.N;
    if (i < CN) {
        s.reached[i] = -1;
        s.start_step[i] = -1;
        s.end_step[i] = -1;
        s.pos[2 * i] = -1;
        s.pos[2 * i + 1] = -1;
    }
    if (i < s.C) {
        s.radius[i] = -1.0;
        s.stats[2 * i] = -1;
        s.stats[2 * i + 1] = -1;
        s.lived[i] = -1;
        s.slot[i] = -1;
        s.t0[i] = -1;
    }
    if (i < p.B) {
        p.done[i] = 1;
        s.slot_case[i] = -1;
        s.slot_t0[i] = 0;
        s.assign[i] = -1;
    }
    if (i == 0) *s.cursor = 0;
}

__global__ __launch_bounds__(kStreamThreads) void rollout_stream_assign_kernel(const RolloutArgs p, const RolloutStreamArgs s) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    int* scan = reinterpret_cast<int*>(gnnpp_smem);            // [kStreamThreads]
    const int tid = threadIdx.x;
    const int per = (p.B + kStreamThreads - 1) / kStreamThreads;
    const int b0 = min(tid * per, p.B), b1 = min(b0 + per, p.B);
    const int cursor = *s.cursor;
    int mine = 0;
    for (int b = b0; b < b1; ++b) mine += p.done[b] != 0;
    scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < kStreamThreads; d <<= 1) {           // inclusive scan, one read and one write phase per round
        const int add = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    int k = scan[tid] - mine;                                // done slots before my first one
    for (int b = b0; b < b1; ++b) {
        int c = -1;
        if (p.done[b] != 0) {
            if (k < s.C - cursor) c = cursor + k;            // (cursor <= C: no overflow)
            ++k;
        }
        s.assign[b] = c;
    }
    if (tid == 0) {                                          // (every thread read the cursor before the scan's barriers)
        const int total = scan[kStreamThreads - 1];
        *s.cursor = total < s.C - cursor ? cursor + total : s.C;
    }
}

__global__ __launch_bounds__(kStreamThreads) void rollout_stream_harvest_seat_kernel(const RolloutArgs p,
                                                                                     const RolloutStreamArgs s, int now) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int b = blockIdx.x, tid = threadIdx.x, N = p.N;
    const int c_old = s.slot_case[b], c_new = s.assign[b];
    if (p.done[b] == 0 || (c_old < 0 && c_new < 0)) return;  // (workgroup-uniform) a live slot, or an empty one that stays so
    int* pos = p.pos + (size_t)b * N * 2;
    int* reached = p.reached + (size_t)b * N;
    int* start_step = p.start_step + (size_t)b * N;
    int* end_step = p.end_step + (size_t)b * N;

    if (c_old >= 0) {                                        // ---- harvest
        int* red = reinterpret_cast<int*>(gnnpp_smem);       // [2][kMaxAgents]: relative end, relative start (missing: 0)
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
            red[kMaxAgents + tid] = rs < 0 ? 0 : rs;
        }
        __syncthreads();
        if (tid == 0) {
            int flow = 0, emax = -(1 << 30), smin = 1 << 30;
            for (int n = 0; n < N; ++n) {
                const int e = red[n], st = red[kMaxAgents + n];
                flow += e - st;
                emax = e > emax ? e : emax;
                smin = st < smin ? st : smin;
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
            for (int i = tid; i < (HW >> 2); i += kStreamThreads) d4[i] = s4[i];
        } else {
            for (int i = tid; i < HW; i += kStreamThreads) dst[i] = src[i];
        }
    }
    const int* cstart = s.case_start + (size_t)c_new * N * 2;
    const int* cgoal = s.case_goal + (size_t)c_new * N * 2;
    int* goal = s.goal + (size_t)b * N * 2;
    for (int i = tid; i < 2 * N; i += kStreamThreads) {
        pos[i] = cstart[i];
        goal[i] = cgoal[i];
    }
    for (int n = tid; n < N; n += kStreamThreads) {
        reached[n] = 0;
        start_step[n] = -1;
        end_step[n] = -1;
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
    __syncthreads();                                         // the slot's memory is the case: build its step-0 state from it
    gso_body(p, b, pos, true, gnnpp_smem, tid, kStreamThreads);
    __syncthreads();                                         // (the graph's LDS is read to the end before the map lands on it)
    int* goal_l = reinterpret_cast<int*>(gnnpp_smem);                       // [2 kMaxAgents]
    unsigned char* cell = reinterpret_cast<unsigned char*>(goal_l + 2 * kMaxAgents);
    observe_stage(p, b, cell, goal_l, tid, kStreamThreads);
    __syncthreads();
    observe_prep(p, pos, cell, goal_l, tid, kStreamThreads);
    __syncthreads();
    observe_rows(p, b, pos, 0, N, cell, goal_l, tid, kStreamThreads);
}

inline unsigned rollout_stream_begin_blocks(const RolloutArgs& r, const RolloutStreamArgs& s) {
    long long n = (long long)s.C * r.N;
    if (r.B > n) n = r.B;
    return (unsigned)((n + kStreamThreads - 1) / kStreamThreads);
}

// GNNPP_OK or GNNPP_ERR_LAUNCH (arguments checked by the entry points)
int rollout_stream_begin_launch(const RolloutArgs& r, const RolloutStreamArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(rollout_stream_begin_kernel, dim3(rollout_stream_begin_blocks(r, s)), dim3(kStreamThreads), 0, st,
                       r, s);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

int rollout_stream_reseat_launch(const RolloutArgs& r, const RolloutStreamArgs& s, int now, hipStream_t st) {
    const size_t occ = ((size_t)r.H * r.W + 15) & ~(size_t)15;
    size_t smem = occ + 2 * kMaxAgents * sizeof(int);        // the observation scratch of gnnpp_rollout_gso_observe ...
    if (smem < (size_t)kGsoSmemBytes) smem = kGsoSmemBytes;   // ... or its graph scratch, whichever is larger
    static LdsAttrOnce once;
    set_lds_attr_once(once, reinterpret_cast<const void*>(&rollout_stream_harvest_seat_kernel), (int)kObserveMaxSmem);
    hipLaunchKernelGGL(rollout_stream_assign_kernel, dim3(1), dim3(kStreamThreads), kStreamThreads * sizeof(int), st, r, s);
    if (hipGetLastError() != hipSuccess) return GNNPP_ERR_LAUNCH;
    hipLaunchKernelGGL(rollout_stream_harvest_seat_kernel, dim3(r.B), dim3(kStreamThreads), smem, st, r, s, now);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

}  // namespace gnnpp
