// The trace of a batched rollout (include/gnnpp_rollout_trace.h): every step's positions in the solvers'
// schedule layout, the action every agent asked for, and per-agent counters of moves and of shielded steps.  Recording
// touches no simulator kernel: a move leaves `pos` in memory and its argmax inputs (`logits` or `actions`) are still
// there, so a small kernel BEHIND the move writes the row.
//
// rollout_trace_begin_kernel / rollout_trace_record_kernel    one THREAD per (episode, agent), consecutive threads are
//     consecutive agents: the loads of pos and the stores of a row are coalesced, every thread is the only writer of its
//     row element, its action byte and its two counters, and the thread of agent 0 is the only writer of the episode's
//     steps / seen_done words.  No atomics, no LDS, no workspace; offsets into path and action are 64-bit (B (T_cap + 1)
//     N 2 passes 2^31 for shapes the rollout accepts).
//     Frozen at entry.  The record runs after the move and sees done[b] as the move LEFT it: it cannot tell "ended in
//     this call" from "ended earlier".  seen_done[b] therefore keeps the step of the record that first saw done[b] set
//     (0: not seen yet), and the episode was frozen at entry of move t when 0 < seen_done[b] < t or t > maxstep[b] -- the
//     move kernels' own condition.  The word is read by every thread of the episode and written by one of them in the
//     same launch, with no order between the two: a reader finds either the old 0 or the new t, and neither is "< t", so
//     the verdict does not depend on who came first.
#include "../../include/gnnpp_rollout_trace.h"
#include "gnnpp_common.h"

namespace gnnpp {

constexpr int kTraceThreads = 256;

struct RolloutTraceArgs {
    const int* pos;          // [B,N,2] after the move
    const float* logits;     // [N,B,5] or nullptr
    const int* actions;      // [B,N] when logits == nullptr
    const int* maxstep;      // [B] or nullptr
    const int* done;         // [B] or nullptr
    int B, N, step, T_cap;
    int* path;
    signed char* action;
    int* moves;
    int* shielded;
    int* steps;
    int* seen_done;
};

__global__ __launch_bounds__(kTraceThreads) void rollout_trace_begin_kernel(const RolloutTraceArgs a) {
    const long long i = (long long)blockIdx.x * kTraceThreads + threadIdx.x;
    if (i >= (long long)a.B * a.N) return;
    const int b = (int)(i / a.N), n = (int)(i - (long long)b * a.N);
    int* row = a.path + ((size_t)b * (a.T_cap + 1) * a.N + n) * 2;
    row[0] = a.pos[2 * i];
    row[1] = a.pos[2 * i + 1];
    if (a.moves) a.moves[i] = 0;
    if (a.shielded) a.shielded[i] = 0;
    if (n == 0) {
        a.steps[b] = 0;
        a.seen_done[b] = 0;
    }
}

__global__ __launch_bounds__(kTraceThreads) void rollout_trace_record_kernel(const RolloutTraceArgs a) {
    const long long i = (long long)blockIdx.x * kTraceThreads + threadIdx.x;
    if (i >= (long long)a.B * a.N) return;
    const int b = (int)(i / a.N), n = (int)(i - (long long)b * a.N);
    const int t = a.step;
    int* row = a.path + (((size_t)b * (a.T_cap + 1) + t) * a.N + n) * 2;
    const int* before = row - (size_t)a.N * 2;
    const int x = a.pos[2 * i], y = a.pos[2 * i + 1];
    row[0] = x;
    row[1] = y;
    const int seen = a.seen_done[b];
    const bool frozen = (seen != 0 && seen < t) || (a.maxstep && t > a.maxstep[b]);
    if (!frozen) {
        int key = 4;
        if (a.action || a.shielded) {
            if (a.logits) {                                  // argmax of the logits, first max wins (move_body's rule)
                const float* l = a.logits + ((size_t)n * a.B + b) * 5;
                float best = l[0];
                key = 0;
#pragma unroll
                for (int k = 1; k < 5; ++k)
                    if (l[k] > best) { best = l[k]; key = k; }
            } else {
                key = a.actions[i];
            }
        }
        const int px = before[0], py = before[1];
        if (a.action) a.action[((size_t)b * a.T_cap + (t - 1)) * a.N + n] = (signed char)key;
        if (a.moves && (x != px || y != py)) a.moves[i] += 1;
        if (a.shielded && key != 4) {
            const int dx = key == 0 ? -1 : key == 2 ? 1 : 0;
            const int dy = key == 1 ? -1 : key == 3 ? 1 : 0;
            if (x != px + dx || y != py + dy) a.shielded[i] += 1;
        }
    }
    if (n == 0) {
        if (!frozen) a.steps[b] = t;
        if (seen == 0 && a.done && a.done[b] != 0) a.seen_done[b] = t;
    }
}

inline RolloutTraceArgs rollout_trace_args(const gnnpp_rollout& r, const gnnpp_rollout_trace& tr) {
    RolloutTraceArgs a;
    a.pos = r.pos;
    a.logits = r.logits;
    a.actions = r.actions;
    a.maxstep = r.maxstep;
    a.done = r.done;
    a.B = r.B;
    a.N = r.N;
    a.step = r.currentstep;
    a.T_cap = tr.T_cap;
    a.path = tr.path;
    a.action = tr.action;
    a.moves = tr.moves;
    a.shielded = tr.shielded;
    a.steps = tr.steps;
    a.seen_done = tr.seen_done;
    return a;
}

inline unsigned rollout_trace_blocks(const gnnpp_rollout& r) {
    return (unsigned)(((long long)r.B * r.N + kTraceThreads - 1) / kTraceThreads);
}

// GNNPP_OK or GNNPP_ERR_LAUNCH (arguments checked by the entry points)
int rollout_trace_begin_launch(const gnnpp_rollout& r, const gnnpp_rollout_trace& tr, hipStream_t st) {
    if (tr.action &&
        hipMemsetAsync(tr.action, 0xff, (size_t)r.B * tr.T_cap * r.N, st) != hipSuccess)     // -1: nothing recorded
        return GNNPP_ERR_LAUNCH;
    hipLaunchKernelGGL(rollout_trace_begin_kernel, dim3(rollout_trace_blocks(r)), dim3(kTraceThreads), 0, st,
                       rollout_trace_args(r, tr));
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

int rollout_trace_record_launch(const gnnpp_rollout& r, const gnnpp_rollout_trace& tr, hipStream_t st) {
    hipLaunchKernelGGL(rollout_trace_record_kernel, dim3(rollout_trace_blocks(r)), dim3(kTraceThreads), 0, st,
                       rollout_trace_args(r, tr));
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

}  // namespace gnnpp
