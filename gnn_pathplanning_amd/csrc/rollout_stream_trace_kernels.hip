// The trace of a streamed rollout (include/gnnpp_rollout_stream_trace.h): what rollout_trace_kernels.hip
// keeps per episode of a fixed batch, kept per CASE of a stream's queue.  A slot is reseated between two moves, so the
// tables are indexed by the case the slot holds (slot_case[b]) and their rows by the step RELATIVE to the seat
// (k = t - slot_t0[b]); both words are the stream's own, written by its reseat.  As in §5.11 nothing touches a simulator
// kernel: a small launch BEHIND the move reads `pos` and the move's argmax inputs, which are still in memory.
//
// rollout_stream_trace_begin_kernel / rollout_stream_trace_record_kernel    one THREAD per (case, agent) resp. (slot, agent),
//     consecutive threads are consecutive agents: the loads of pos and the stores of a row are coalesced.  A case sits in
//     exactly one slot exactly once, so every thread is the only writer of its row elements, its action byte and its two
//     counters, and the thread of agent 0 is the only writer of the case's steps word and the slot's seen_done word.  No
//     atomics, no LDS, no workspace; offsets into path and action are 64-bit.
//     Frozen at entry.  The record runs after the move and sees done[b] as the move LEFT it, so seen_done[b] keeps the
//     step of the record that first saw done[b] set for the slot's tenant.  The word is NEVER rewound at a seat: a value
//     counts only when it is younger than the seat, i.e. the tenant was frozen at entry of move t when
//     t0 < seen_done[b] < t, or t > maxstep[b].  A previous tenant's word is <= t0 by construction: the record that stored
//     it ran behind the move t' in which that tenant ended, a slot is reseated only once its episode has ended, and the
//     seat's step count `now` = t0 is at least t' (equal when the seat follows that very move).  begin's 0 is <= t0 too.
//     The word is read by every thread of the slot and written by one of them in the same launch, with no order between
//     the two: a reader finds either the old value, which is <= t0 (the writer only stores when it is), or the new t, and
//     neither satisfies "> t0 and < t", so the verdict does not depend on who came first.
//     A frozen or empty slot writes NOTHING (§5.11 repeats the last row; here the rows beyond steps[c] stay as begin left
//     them), and a step beyond the trace's last row (k > T_cap) writes nothing either: the kernel guards its own memory.
//     The action / moves / shielded arithmetic restates rollout_trace_record_kernel's (sharing it as a device function
//     would have meant editing that kernel).
#include "../../include/gnnpp_rollout_stream_trace.h"
#include "gnnpp_common.h"

namespace gnnpp {

constexpr int kStreamTraceThreads = 256;

struct RolloutStreamTraceArgs {
    const int* pos;          // [B,N,2] after the move
    const float* logits;     // [N,B,5] or nullptr
    const int* actions;      // [B,N] when logits == nullptr
    const int* maxstep;      // [B] in global steps (the seat's now + the case's limit)
    const int* done;         // [B]
    const int* slot_case;    // [B] -1 = empty
    const int* slot_t0;      // [B]
    const int* case_start;   // [C,N,2]
    int B, N, C, step, T_cap;
    int* path;
    signed char* action;
    int* moves;
    int* shielded;
    int* steps;
    int* seen_done;
};

__global__ __launch_bounds__(kStreamTraceThreads) void rollout_stream_trace_begin_kernel(const RolloutStreamTraceArgs a) {
    const long long i = (long long)blockIdx.x * kStreamTraceThreads + threadIdx.x;
    if (i < (long long)a.C * a.N) {
        if (a.moves) a.moves[i] = 0;
        if (a.shielded) a.shielded[i] = 0;
    }
    if (i < a.C) a.steps[i] = -1;
    if (i < a.B) a.seen_done[i] = 0;
}

__global__ __launch_bounds__(kStreamTraceThreads) void rollout_stream_trace_record_kernel(const RolloutStreamTraceArgs a) {
    const long long i = (long long)blockIdx.x * kStreamTraceThreads + threadIdx.x;
    if (i >= (long long)a.B * a.N) return;
    const int b = (int)(i / a.N), n = (int)(i - (long long)b * a.N);
    const int c = a.slot_case[b];
    if (c < 0 || c >= a.C) return;                           // an empty slot: nothing, seen_done[b] included
    const int t = a.step, t0 = a.slot_t0[b], k = t - t0;
    const int seen = a.seen_done[b];
    const bool frozen = (seen > t0 && seen < t) || t > a.maxstep[b];
    if (!frozen && k >= 1 && k <= a.T_cap) {
        const size_t cn = (size_t)c * a.N + n;
        int* row = a.path + (((size_t)c * (a.T_cap + 1) + k) * a.N + n) * 2;
        const int* before = k == 1 ? a.case_start + cn * 2 : row - (size_t)a.N * 2;
        const int px = before[0], py = before[1];
        const int x = a.pos[2 * i], y = a.pos[2 * i + 1];
        if (k == 1) {                                        // row 0: the starts, with the case's first record
            int* row0 = row - (size_t)a.N * 2;
            row0[0] = px;
            row0[1] = py;
        }
        row[0] = x;
        row[1] = y;
        int key = 4;
        if (a.action || a.shielded) {
            if (a.logits) {                                  // argmax of the logits, first max wins (move_body's rule)
                const float* l = a.logits + ((size_t)n * a.B + b) * 5;
                float best = l[0];
                key = 0;
#pragma unroll
                for (int j = 1; j < 5; ++j)
                    if (l[j] > best) { best = l[j]; key = j; }
            } else {
                key = a.actions[i];
            }
        }
        if (a.action) a.action[((size_t)c * a.T_cap + (k - 1)) * a.N + n] = (signed char)key;
        if (a.moves && (x != px || y != py)) a.moves[cn] += 1;
        if (a.shielded && key != 4) {
            const int dx = key == 0 ? -1 : key == 2 ? 1 : 0;
            const int dy = key == 1 ? -1 : key == 3 ? 1 : 0;
            if (x != px + dx || y != py + dy) a.shielded[cn] += 1;
        }
        if (n == 0) a.steps[c] = k;
    }
    if (n == 0 && !(seen > t0) && a.done[b] != 0) a.seen_done[b] = t;
}

inline RolloutStreamTraceArgs rollout_stream_trace_args(const gnnpp_rollout& r, const gnnpp_rollout_stream& s,
                                                        const gnnpp_rollout_stream_trace& tr) {
    RolloutStreamTraceArgs a;
    a.pos = r.pos;
    a.logits = r.logits;
    a.actions = r.actions;
    a.maxstep = r.maxstep;
    a.done = r.done;
    a.slot_case = s.slot_case;
    a.slot_t0 = s.slot_t0;
    a.case_start = s.case_start;
    a.B = r.B;
    a.N = r.N;
    a.C = s.C;
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

// GNNPP_OK or GNNPP_ERR_LAUNCH (arguments checked by the entry points)
int rollout_stream_trace_begin_launch(const gnnpp_rollout& r, const gnnpp_rollout_stream& s,
                                      const gnnpp_rollout_stream_trace& tr, hipStream_t st) {
    const size_t rows = (size_t)s.C * r.N;
    if (hipMemsetAsync(tr.path, 0, rows * (tr.T_cap + 1) * 2 * sizeof(int), st) != hipSuccess) return GNNPP_ERR_LAUNCH;
    if (tr.action && hipMemsetAsync(tr.action, 0xff, rows * tr.T_cap, st) != hipSuccess)     // -1: nothing recorded
        return GNNPP_ERR_LAUNCH;
    long long n = (long long)rows;
    if (r.B > n) n = r.B;
    hipLaunchKernelGGL(rollout_stream_trace_begin_kernel, dim3((unsigned)((n + kStreamTraceThreads - 1) / kStreamTraceThreads)),
                       dim3(kStreamTraceThreads), 0, st, rollout_stream_trace_args(r, s, tr));
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

int rollout_stream_trace_record_launch(const gnnpp_rollout& r, const gnnpp_rollout_stream& s,
                                       const gnnpp_rollout_stream_trace& tr, hipStream_t st) {
    const long long n = (long long)r.B * r.N;
    hipLaunchKernelGGL(rollout_stream_trace_record_kernel, dim3((unsigned)((n + kStreamTraceThreads - 1) / kStreamTraceThreads)),
                       dim3(kStreamTraceThreads), 0, st, rollout_stream_trace_args(r, s, tr));
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

}  // namespace gnnpp
