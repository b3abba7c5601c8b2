/* The trace of a streamed rollout, kept on the device per CASE of the stream's queue: every step's positions, the action
 * every agent asked for, and per-agent counters of moves and of shielded steps -- three entry points of libgnnpp.so, added
 * without a version change (gnnpp_version() stays 330) and kept in a header of their own: gnnpp.h, gnnpp_rollout_trace.h,
 * gnnpp_rollout_stream.h and the other companion headers are exactly what they were, and so is every kernel behind them.
 * csrc/rollout_stream_trace_kernels.hip; DESIGN.md 5.13.
 *
 * gnnpp_rollout_trace (gnnpp_rollout_trace.h) is laid out per episode of a fixed batch and its rows are global steps.  A
 * stream (gnnpp_rollout_stream.h) reseats a slot between two moves: the case c = slot_case[b] that slot b holds was seated
 * at step count t0 = slot_t0[b], and its step k runs as global step t0 + k.  The tables here have one row block per CASE
 * and their rows are RELATIVE to the seat, so what they hold for a case is what a recorded plain rollout of that case
 * alone holds in rows 0 .. steps.  A trace is filled by one small launch BEHIND each move, as there.  No call here
 * synchronises with the host; every call is capturable in a HIP graph and enqueues nothing on an error.  One thread per
 * (slot, agent), one writer per output element (a case sits in exactly one slot exactly once), no atomics: two identical
 * streams give the same bytes. */
#ifndef GNNPP_ROLLOUT_STREAM_TRACE_H_
#define GNNPP_ROLLOUT_STREAM_TRACE_H_

#include "gnnpp.h"
#include "gnnpp_rollout_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HOST struct of DEVICE pointers; B and N are the rollout's, C is the stream's.
 *
 * What gnnpp_rollout_stream_trace_record writes behind the move of global step t = r->currentstep, for slot b:
 *   c = slot_case[b] < 0: the slot is empty.  Nothing is written, seen_done[b] included.
 *   t0 = slot_t0[b], k = t - t0.  The slot's tenant was FROZEN AT ENTRY of that move when
 *       (seen_done[b] > t0 && seen_done[b] < t) || t > maxstep[b]
 *   and then nothing at all is written: unlike gnnpp_rollout_trace no row is repeated, the rows of case c beyond steps[c]
 *   stay as begin left them (0) and action stays -1 there.  Otherwise, when k <= T_cap (a later step writes nothing:
 *   the call guards its own memory; size the trace for the longest case):
 *   path[c,0,n]      = case_start[c,n], written with the record of k = 1.
 *   path[c,k,n]      = pos[b,n].
 *   action[c,k-1,n]  = the action the agent asked for: the first maximum of logits[n,b,0..4] by exactly the comparison of
 *                      the move kernels (`l[j] > best`: the lowest index wins a tie, a NaN never wins), or actions[b,n]
 *                      (its low 8 bits) where r->logits is NULL.
 *   moves[c,n]      += 1 where path[c,k,n] != the previous position (case_start[c,n] for k = 1, else path[c,k-1,n]).
 *   shielded[c,n]   += 1 where the asked action is not 4 (stay) and path[c,k,n] != the previous position + that action's
 *                      delta (0 up (-1,0), 1 left (0,-1), 2 down (1,0), 3 right (0,1); any other id: (0,0)).
 *   steps[c]         = k: the case's last step that was not frozen; -1 = no move of the case was recorded yet.
 *   In either case seen_done[b] = t when !(seen_done[b] > t0) and done[b] != 0: the record that first saw the tenant's
 *   done word set.  The word is never rewound: what a previous tenant left is <= t0 by construction (the record that
 *   stored it ran behind the move in which that tenant ended, and the seat came at that step count or later), and the
 *   comparison with t0 discards it.  Row k - 1 is read for the counters, so the records of a stream come in step order,
 *   each behind its move. */
typedef struct gnnpp_rollout_stream_trace {
    int*         path;       /* [C,T_cap+1,N,2] (row, col); rows relative to the case's seat, row 0 = its starts      */
    signed char* action;     /* [C,T_cap,N] asked actions, -1 = nothing recorded; or NULL                             */
    int*         moves;      /* [C,N] steps at which the agent's position changed; or NULL                            */
    int*         shielded;   /* [C,N] steps at which the agent asked to move and was stopped; or NULL                 */
    int*         steps;      /* [C] the case's last step that was not frozen, -1 = none recorded                      */
    int*         seen_done;  /* [B] per SLOT: 0, or the global step of the record that first saw done[b] set (above)  */
    int          T_cap;      /* rows 0 .. T_cap exist per case                                                        */
} gnnpp_rollout_stream_trace;

/* gnnpp_rollout_stream_trace_begin: once, before the first move: path = 0, action = -1, moves = shielded = 0, steps = -1,
 *     seen_done = 0.
 * gnnpp_rollout_stream_trace_record: the record above for t = r->currentstep, behind the move of that step.
 * gnnpp_rollout_stream_policy_steps_traced: gnnpp_rollout_policy_steps with a streamed record behind each of its nsteps
 *     launches -- the same launches in the same order, enqueued by one call; r->logits is the policy's output and the
 *     record's input.
 *
 * Errors, with nothing enqueued and before any HIP call.  GNNPP_ERR_ARG: r, s or tr NULL; a NULL pointer among r->pos,
 * r->done, r->maxstep, s->slot_case, s->slot_t0, s->case_start, path, steps, seen_done; B <= 0, N < 1, C <= 0, B * N or
 * C * N > 2^31 - 1; T_cap < 1; for a record currentstep < 1 (the traced burst also: nsteps < 1), or both logits and
 * actions NULL while action or shielded is wanted.  GNNPP_ERR_UNSUPPORTED, where gnnpp_rollout_stream_reseat answers it:
 * N > GNNPP_ROLLOUT_MAX_AGENTS, GNNPP_TIE_REPLAY, GNNPP_TIE_MT19937.  The traced burst checks the trace first, then
 * answers what gnnpp_rollout_policy_steps answers. */
int gnnpp_rollout_stream_trace_begin(const gnnpp_rollout* r, const gnnpp_rollout_stream* s,
                                     const gnnpp_rollout_stream_trace* tr, void* stream);
int gnnpp_rollout_stream_trace_record(const gnnpp_rollout* r, const gnnpp_rollout_stream* s,
                                      const gnnpp_rollout_stream_trace* tr, void* stream);
int gnnpp_rollout_stream_policy_steps_traced(const gnnpp_rollout* r, const float* enc_packed, const float* filt_packed,
                                             const float* gf_bias, const float* act_w, const float* act_b, int K,
                                             int nsteps, int precision, const gnnpp_rollout_stream* s,
                                             const gnnpp_rollout_stream_trace* tr, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNPP_ROLLOUT_STREAM_TRACE_H_ */
