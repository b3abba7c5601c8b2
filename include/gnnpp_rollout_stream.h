/* Streamed rollouts: B episode slots stay resident and a slot whose episode has ended is refilled from a queue of C cases,
 * on the device, between two steps -- two entry points of libgnnpp.so, added without a version change (gnnpp_version()
 * stays 330) and kept in a header of their own: gnnpp.h and the other companion headers are exactly what they were, and so
 * is every kernel behind them.  csrc/rollout_stream_kernels.hip; DESIGN.md 5.12.
 *
 * A batched rollout steps until its slowest episode ends, and a frozen episode still costs its share of every launch.
 * Here the rollout `r` (include/gnnpp.h) is a set of B SLOTS with one global step count: `now` is the number of moves taken
 * so far, and the next move runs with r->currentstep = now + 1.  A reseat between two moves
 *   1. assign        one workgroup: scans done[0..B) in slot order; the k-th slot whose done[b] != 0 gets case cursor + k
 *                    while that is < C, else -1; writes assign[b] (-1 for a slot that is not done) and advances cursor.  A
 *                    prefix count in slot order: two runs seat the same cases in the same slots.
 *   2. harvest_seat  one workgroup per slot; a slot that is not done, or is empty and gets no case, is left untouched.
 *        harvest     (done[b] != 0 and slot_case[b] = c >= 0) writes row c of the result tables, step records RELATIVE to
 *                    t0 = slot_t0[b], the step count at which the case was seated:
 *                        start_step[c,n] = s >= t0 ? s - t0 : (s < 0 ? -1 : 0)       s = r->start_step[b,n]
 *                        end_step[c,n]   = e < 0 ? -1 : e - t0                      e = r->end_step[b,n]
 *                    (the move kernels write start_step = 0, in global steps, for an agent that never asked to move and had
 *                    not arrived at the limit: relative step 0 in any slot), stats[c] = (makespan, flowtime) recomputed from
 *                    the relative records by the move kernels' formula (max end - min start, sum of end - start, a missing
 *                    start counted as 0; r->stats is not read), reached, pos and radius as they stand,
 *                    lived[c] = min(max end + 1, case_maxstep[c]): the moves that did not find the episode frozen,
 *                    slot[c] = b and t0[c].
 *        seat        (assign[b] = c >= 0) copies the case into the slot -- its map into row b of slot_grid when maps are per
 *                    case, pos <- case_start[c], goal <- case_goal[c] -- and resets the episode: reached = 0, start_step =
 *                    end_step = -1, flags = stats = done = 0 (choice_count too, when given), maxstep[b] = now +
 *                    case_maxstep[c], radius[b] = commR; then builds the slot's step-0 state exactly as gnnpp_rollout_observe
 *                    and gnnpp_rollout_gso with grow = 1 do (the same device functions): radius[b], connected[b], S[b],
 *                    obs[b].  slot_case[b] = c, slot_t0[b] = now.
 *                    A harvested slot that gets no case keeps done[b] = 1 and becomes empty (slot_case[b] = -1).
 * Neither launch uses an atomic or reads anything on the host; both are capturable in a HIP graph; one writer per word.
 *
 * Scope: 1 <= N <= GNNPP_ROLLOUT_MAX_AGENTS, the dense graph (r->S), tie modes GNNPP_TIE_LOWEST and GNNPP_TIE_HASHED.  The
 * hashed rule draws from (seed, slot, global step), i.e. a different -- equally arbitrary -- stream than a plain rollout of
 * the same case.  GNNPP_TIE_REPLAY and GNNPP_TIE_MT19937 keep per-episode state that a seat would have to rewind and are
 * refused.  Map limit: that of gnnpp_rollout_gso_observe (H * W <= 65 536 cells). */
#ifndef GNNPP_ROLLOUT_STREAM_H_
#define GNNPP_ROLLOUT_STREAM_H_

#include "gnnpp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HOST struct of DEVICE pointers; B, N, H and W are the rollout's. */
typedef struct gnnpp_rollout_stream {
    /* the case queue (read only) */
    const unsigned char* case_grid;  /* [C,H,W] when case_grid_batched, else the one shared map [H,W] = r->grid */
    int          case_grid_batched;
    const int*   case_start;    /* [C,N,2] (row, col)                                                           */
    const int*   case_goal;     /* [C,N,2]                                                                      */
    const int*   case_maxstep;  /* [C] each case's own step limit, >= 1                                         */
    int          C;
    double       commR;         /* every case's communication radius at its step 0                              */
    /* the slots */
    int*         cursor;        /* [1] the next case of the queue                                               */
    int*         slot_case;     /* [B] the case a slot holds, -1 = empty                                        */
    int*         slot_t0;       /* [B] the step count at which that case was seated                             */
    int*         assign;        /* [B] what the last reseat gave the slot: a case, or -1                        */
    unsigned char* slot_grid;   /* the rollout's map rows, writable: r->grid when case_grid_batched, else unused */
    int*         goal;          /* [B,N,2] r->goal, writable                                                    */
    int*         maxstep;       /* [B] r->maxstep, writable                                                     */
    /* result tables, one row per CASE; -1 until the case is harvested */
    int*         reached;       /* [C,N] 0/1                                                                    */
    int*         start_step;    /* [C,N] relative to the seat, -1 = never asked to move                         */
    int*         end_step;      /* [C,N] relative to the seat                                                   */
    int*         pos;           /* [C,N,2] final positions                                                      */
    double*      radius;        /* [C] the radius the case's step 0 grew                                        */
    int*         stats;         /* [C,2] makespan, flowtime                                                     */
    int*         lived;         /* [C] moves that did not find the episode frozen                               */
    int*         slot;          /* [C] the slot the case ran in                                                 */
    int*         t0;            /* [C] the step count at which it was seated                                    */
} gnnpp_rollout_stream;

/* gnnpp_rollout_stream_begin: done[b] = 1, slot_case[b] = assign[b] = -1, slot_t0[b] = 0 for every slot (all empty),
 *     cursor = 0, every result table = -1 (radius: -1.0).  One launch.
 * gnnpp_rollout_stream_reseat: the two launches above at step count `now`.
 *
 * Errors, with nothing enqueued and before any HIP call.  GNNPP_ERR_ARG: r or s NULL; B <= 0, N < 1, H or W <= 0, C <= 0;
 * a NULL pointer among r->pos, done and (reseat) grid, goal, obs, radius, S, reached, start_step, end_step, maxstep, flags,
 * stats, or among the fields of s (slot_grid only when case_grid_batched); r->grid_batched != case_grid_batched; slot_grid
 * != r->grid when case_grid_batched, case_grid != r->grid when not; s->goal != r->goal or s->maxstep != r->maxstep; commR
 * not a positive finite number; now outside 0 .. 2^30; a tie mode outside 0 .. 3.  GNNPP_ERR_UNSUPPORTED: N >
 * GNNPP_ROLLOUT_MAX_AGENTS, H * W > 65 536, GNNPP_TIE_REPLAY, GNNPP_TIE_MT19937. */
int gnnpp_rollout_stream_begin(const gnnpp_rollout* r, const gnnpp_rollout_stream* s, void* stream);
int gnnpp_rollout_stream_reseat(const gnnpp_rollout* r, const gnnpp_rollout_stream* s, int now, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNPP_ROLLOUT_STREAM_H_ */
