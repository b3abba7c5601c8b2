/* Streamed rollouts of large teams: the slots of include/gnnpp_rollout_stream.h for GNNPP_ROLLOUT_MAX_AGENTS < N <=
 * GNNPP_ROLLOUT_MAX_TEAM agents, on the dense graph or on the team filter's neighbour lists -- two entry points of
 * libgnnpp.so, added without a version change (gnnpp_version() stays 330) and kept in a header of their own: gnnpp.h and the
 * other companion headers are exactly what they were, and so is every entry point behind them.
 * csrc/rollout_team_stream_kernels.hip; DESIGN.md 5.14.
 *
 * The stream is the one of gnnpp_rollout_stream.h: the same struct gnnpp_rollout_stream, the same meaning of `now`, the same
 * per-case result tables with step records relative to the seat, the same prefix rule of seating.  A reseat is three
 * launches on the caller's stream:
 *   1. assign        as in gnnpp_rollout_stream_reseat (the same kernel).
 *   2. harvest_seat  one workgroup of one thread per agent per slot: the table writes and the seat of
 *                    gnnpp_rollout_stream_reseat; the seat then builds the slot's step-0 graph with the radius search of
 *                    step 0 (grow = 1), from the slot's own memory:
 *                        lists == NULL   S[b], radius[b], connected[b]        as gnnpp_rollout_gso does for the case alone
 *                        lists != NULL   columns [b * N, (b + 1) * N) of the lists block (the layout gnnpp_rollout_lists
 *                                        writes for B graphs), radius[b], connected[b]   as gnnpp_rollout_lists does
 *   3. seat_observe  obs[b] of every slot seated by this reseat (assign[b] >= 0), as gnnpp_rollout_observe does.
 * A seated slot holds, bit for bit, what those calls give for its case alone; a slot the reseat did not seat keeps its bytes.
 * No launch uses an atomic or reads anything on the host; all three are capturable in a HIP graph; one writer per word.
 *
 * Scope: GNNPP_ROLLOUT_MAX_AGENTS < N <= GNNPP_ROLLOUT_MAX_TEAM, H * W <= GNNPP_ROLLOUT_TEAM_MAX_CELLS, tie modes
 * GNNPP_TIE_LOWEST and GNNPP_TIE_HASHED (hashed from (seed, slot, global step), as in gnnpp_rollout_stream.h).  Teams of up
 * to GNNPP_ROLLOUT_MAX_AGENTS agents are streamed by gnnpp_rollout_stream_begin / gnnpp_rollout_stream_reseat.  The per-case
 * trace (gnnpp_rollout_stream_trace.h) does not cover these teams yet. */
#ifndef GNNPP_ROLLOUT_TEAM_STREAM_H_
#define GNNPP_ROLLOUT_TEAM_STREAM_H_

#include "gnnpp_rollout_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gnnpp_rollout_team_stream_begin: what gnnpp_rollout_stream_begin does (the same launch).
 * gnnpp_rollout_team_stream_reseat: the three launches above at step count `now`.  lists == NULL: the dense form, r->S is
 *     required (lists_bytes is ignored).  lists != NULL: the lists form, a 16-byte aligned block of lists_bytes >=
 *     gnnpp_team_lists_bytes(B, N) bytes; r->S may be NULL and is not touched.
 *
 * Errors, with nothing enqueued and before any HIP call.  GNNPP_ERR_ARG: everything gnnpp_rollout_stream_reseat answers
 * with it (r->S only in the dense form); a lists block that is misaligned or too small (checked for N <=
 * GNNPP_ROLLOUT_MAX_TEAM).  Then GNNPP_ERR_UNSUPPORTED: N <= GNNPP_ROLLOUT_MAX_AGENTS (call gnnpp_rollout_stream_reseat),
 * N > GNNPP_ROLLOUT_MAX_TEAM, H * W > GNNPP_ROLLOUT_TEAM_MAX_CELLS, GNNPP_TIE_REPLAY, GNNPP_TIE_MT19937. */
int gnnpp_rollout_team_stream_begin(const gnnpp_rollout* r, const gnnpp_rollout_stream* s, void* stream);
int gnnpp_rollout_team_stream_reseat(const gnnpp_rollout* r, const gnnpp_rollout_stream* s, int now, void* lists,
                                     size_t lists_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNPP_ROLLOUT_TEAM_STREAM_H_ */
