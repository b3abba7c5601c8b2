/* The trace of a batched rollout, kept on the device: every step's positions, the action every agent asked for, and
 * per-agent counters of moves and of shielded steps -- three entry points of libgnnpp.so, added without a version change
 * (gnnpp_version() stays 330) and kept in a header of their own: gnnpp.h, gnnpp_mapf_distance.h, gnnpp_casegen.h and
 * gnnpp_mapf_audit.h are exactly what they were, and so is every kernel behind them.
 * csrc/rollout_trace_kernels.hip; DESIGN.md 5.11.
 *
 * The reference simulator keeps path_predict and action_predict per agent and writes the predicted schedule to a file
 * (utils/multirobotsim_dcenlocal_onlineExpert.py:732-799).  gnnpp_rollout keeps the current positions only.  A trace is
 * filled by one small launch BEHIND each move: the move leaves `pos` in memory and its argmax inputs (`logits` or
 * `actions`) are still there.  The positions are laid out as the solvers' schedules are ([B,T_cap+1,N,2] int32, the
 * layout of gnnpp_mapf.schedule), so gnnpp_mapf_audit and the sample builders read a trace as it is.  No call here
 * synchronises with the host; every call is capturable in a HIP graph and enqueues nothing on an error.  One thread per
 * (episode, agent), one writer per output element, no atomics: two identical calls give the same bytes. */
#ifndef GNNPP_ROLLOUT_TRACE_H_
#define GNNPP_ROLLOUT_TRACE_H_

#include "gnnpp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HOST struct of DEVICE pointers; B and N are the rollout's.
 *
 * What gnnpp_rollout_trace_record writes behind the move of step t = r->currentstep (1-based, as the move takes it):
 *   path[b,t,n]      = pos[b,n], for every episode, frozen or not: a frozen episode repeats its last state, as the solvers'
 *                      schedules repeat a goal.
 *   An episode that was FROZEN AT ENTRY of that move (below) changes nothing else.  Of every other episode:
 *   action[b,t-1,n]  = the action the agent asked for: the first maximum of logits[n,b,0..4] by exactly the comparison of
 *                      the move kernels (`l[k] > best`: the lowest index wins a tie, a NaN never wins), or actions[b,n]
 *                      (its low 8 bits) where r->logits is NULL.
 *   moves[b,n]      += 1 where path[b,t,n] != path[b,t-1,n].
 *   shielded[b,n]   += 1 where the asked action is not 4 (stay) and path[b,t,n] != path[b,t-1,n] + that action's delta
 *                      (0 up (-1,0), 1 left (0,-1), 2 down (1,0), 3 right (0,1); any other id: (0,0)): the map's edge, an
 *                      obstacle or the collision shield stopped the agent.
 *   steps[b]         = t: the last step at which the episode was not frozen.
 *
 * Frozen at entry.  The move kernels freeze an episode whose done[b] was nonzero BEFORE the call, or that is called with
 * currentstep > maxstep[b].  The record runs after the move and sees done[b] as the move left it; it cannot tell "ended in
 * this call" from "ended earlier".  The trace therefore carries a word of its own, seen_done[b]: 0 as long as no record
 * has seen done[b] set, else the step t of the record that saw it first.  An episode was frozen at entry of move t when
 * 0 < seen_done[b] < t, or t > maxstep[b] (r->done or r->maxstep NULL: that half of the condition never holds).  Row t - 1
 * is read for the counters, so the records of a trace come in step order, t = 1, 2, ..., each behind its move. */
typedef struct gnnpp_rollout_trace {
    int*         path;       /* [B,T_cap+1,N,2] (row, col); row 0 by begin, row t by the record of step t       */
    signed char* action;     /* [B,T_cap,N] asked actions, -1 = nothing recorded; or NULL                        */
    int*         moves;      /* [B,N] steps at which the agent's position changed; or NULL                       */
    int*         shielded;   /* [B,N] steps at which the agent asked to move and was stopped; or NULL            */
    int*         steps;      /* [B] the last step at which the episode was not frozen                            */
    int*         seen_done;  /* [B] 0, or the step of the record that first saw done[b] set (see above)          */
    int          T_cap;      /* rows 0 .. T_cap exist; a record beyond it is refused                             */
} gnnpp_rollout_trace;

/* gnnpp_rollout_trace_begin: path row 0 = r->pos, steps = seen_done = 0, action = -1, moves = shielded = 0.
 * gnnpp_rollout_trace_record: the record above for t = r->currentstep, behind the move of that step.
 * gnnpp_rollout_policy_steps_traced: gnnpp_rollout_policy_steps with a record behind each of its nsteps launches -- the
 *     same launches in the same order, enqueued by one call; r->logits is the policy's output and the record's input.
 *
 * Errors, GNNPP_ERR_ARG with nothing enqueued: r, tr or r->pos NULL, B <= 0, B * N > 2^31 - 1; N outside
 * 1 .. GNNPP_ROLLOUT_MAX_TEAM; path, steps or seen_done NULL; T_cap < 1; for a record currentstep < 1 or currentstep >
 * T_cap (the traced burst: currentstep + nsteps - 1 > T_cap), or both logits and actions NULL while action or shielded
 * is wanted.  The traced burst checks the trace first, then answers what gnnpp_rollout_policy_steps answers. */
int gnnpp_rollout_trace_begin(const gnnpp_rollout* r, const gnnpp_rollout_trace* tr, void* stream);
int gnnpp_rollout_trace_record(const gnnpp_rollout* r, const gnnpp_rollout_trace* tr, void* stream);
int gnnpp_rollout_policy_steps_traced(const gnnpp_rollout* r, const float* enc_packed, const float* filt_packed,
                                      const float* gf_bias, const float* act_w, const float* act_b, int K, int nsteps,
                                      int precision, const gnnpp_rollout_trace* tr, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNPP_ROLLOUT_TRACE_H_ */
