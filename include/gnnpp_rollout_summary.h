/* The summary of a rollout's per-case result tables: the numbers the reference reports for every validation and test run
 * (utils/metrics.py, MonitoringMultiAgentPerformance), reduced on the device -- two entry points of libgnnpp.so, added
 * without a version change (gnnpp_version() stays 330) and kept in a header of their own: gnnpp.h and the other companion
 * headers are exactly what they were, and so is every entry point behind them.
 * csrc/rollout_summary_kernels.hip; DESIGN.md 5.15.
 *
 * One launch on the caller's stream: one workgroup of 256 threads per group.  The tables are read where a rollout left
 * them (BatchedRollout with C = B, gnnpp_rollout_stream's per-case tables): reached [C,N] (an agent reached when its word
 * is > 0), stats [C,2] = (makespan, flowtime).  The expert's costs are element c of target_makespan / target_flowtime at
 * [c * target_stride]: two arrays of their own (stride 1), or the two columns of one int32 [C,2] table (stride 2,
 * target_flowtime = target_makespan + 1).
 *
 * Which cases count.  valid == NULL: every case; else the cases with valid[c] != 0 (a stream's caller passes lived[c] >= 0:
 * an unfinished case holds no result).  group == NULL: one group (G must be 1); else group[c] in 0 .. G - 1 names the
 * case's group.  A valid case whose group id lies outside that range is counted in n_bad_group of group 0 and in nothing
 * else.  In what follows "case" means a valid case of the group.
 *
 * A case is DEGENERATE when its target_makespan or its target_flowtime is <= 0 (every start already on its goal; an
 * unsolved target): it is counted in n, in the reach counts, in n_optimal by the rule below and in n_degenerate, and it is
 * left out of both deterioration rates, whose divisor is m = n - n_degenerate, and out of the four cost sums.
 *
 * The record of group g, in `out` (8-byte aligned, gnnpp_rollout_summary_out_bytes(N, G) bytes):
 *   out_i64 [G,GNNPP_SUMMARY_I64]  long long, at byte 0
 *     GNNPP_SUMMARY_N                 cases
 *     GNNPP_SUMMARY_N_REACH_ALL       ... in which every agent reached
 *     GNNPP_SUMMARY_N_OPTIMAL         ... in which every agent reached and makespan <= target_makespan and flowtime <=
 *                                     target_flowtime
 *     GNNPP_SUMMARY_AGENTS_REACHED    agents that reached, summed over the cases
 *     GNNPP_SUMMARY_N_DEGENERATE      degenerate cases
 *     GNNPP_SUMMARY_N_BAD_GROUP       group 0: valid cases with a group id outside 0 .. G - 1; other groups: 0
 *     GNNPP_SUMMARY_SUM_MP_PRED, _SUM_MP_TARGET, _SUM_FT_PRED, _SUM_FT_TARGET   makespan, target_makespan, flowtime,
 *                                     target_flowtime summed over the cases that are not degenerate
 *     GNNPP_SUMMARY_MIN_REACHED, _MAX_REACHED   fewest / most agents that reached in one case; -1 when n == 0
 *     GNNPP_SUMMARY_N_FAIL_SHIELDED   shielded != NULL: cases in which NOT every agent reached and some agent a with
 *                                     reached[c][a] <= 0 has shielded[c][a] > 0 -- an agent that did not arrive was, at
 *                                     least once, stopped where it asked to move.  The reference's
 *                                     noReachGoalbyCollsionShielding (step limit hit, not all arrived, a collision was
 *                                     predicted and shielded at some step, by any agent) restated on the trace's counters,
 *                                     which also count a move stopped by the map's edge or an obstacle.  shielded == NULL: -1
 *     GNNPP_SUMMARY_N_COLLISION_FREE  audit_ok != NULL: cases with audit_ok[c] != 0; audit_ok == NULL: -1
 *     GNNPP_SUMMARY_N_SHIELDED        shielded != NULL: cases in which some agent has shielded[c][a] > 0 (the reference's
 *                                     check_CollisionPredictedinLoop on the same counters); shielded == NULL: -1
 *     word 15                         0
 *   out_f64 [G,GNNPP_SUMMARY_F64]  double, at byte G * GNNPP_SUMMARY_I64 * 8
 *     GNNPP_SUMMARY_RATE_REACH        n_reach_all / n; NaN when n == 0
 *     GNNPP_SUMMARY_AVG_DMP, _STD_DMP mean and sample standard deviation (divisor m - 1) over the m cases that are not
 *                                     degenerate of |makespan - target_makespan| / target_makespan, in double as the
 *                                     reference's update() forms it; the mean is NaN when m == 0, the deviation when m < 2
 *     GNNPP_SUMMARY_AVG_DFT, _STD_DFT the same of the flowtime
 *     GNNPP_SUMMARY_MEAN_REACHED      agents_reached / n; NaN when n == 0
 *     GNNPP_SUMMARY_M2_DMP, _M2_DFT   the sums of squared differences from the two means (0 when m == 0): with n,
 *                                     n_degenerate and the means, what two records need to be merged exactly
 *   hist [G,N+1]  int, at byte G * (GNNPP_SUMMARY_I64 + GNNPP_SUMMARY_F64) * 8: cases per count of agents that reached
 *
 * Order of the arithmetic, fixed: a thread takes the cases tid, tid + 256, ... in that order; its partial results are
 * reduced over its wave by a butterfly, then the four waves' results are added in wave order through LDS.  Counts and sums
 * of integers are long long; the rates are reduced in double and in two passes, the means first, then the squared
 * differences from them, which makes the deviation what numpy's std(ddof=1) computes up to the order of summation.  No
 * atomics, one writer per word of `out`: two identical calls give identical bytes.  Nothing is read on the host; the
 * launch is capturable in a HIP graph; offsets are 64-bit.  end_step is not needed. */
#ifndef GNNPP_ROLLOUT_SUMMARY_H_
#define GNNPP_ROLLOUT_SUMMARY_H_

#include "gnnpp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GNNPP_SUMMARY_MAX_GROUPS 64
#define GNNPP_SUMMARY_I64 16
#define GNNPP_SUMMARY_F64 8

#define GNNPP_SUMMARY_N 0
#define GNNPP_SUMMARY_N_REACH_ALL 1
#define GNNPP_SUMMARY_N_OPTIMAL 2
#define GNNPP_SUMMARY_AGENTS_REACHED 3
#define GNNPP_SUMMARY_N_DEGENERATE 4
#define GNNPP_SUMMARY_N_BAD_GROUP 5
#define GNNPP_SUMMARY_SUM_MP_PRED 6
#define GNNPP_SUMMARY_SUM_MP_TARGET 7
#define GNNPP_SUMMARY_SUM_FT_PRED 8
#define GNNPP_SUMMARY_SUM_FT_TARGET 9
#define GNNPP_SUMMARY_MIN_REACHED 10
#define GNNPP_SUMMARY_MAX_REACHED 11
#define GNNPP_SUMMARY_N_FAIL_SHIELDED 12
#define GNNPP_SUMMARY_N_COLLISION_FREE 13
#define GNNPP_SUMMARY_N_SHIELDED 14

#define GNNPP_SUMMARY_RATE_REACH 0
#define GNNPP_SUMMARY_AVG_DMP 1
#define GNNPP_SUMMARY_STD_DMP 2
#define GNNPP_SUMMARY_AVG_DFT 3
#define GNNPP_SUMMARY_STD_DFT 4
#define GNNPP_SUMMARY_MEAN_REACHED 5
#define GNNPP_SUMMARY_M2_DMP 6
#define GNNPP_SUMMARY_M2_DFT 7

typedef struct gnnpp_rollout_summary_in {
    const int* reached;              /* [C,N]  > 0: the agent reached its goal */
    const int* stats;                /* [C,2]  makespan, flowtime */
    const int* target_makespan;      /* element c at [c * target_stride] */
    const int* target_flowtime;      /* element c at [c * target_stride] */
    const int* valid;                /* [C] or NULL */
    const int* group;                /* [C] or NULL (one group) */
    const int* shielded;             /* [C,N] or NULL: a trace's table */
    const int* audit_ok;             /* [C] or NULL: != 0 where the case's schedule has no offence */
    int C, N, G;
    int target_stride;               /* >= 1 */
} gnnpp_rollout_summary_in;

/* gnnpp_rollout_summary_out_bytes: the size of `out` for teams of N agents in G groups; 0 when N < 1, G < 1 or G >
 *     GNNPP_SUMMARY_MAX_GROUPS.
 * gnnpp_rollout_summary: the launch above.
 *
 * Errors, with nothing enqueued and before any HIP call.  GNNPP_ERR_ARG: in, out, reached, stats, target_makespan or
 * target_flowtime NULL; C <= 0, N < 1, G < 1, G > GNNPP_SUMMARY_MAX_GROUPS, target_stride < 1; group NULL with G != 1;
 * C * N > 2^31 - 1; out not 8-byte aligned. */
size_t gnnpp_rollout_summary_out_bytes(int N, int G);
int gnnpp_rollout_summary(const gnnpp_rollout_summary_in* in, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNPP_ROLLOUT_SUMMARY_H_ */
