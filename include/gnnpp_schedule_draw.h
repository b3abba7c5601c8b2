/* A training batch drawn straight from expert schedules -- two entry points of libgnnpp.so, added without a version
 * change (gnnpp_version() stays 330) and kept in a header of their own: gnnpp.h and its companions are exactly what they
 * were.  csrc/schedule_draw_kernels.hip; DESIGN.md 5.8.
 *
 * gnnpp_schedule_samples, gnnpp_schedule_team_samples and gnnpp_schedule_team_fill_lists materialise every step of every
 * schedule: 1 452 bytes of observation per agent and step, plus the graph.  Those tensors are a pure function of the
 * step's positions (8 bytes per agent) and of three things held once per case: the map, the goals and the radius the
 * case's graphs were built with.  A pool that keeps the schedules and builds a batch when it is drawn holds two orders
 * of magnitude less.  This call is that draw: B picked steps in, the batch training takes out, nothing in between.
 *
 * What is read.  Of the gnnpp_schedules struct (gnnpp.h; HOST struct of DEVICE pointers): grid, grid_batched, goal, pos,
 * case_start, C, N, H, W, T_total as every schedule call reads them, and radius [C] and status [C], which are INPUTS here:
 * what gnnpp_schedule_team_plan (or either sample call) wrote for these cases.  radius0 and the fields that are outputs of
 * the sample calls -- obs, S, S64, target, growth, step_info -- are ignored and may be NULL.  index [B]: int32, device;
 * each entry a step in [0, T_total).  Indices may repeat; an index outside [0, T_total) is CLAMPED into it, as
 * gnnpp_team_lists_gather clamps (never an out-of-range read).
 *
 * What is written, for pick b with t = index[b] (clamped) and c the case that owns step t:
 *   obs[b]     [N,3,11,11] fp32  the observation of pos[t] on grid[c] with goal[c]
 *   target[b]  [N,5] fp32        one-hot of pos[t+1] - pos[t] in the order [-1,0] [0,-1] [1,0] [0,1] [0,0]; the next state
 *                                of a case's last step is the goal
 *   the graph of pos[t] under radius[c] -- the case's FINAL radius, never radius0, never a radius of the step's own --
 *   in ONE of two forms, exactly one of S and lists non-NULL:
 *   S[b]       [N,N] fp32        (float)((s_i * A_ij) * s_j), s = sqrt(1.0 / deg) in fp64
 *   lists                        graph b of a standard lists block of B graphs of N nodes (gnnpp.h "Neighbour lists as
 *                                an INPUT format": gnnpp_team_lists_bytes(B, N) bytes, 16-byte aligned): cnt and the first
 *                                roundup4(cnt) entries of every column, rows ascending, (0, 0.0f) up to the multiple of
 *                                four; entries behind that are not written
 * Every written row is BYTE FOR BYTE what the existing calls produce for step t: obs, target and S of
 * gnnpp_schedule_samples / gnnpp_schedule_team_samples, and the block gnnpp_team_lists_gather makes of the set of
 * gnnpp_schedule_team_fill_lists.  Equality, not a tolerance: the work is integers, {0, 1} values and fp64 products in
 * a fixed order, and the device functions are the very ones those calls run.
 * A pick whose case has status[c] != 0 writes zeros everywhere -- obs[b], target[b], S[b], or cnt = 0 for every column
 * of graph b -- so a caller that ignores status still gets a defined batch.  Every other pick is unaffected.
 *
 * Limits: 2 <= N <= GNNPP_ROLLOUT_MAX_TEAM, one contract and one route for every team size; H * W <=
 * GNNPP_ROLLOUT_TEAM_MAX_CELLS (the case's occupancy grid lives in LDS).  Outputs are indexed in size_t.  When N % 4 == 0
 * and S is 16-byte aligned the graph is stored 16 bytes per lane; any other 4-byte alignment gives the same bytes.
 * workspace: device memory, no initial contents, gnnpp_schedule_draw_workspace_bytes(N, B) bytes, 8-byte aligned: s of
 * every agent of every pick in fp64 ([B, N]), the hand-over from the degree launch to the graph launch.
 *
 * Errors; every check comes before any HIP call and nothing is enqueued on one.
 *   GNNPP_ERR_ARG          s, one of the pointers read above, index, obs, target or workspace NULL; obs, target, S or index
 *                          not 4-byte, radius or workspace not 8-byte, lists not 16-byte aligned; C, T_total, H, W or
 *                          N <= 0, C > T_total; B <= 0; both or neither of S and lists; lists_bytes <
 *                          gnnpp_team_lists_bytes(B, N); workspace_bytes < gnnpp_schedule_draw_workspace_bytes(N, B);
 *                          N > GNNPP_ROLLOUT_MAX_TEAM
 *   GNNPP_ERR_UNSUPPORTED  N == 1 (a graph of one node: deg = 0, the reference divides by it); H * W >
 *                          GNNPP_ROLLOUT_TEAM_MAX_CELLS; more workgroups than a grid dimension holds (B * ceil(N / 16) >
 *                          2^31 - 1)
 *
 * THREE launches on `stream` (degrees and targets; the graph in the form asked for; observations), against the five of
 * gnnpp_schedule_team_samples: the scan and the case launch are the plan's, run once when the cases were stored.  No
 * atomics, one writer per element (two calls give the same bytes), no host synchronisation, capturable in a HIP graph
 * as a single chain. */
#ifndef GNNPP_SCHEDULE_DRAW_H_
#define GNNPP_SCHEDULE_DRAW_H_

#include "gnnpp.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t gnnpp_schedule_draw_workspace_bytes(int N, int B);   /* 0 on invalid arguments */
int gnnpp_schedule_draw(const gnnpp_schedules* s, const int* index, int B, float* obs, float* target, float* S,
                        void* lists, size_t lists_bytes, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNPP_SCHEDULE_DRAW_H_ */
