/* Goal distances and planning orders for the MAPF solver of gnnpp.h -- two entry points of libgnnpp.so, added without a
 * version change (gnnpp_version() stays 330) and kept in a header of their own: gnnpp.h, its struct gnnpp_mapf and both
 * solver calls are exactly what they were.  csrc/mapf_distance_kernels.hip; DESIGN.md 5.9.
 *
 * A prioritized planner depends on its planning orders.  These calls compute, on the device and on the caller's stream,
 * what the orders should be built from -- the true shortest-path distance of every agent from its start to its goal on
 * its own map -- and rank planning orders from them, so that `distances -> orders -> gnnpp_mapf_solve /
 * gnnpp_mapf_team_solve` is one linear chain of launches on one stream: no host round trip, no host synchronisation,
 * capturable in a HIP graph together with the solve.  No atomics, one writer per output element (two calls give the same
 * bytes), no workspace. */
#ifndef GNNPP_MAPF_DISTANCE_H_
#define GNNPP_MAPF_DISTANCE_H_

#include "gnnpp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gnnpp_mapf_distances: C cases of N agents on maps of H x W cells (grid [C,H,W] when grid_batched else [H,W], 1 =
 * obstacle; start, goal [C,N,2] (row, col)); all pointers are device pointers.  Every output is written by the call:
 *   dist [C,N]          the length of a shortest 4-connected obstacle-free path from start to goal; other agents are
 *                       ignored.  0 when start == goal; GNNPP_MAPF_DIST_UNREACHABLE when there is no such path;
 *                       GNNPP_MAPF_DIST_INVALID when the start or the goal is off the map or on an obstacle (the other
 *                       agents and cases of the call are unaffected)
 *   lower_makespan [C]  max of the case's distances: no plan of the case has a smaller makespan
 *   lower_flowtime [C]  their sum: no plan has a smaller flowtime.  Both are -1 if any distance of the case is negative.
 * Limits and errors as gnnpp_mapf_team_solve's, checked in its order before any HIP call: a NULL pointer, C <= 0 or
 * N outside 1 .. GNNPP_ROLLOUT_MAX_TEAM, H <= 0, W <= 0, C * N > 2^31 - 1: GNNPP_ERR_ARG; H or W >
 * GNNPP_MAPF_TEAM_MAX_SIDE: GNNPP_ERR_UNSUPPORTED.  Nothing is enqueued on an error.  Two launches. */
#define GNNPP_MAPF_DIST_UNREACHABLE (-1)
#define GNNPP_MAPF_DIST_INVALID     (-2)

int gnnpp_mapf_distances(const unsigned char* grid, int grid_batched, const int* start, const int* goal, int C, int N,
                         int H, int W, int* dist, int* lower_makespan, int* lower_flowtime, void* stream);

/* gnnpp_mapf_orders: order [C,R,N] (device), row (c, r) the permutation of 0 .. N-1 that sorts the agents of case c by
 * rule rules[r] (rules: R values on the HOST, read before the call returns).  dist [C,N] (device) holds the keys of the
 * two distance rules: gnnpp_mapf_distances' output, or any int32 values a caller wants ranked.  Every rule breaks ties
 * by the agent index, ascending, so the ranks are distinct and every slot of `order` is written exactly once.
 *   GNNPP_MAPF_ORDER_INDEX           0, 1, .., N-1
 *   GNNPP_MAPF_ORDER_LONGEST_FIRST   every agent with a NEGATIVE key first (all negative keys rank alike: among
 *                                    themselves these agents stay in index order), then the others by key DESCENDING.
 *                                    A case with an unreachable agent so fails at its first planned agent
 *   GNNPP_MAPF_ORDER_SHORTEST_FIRST  the negative keys first in the same way, then the others by key ASCENDING
 *   GNNPP_MAPF_ORDER_HASHED          by hash ASCENDING, a counter hash of (seed, case c, restart r, agent i), all uint32
 *                                    arithmetic mod 2^32:
 *                                        mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;
 *                                                 x ^= x >> 16
 *                                        hash = mix(seed ^ mix(c * 0x9E3779B9 + r * 0x85EBCA6B + i))
 *                                    -- the counter hash of the simulator's GNNPP_TIE_HASHED (csrc/rollout_kernels.hip,
 *                                    hash_u32), with (case, restart, agent) in the place of (episode, step, call).
 * dist may be NULL when no rule of the call reads it.  NULL rules / order (or dist where a rule needs it), C, R <= 0,
 * N outside 1 .. GNNPP_ROLLOUT_MAX_TEAM, a rule that is none of the four, C * R > 2^31 - 1: GNNPP_ERR_ARG, nothing
 * enqueued.  One workgroup per (case, restart); one launch per 32 restarts. */
#define GNNPP_MAPF_ORDER_INDEX          0
#define GNNPP_MAPF_ORDER_LONGEST_FIRST  1
#define GNNPP_MAPF_ORDER_SHORTEST_FIRST 2
#define GNNPP_MAPF_ORDER_HASHED         3

int gnnpp_mapf_orders(const int* dist, int C, int N, int R, const int* rules, unsigned seed, int* order, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNPP_MAPF_DISTANCE_H_ */
