/* MAPF schedules audited on the device: conflicts, arrivals and costs of any schedule in gnnpp_mapf's layout -- two entry
 * points of libgnnpp.so, added without a version change (gnnpp_version() stays 330) and kept in a header of their own:
 * gnnpp.h, gnnpp_mapf_distance.h and gnnpp_casegen.h are exactly what they were.  csrc/mapf_audit_kernels.hip; DESIGN.md
 * 5.9.
 *
 * gnnpp_schedule_samples flags a move that is none of the five actions and a state off the map or on an obstacle, one
 * agent at a time; nothing looked at two agents at once.  This call does: it says whether a schedule -- the solvers' own,
 * or any other solver's read from a file -- is a legal, collision-free plan that ends on the goals, and it delivers the
 * by-products a search or a report needs: per-agent arrivals, makespan and flowtime, the number of offences per class and
 * the first offence as (t, class, agent, other).  An audit has no dependence between time steps; the call is two launches
 * on the caller's stream, makes no host synchronisation, is capturable in a HIP graph and enqueues nothing on an error.
 * No atomics on global memory, one writer per output element: two calls give the same bytes.  Where several threads of a
 * workgroup store to one LDS word, NO OUTPUT MAY DEPEND ON WHICH OF THE RACING WRITERS WINS: the winner is only ever used
 * to find out THAT a cell is shared, and every value derived from it is the same whoever won. */
#ifndef GNNPP_MAPF_AUDIT_H_
#define GNNPP_MAPF_AUDIT_H_

#include "gnnpp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gnnpp_mapf_audit: C cases of N agents on maps of H x W cells, schedules of T_max + 1 rows; all pointers are device
 * pointers.
 *   grid [C,H,W] uint8 when grid_batched, else one [H,W] map shared by the cases; 1 (nonzero) = obstacle
 *   start [C,N,2] (row, col), or NULL: no start check
 *   goal [C,N,2]
 *   schedule [C,T_max+1,N,2] int32, the layout of gnnpp_mapf.schedule: row t holds the agents' positions at time t
 *   steps [C] int32, or NULL.  L_c = steps[c] is the last row of case c that counts; rows beyond it are never read.
 *       NULL: L_c = T_max for every case.  steps[c] < 0: the case is skipped -- status GNNPP_MAPF_AUDIT_SKIPPED, every
 *       other output element of the case -1 (a solver's `makespan` can be passed as it is: -1 for an unsolved case).
 *       steps[c] > T_max is clamped to T_max.
 *
 * The classes of offence, per time step, in the order they are examined; an earlier class shields the later ones:
 *   STATE   layer t:  every agent off the map or on an obstacle.  A layer with a STATE flag is not examined for VERTEX.
 *   VERTEX  layer t, t = 0 included:  every agent that shares its cell with another agent.
 *   MOVE    transition t -> t + 1, t < L_c, examined only when the layers t and t + 1 hold neither STATE nor VERTEX flags:
 *           every agent whose displacement is none of up, left, down, right, stop.
 *   SWAP    the same transition, examined only when MOVE was and flagged nobody:  agent i if it moves and some j != i has
 *           pos_t[j] = pos_{t+1}[i] and pos_{t+1}[j] = pos_t[i].
 * Following into a cell vacated in the same step is no conflict, and neither is a rotation of three or more agents: the
 * rule of gnnpp.h's solver contract and of the simulator.
 *
 * Outputs; every element is written by the call:
 *   status [C]      the OR of the class bits of all steps, GNNPP_MAPF_AUDIT_BAD_START (start given and pos_0 != start for
 *                   some agent), GNNPP_MAPF_AUDIT_NOT_AT_GOAL (some agent is not on its goal at L_c) and
 *                   GNNPP_MAPF_AUDIT_SKIPPED.  0: a legal, collision-free plan that ends on the goals.
 *   arrival [C,N]   the smallest t with pos_s[i] = goal[i] for all s in t .. L_c; -1 if agent i is not on its goal at L_c
 *   makespan, flowtime [C]   the max and the sum of the case's arrivals; -1 if any arrival is -1
 *   counts [C,4]    the number of flagged (step, agent) pairs per class, in the class order GNNPP_MAPF_AUDIT_CLASS_*
 *   first [C,4]     (t, class, agent, other): the flagged pair with the smallest t, then the class order above, then the
 *                   smallest agent; class is GNNPP_MAPF_AUDIT_CLASS_*; other is the smallest j != agent on the same cell
 *                   (VERTEX) or swapping with it (SWAP), else -1.  All four are -1 when nothing is flagged.
 *
 * GNNPP_MAPF_AUDIT_CHUNK is the number of transitions one work item covers, published so that tests can put offences on
 * the seams between items.  No output depends on it.
 *
 * Limits and errors, checked in this order before any HIP call: C <= 0, N outside 1 .. GNNPP_ROLLOUT_MAX_TEAM, H <= 0,
 * W <= 0: GNNPP_ERR_ARG; H or W > GNNPP_MAPF_TEAM_MAX_SIDE: GNNPP_ERR_UNSUPPORTED; T_max outside
 * 0 .. GNNPP_MAPF_TEAM_MAX_STEPS, or more than 2^31 - 1 work items (C (T_max / GNNPP_MAPF_AUDIT_CHUNK + 1)):
 * GNNPP_ERR_ARG; a NULL pointer other than start and steps: GNNPP_ERR_ARG; workspace_bytes below
 * gnnpp_mapf_audit_workspace_bytes(C, N, T_max): GNNPP_ERR_ARG.  gnnpp_mapf_audit_workspace_bytes returns 0 for sizes the
 * call refuses.  The workspace needs no initialisation and holds nothing between calls. */
#define GNNPP_MAPF_AUDIT_CHUNK        32

#define GNNPP_MAPF_AUDIT_CLASS_STATE  0
#define GNNPP_MAPF_AUDIT_CLASS_VERTEX 1
#define GNNPP_MAPF_AUDIT_CLASS_MOVE   2
#define GNNPP_MAPF_AUDIT_CLASS_SWAP   3

#define GNNPP_MAPF_AUDIT_STATE        1
#define GNNPP_MAPF_AUDIT_VERTEX       2
#define GNNPP_MAPF_AUDIT_MOVE         4
#define GNNPP_MAPF_AUDIT_SWAP         8
#define GNNPP_MAPF_AUDIT_BAD_START    16
#define GNNPP_MAPF_AUDIT_NOT_AT_GOAL  32
#define GNNPP_MAPF_AUDIT_SKIPPED      64

size_t gnnpp_mapf_audit_workspace_bytes(int C, int N, int T_max);

int gnnpp_mapf_audit(const unsigned char* grid, int grid_batched, const int* start, const int* goal, const int* schedule,
                     const int* steps, int C, int N, int H, int W, int T_max, int* status, int* arrival, int* makespan,
                     int* flowtime, int* counts, int* first, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNPP_MAPF_AUDIT_H_ */
