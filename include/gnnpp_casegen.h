/* MAPF cases generated on the device, from a seed to connected maps with start and goal pairs -- one entry point of
 * libgnnpp.so, added without a version change (gnnpp_version() stays 330) and kept in a header of its own: gnnpp.h and
 * gnnpp_mapf_distance.h are exactly what they were.  csrc/casegen_kernels.hip; DESIGN.md 5.10.
 *
 * The reference draws its cases on the host (offlineExpert/CasesGenerator.py): a random map, a flood fill that leaves one
 * connected free region, then start and goal pairs from the free space without duplicates.  This call states that
 * generator as a contract of its own -- counter hashes instead of a sequential random stream, so that a case depends on
 * (seed, case index) alone and a caller can reproduce it -- and runs it for C cases at once on the caller's stream:
 * `gnnpp_casegen -> gnnpp_mapf_distances -> gnnpp_mapf_orders -> gnnpp_mapf_solve / gnnpp_mapf_team_solve` is one linear
 * chain of launches, capturable in a HIP graph.  No workspace, no atomics on global memory, one writer per output element
 * (two calls give the same bytes). */
#ifndef GNNPP_CASEGEN_H_
#define GNNPP_CASEGEN_H_

#include "gnnpp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gnnpp_casegen: C cases of N agents on maps of H x W cells; all pointers are device pointers.  Every output element is
 * written by the call:
 *   grid [C,H,W] uint8       the closed map, 1 = obstacle
 *   start, goal [C,N,2]      (row, col)
 *   cells [C]                the size of the kept free region
 *   status [C]               GNNPP_CASEGEN_OK or GNNPP_CASEGEN_TOO_SMALL
 *
 * The contract.  All arithmetic is uint32 mod 2^32; a cell is named q = row * W + col;
 *     mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *     key(s, c, q) = mix(seed ^ mix(c * 0x9E3779B9 + s * 0x85EBCA6B + q))         stream s, case c, cell q
 * (the counter hash of gnnpp_mapf_distance.h's GNNPP_MAPF_ORDER_HASHED, with (case, stream, cell) in the counter slots).
 * mix is a bijection of the uint32 values, so the keys of one stream of one case are pairwise distinct: the q of the
 * (key, q) orders below states the tie-break of a sort, it never decides.
 *   1. The raw map.  grid_in == NULL: cell q of case c is an obstacle iff key(0, c, q) < obstacle_threshold (0: an empty
 *      map; density d: min(floor(d * 2^32), 2^32 - 1)).  Otherwise the raw map is grid_in, nonzero = obstacle, [C,H,W]
 *      when grid_in_batched else one [H,W] map shared by the cases: the call draws cases on the caller's own maps.
 *   2. Closure.  The largest 4-connected component of free cells is kept; among components of equal size the one that
 *      holds the lowest q.  Every other free cell becomes an obstacle in `grid`.  cells[c] is the kept component's size,
 *      0 on a map without a free cell.
 *   3. cells < N or cells < 2: status = GNNPP_CASEGEN_TOO_SMALL and every start and goal entry of the case is -1; grid
 *      is still the closed map, and the other cases of the call are unaffected.
 *   4. Starts.  The kept cells ranked by (key(1, c, q), q) ascending: the start of agent i is the cell of rank i.
 *   5. Goals.  The kept cells ranked by (key(2, c, q), q) ascending give g_0 .. g_{N-1}; then, for i = 0 .. N-1
 *      ascending, if g_i == start_i, g_i and g_{(i+1) mod N} are exchanged.  N == 1: if g_0 == start_0, the goal is the
 *      cell of rank 1 instead.
 * So the starts of a case are pairwise distinct, its goals are pairwise distinct, no agent starts on its own goal, and
 * every start and goal lies in one connected free region: every agent has a path (gnnpp_mapf_distances >= 1).  A goal may
 * be another agent's start, as in the reference.
 *
 * Limits and errors as gnnpp_mapf_distances', checked in its order before any HIP call: a NULL output pointer, C <= 0,
 * N outside 1 .. GNNPP_ROLLOUT_MAX_TEAM, H <= 0, W <= 0, C * N > 2^31 - 1: GNNPP_ERR_ARG; H or W >
 * GNNPP_MAPF_TEAM_MAX_SIDE: GNNPP_ERR_UNSUPPORTED.  Nothing is enqueued on an error.  grid_in may be NULL.  One launch,
 * one workgroup per case; the time of a case grows with the number of components its raw map holds (one flood each until
 * the cells left cannot outnumber the best component). */
#define GNNPP_CASEGEN_OK        0
#define GNNPP_CASEGEN_TOO_SMALL 1

int gnnpp_casegen(const unsigned char* grid_in, int grid_in_batched, unsigned obstacle_threshold, unsigned seed, int C,
                  int N, int H, int W, unsigned char* grid, int* start, int* goal, int* cells, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNPP_CASEGEN_H_ */
