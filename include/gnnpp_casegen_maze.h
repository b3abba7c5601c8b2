/* The reference's maze maps drawn on the device, bit for bit -- one entry point of libgnnpp.so, added without a version
 * change (gnnpp_version() stays 330) and kept in a header of its own: gnnpp.h and gnnpp_casegen.h are exactly what they
 * were.  csrc/casegen_maze_kernels.hip; DESIGN.md 5.10.
 *
 * The reference draws every training and test map with CasesGen.mapGen (offlineExpert/CasesGenerator.py): wall segments
 * grown by random walks on the even lattice, on numpy's legacy global stream.  This call states that walk and that stream
 * as a contract and runs it for C maps at once on the caller's stream; its output is the `grid_in` of gnnpp_casegen, which
 * closes the map and draws starts and goals:  gnnpp_casegen_maze -> gnnpp_casegen -> gnnpp_mapf_distances -> ...  is one
 * linear chain of launches, capturable in a HIP graph.  No workspace, no atomics, one writer per output element (two calls
 * give the same bytes).
 *
 * The stream of one map.  MT19937 as np.random.seed(s) leaves it: mt[0] = s, mt[i] = 1812433253 * (mt[i-1] ^ (mt[i-1] >>
 * 30)) + i (uint32), the standard twist of all 624 words before the first word and after every 624th, the standard
 * tempering.  randint(0, high), high exclusive, is numpy's masked rejection on 32-bit words: rng = high - 1; rng == 0
 * gives 0 and draws NO word; otherwise mask = rng with every bit below its top bit set, and words are drawn until
 * (word & mask) <= rng.
 *
 * The walk of one map, all cells free at first, 1 = wall; a cell is (row y, column x).  `walls` times:
 *   1. x = 2 * randint(0, W / 2), then y = 2 * randint(0, H / 2) (integer division): x is drawn first.  Cell (y, x) is set.
 *   2. `steps` times: the neighbours at distance 2 that lie on the map are listed in the order left (x > 1), right
 *      (x < W - 2), up (y > 1), down (y < H - 2); H, W >= 3 give a list of 2 to 4.  One is picked by index
 *      randint(0, len - 1): the high end is exclusive, so the LAST neighbour of the list is never picked, and a list of two
 *      draws no word and takes its first.  If the picked cell is free, it and the cell between are set and the walk moves
 *      there; otherwise nothing changes.  Either way the step is spent.
 * The reference computes walls = int(density * ((H / 2) * (W / 2))) and steps = int(complexity * (5 * (H + W))) in
 * Python floats; the caller passes the two integers (gnn_pathplanning_amd.casegen computes them by those expressions).
 *
 * Map c is drawn from seeds[c], or with seeds == NULL from seed0 + c mod 2^32.  All pointers are device pointers:
 *   grid [C,H,W] uint8      the raw maze, 1 = wall; every byte is written
 *   words [C] or NULL       the number of 32-bit words the map took from its stream
 *
 * Errors, checked in this order before any HIP call, nothing is enqueued on one: grid == NULL, C <= 0, H < 3, W < 3 (the
 * reference itself raises there: randint(0, 0)), walls < 0, steps < 0, walls * steps > 2^31 - 1: GNNPP_ERR_ARG; H or W >
 * GNNPP_MAPF_TEAM_MAX_SIDE: GNNPP_ERR_UNSUPPORTED.  One launch, one wave per map; the time of a map is its seeding (623
 * dependent steps), its refills (one per 624 words) and walls * steps sequential steps. */
#ifndef GNNPP_CASEGEN_MAZE_H_
#define GNNPP_CASEGEN_MAZE_H_

#include "gnnpp.h"

#ifdef __cplusplus
extern "C" {
#endif

int gnnpp_casegen_maze(const unsigned* seeds, unsigned seed0, int C, int H, int W, int walls, int steps,
                       unsigned char* grid, int* words, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNPP_CASEGEN_MAZE_H_ */
