// Prioritized planning of MAPF cases: the reference's SIPP expert option
// (offlineExpert/CasesSolver.py:517-539 runs a prebuilt `mapf_prioritized_sipp`), restated as a bit-parallel
// breadth-first search over time.  The contract (include/gnnpp.h, gnnpp_mapf) in short: agents are planned one
// after another in a given order; each plans against the finished plans of the agents before it, parked agents
// included; R_0 = {start}, R_{t+1} = free cells no earlier agent holds at t+1, reached from R_t by a stop or by a move
// that is not a swap; arrival a = the first t >= t_min with the goal in R_t (t_min = 1 + the last time an earlier agent
// holds the goal); the path is walked back from (goal, a) taking the first predecessor in the order stop, entered by
// up, left, down, right.
//
// One WAVE per (case, restart) item, one map row per lane: row x of a bitset is the 64-bit word of lane x (H, W <=
// 64), bit y = column y.  Horizontal moves are shifts, vertical moves read the neighbouring lane's word through LDS.
// A persistent grid of at most kMapfSlots workgroups strides over the items; each workgroup owns one workspace slot
// (global memory) holding, per time step t = 0 .. T_max, six planes of H words:
//
//   plane 0      occupancy of the agents planned so far at t (parked agents until T_max)
//   plane 1 + e  cells whose occupant moves in direction e (up, left, down, right) between t and t + 1: entering cell
//                a by direction d is a swap exactly when a's occupant moves by -d, so these planes are the swap blocks
//                indexed by the TARGET cell
//   plane 5      the reachable layer R_t of the agent being planned (the walk back reads it)
//
// Launches on one stream, no atomics, every output written by one work-item:
//   mapf_plan_kernel (pass 0)  every (case, restart): summary (status, flowtime, makespan, failing agent) -> workspace;
//                              with R = 1 also the schedule and the arrivals
//   mapf_select_kernel         one thread per case: the best restart -> makespan / flowtime / status / failing / restart
//   mapf_plan_kernel (pass 1)  R > 1 only: the chosen restart of every case again, now writing schedule and arrivals
// Memory is slots x slot size, independent of C x R; the price of R > 1 is one more plan per case.
#include "../../include/gnnpp.h"
#include "gnnpp_common.h"

namespace gnnpp {

struct MapfArgs : ::gnnpp_mapf {
    int* summary_ws;                            // [C,R,4] status, flowtime, makespan, failing agent of every item
    unsigned long long* slots_ws;               // [slots][T_max + 1][kMapfPlanes][H]
};

constexpr int kMapfSlots = 512;                 // persistent workgroups at most (= workspace slots)
constexpr int kMapfPlanes = 6;                  // per time step: occupancy, 4 move planes, reachable layer
constexpr int kMapfReach = 5;
// LDS: rows [2][64] u64 (double-buffered neighbour exchange) | path [GNNPP_MAPF_MAX_STEPS + 1] int | arrival [128] int
constexpr size_t kMapfLdsBytes = 2 * 64 * 8 + (GNNPP_MAPF_MAX_STEPS + 1) * 4 + GNNPP_ROLLOUT_MAX_AGENTS * 4;

inline size_t mapf_summary_bytes(long long items) { return ((size_t)items * 4 * sizeof(int) + 255) & ~(size_t)255; }
__host__ __device__ inline size_t mapf_slot_words(int H, int T) { return (size_t)(T + 1) * kMapfPlanes * H; }
inline int mapf_slots(long long items) { return items < kMapfSlots ? (int)items : kMapfSlots; }
inline size_t mapf_workspace_bytes(int C, int R, int H, int T) {
    const long long items = (long long)C * R;
    return mapf_summary_bytes(items) + (size_t)mapf_slots(items) * mapf_slot_words(H, T) * sizeof(unsigned long long);
}

// word of plane `plane`, row x, time t in a slot
__device__ __forceinline__ size_t mapf_word(int H, int t, int plane, int x) {
    return ((size_t)t * kMapfPlanes + plane) * H + x;
}

// starts and goals on the map and free, no two starts / goals alike, the order a permutation of 0 .. N-1 (wave-uniform)
__device__ bool mapf_case_valid(const MapfArgs& p, const unsigned char* grid, const int* st, const int* gl,
                                const int* ord, int lane) {
    const int N = p.N, H = p.H, W = p.W;
    bool bad = false;
    for (int n = lane; n < N; n += 64) {
        const int sx = st[2 * n], sy = st[2 * n + 1], gx = gl[2 * n], gy = gl[2 * n + 1];
        bad |= sx < 0 || sx >= H || sy < 0 || sy >= W || gx < 0 || gx >= H || gy < 0 || gy >= W;
        if (!bad) bad |= grid[sx * W + sy] != 0 || grid[gx * W + gy] != 0;
        int seen = 0;
        for (int m = 0; m < N; ++m) {
            if (m != n) {
                bad |= st[2 * m] == sx && st[2 * m + 1] == sy;
                bad |= gl[2 * m] == gx && gl[2 * m + 1] == gy;
            }
            if (ord) seen += ord[m] == n;
        }
        if (ord) bad |= seen != 1;                       // N entries, each of 0 .. N-1 exactly once: a permutation
    }
    return __ballot(bad) == 0ull;
}

// One (case, restart) item.  write: schedule and arrivals of this case (the item's restart is the case's answer);
// summarise: the item's summary for mapf_select_kernel.  r < 0: a case flagged BAD_CASE by the selection (pass 1).
__device__ void mapf_item(const MapfArgs& p, int c, int r, bool write, bool summarise, unsigned long long* ws,
                          char* smem) {
    const int lane = threadIdx.x, N = p.N, H = p.H, W = p.W, T = p.T_max;
    unsigned long long* rows = reinterpret_cast<unsigned long long*>(smem);
    int* path = reinterpret_cast<int*>(smem + 2 * 64 * 8);
    int* arr_l = path + (GNNPP_MAPF_MAX_STEPS + 1);
    const unsigned char* grid = p.grid + (p.grid_batched ? (size_t)c * H * W : 0);
    const int* st = p.start + (size_t)c * N * 2;
    const int* gl = p.goal + (size_t)c * N * 2;
    const int* ord = (r >= 0 && p.order) ? p.order + ((size_t)c * p.R + r) * N : nullptr;

    __syncthreads();                                     // (the previous item's readers of the LDS are done)
    for (int n = lane; n < N; n += 64) arr_l[n] = -1;
    int status = 0, failing = -1, flow = 0, mk = 0;
    if (r < 0 || !mapf_case_valid(p, grid, st, gl, ord, lane)) {
        status = GNNPP_MAPF_BAD_CASE;
    } else {
        unsigned long long free_row = 0ull;
        if (lane < H)
            for (int y = 0; y < W; ++y)
                if (grid[lane * W + y] == 0) free_row |= 1ull << y;
        for (size_t i = lane; i < (size_t)(T + 1) * 5 * H; i += 64) {          // occupancy and move planes
            const size_t t = i / (5 * H), j = i - t * 5 * H;
            ws[t * kMapfPlanes * H + j] = 0ull;
        }
        __syncthreads();
        for (int k = 0; k < N; ++k) {
            const int i = ord ? ord[k] : k;
            const int sx = st[2 * i], sy = st[2 * i + 1], gx = gl[2 * i], gy = gl[2 * i + 1];
            const unsigned long long gbit = 1ull << gy;
            // t_min: one more than the last t <= T at which an earlier agent holds the goal
            int last = -1;
            for (int base = 0; base <= T; base += 64) {
                const int t = base + lane;
                const bool hit = t <= T && (ws[mapf_word(H, t, 0, gx)] & gbit) != 0ull;
                const unsigned long long m = __ballot(hit);
                if (m) last = base + 63 - __builtin_clzll(m);
            }
            const int tmin = last + 1;
            // forward: reachable layers until the goal is in one at t >= tmin
            unsigned long long R = lane == sx ? 1ull << sy : 0ull;
            if (lane < H) ws[mapf_word(H, 0, kMapfReach, lane)] = R;
            int a = (tmin <= 0 && sx == gx && sy == gy) ? 0 : -1;
            for (int t = 0; a < 0 && tmin <= T && t < T; ++t) {                // (wave-uniform)
                unsigned long long occ = ~0ull, m0 = 0ull, m1 = 0ull, m2 = 0ull, m3 = 0ull;
                if (lane < H) {
                    occ = ws[mapf_word(H, t + 1, 0, lane)];
                    m0 = ws[mapf_word(H, t, 1, lane)];
                    m1 = ws[mapf_word(H, t, 2, lane)];
                    m2 = ws[mapf_word(H, t, 3, lane)];
                    m3 = ws[mapf_word(H, t, 4, lane)];
                }
                unsigned long long* buf = rows + 64 * (t & 1);     // (double-buffered: one barrier per step)
                buf[lane] = R;
                __syncthreads();
                const unsigned long long below = lane + 1 < 64 ? buf[lane + 1] : 0ull;     // row x+1 moves up
                const unsigned long long above = lane > 0 ? buf[lane - 1] : 0ull;          // row x-1 moves down
                // entering cell a by d is a swap when a's occupant moves by -d (up <-> down, left <-> right)
                unsigned long long Rn = R | (below & ~m2) | ((R >> 1) & ~m3) | (above & ~m0) | ((R << 1) & ~m1);
                Rn &= free_row & ~occ;
                if (lane < H) ws[mapf_word(H, t + 1, kMapfReach, lane)] = Rn;
                R = Rn;
                const unsigned long long alive = __ballot(Rn != 0ull);
                const unsigned long long there = __ballot(lane == gx && (Rn & gbit) != 0ull);
                if (t + 1 >= tmin && there) a = t + 1;
                if (!alive) break;
            }
            if (a < 0) {
                status = GNNPP_MAPF_NO_PATH;
                failing = i;
                break;
            }
            // walk back from (goal, a): stop, then the cell that entered by up, left, down, right
            int cx = gx, cy = gy;
            if (lane == 0) path[a] = gx | gy << 8;
            for (int t = a; t > 0; --t) {
                int v = 0;                               // bits of row `lane` at t - 1 around column cy
                if (lane < H) {
                    const unsigned long long rp = ws[mapf_word(H, t - 1, kMapfReach, lane)];
                    v = (int)((rp >> cy) & 1ull);
                    if (cy + 1 < W) v |= (int)((rp >> (cy + 1)) & 1ull) << 1;
                    if (cy > 0) v |= (int)((rp >> (cy - 1)) & 1ull) << 2;
                    for (int e = 0; e < 4; ++e) v |= (int)((ws[mapf_word(H, t - 1, 1 + e, lane)] >> cy) & 1ull) << (3 + e);
                }
                const int me = __builtin_amdgcn_readlane(v, cx);
                const int below = cx + 1 < 64 ? __builtin_amdgcn_readlane(v, cx + 1) : 0;
                const int above = cx > 0 ? __builtin_amdgcn_readlane(v, cx - 1) : 0;
                if (me & 1) {
                } else if ((below & 1) && !((me >> (3 + 2)) & 1)) {
                    cx += 1;                             // came up from below (a swap if the occupant moves down)
                } else if (((me >> 1) & 1) && !((me >> (3 + 3)) & 1)) {
                    cy += 1;                             // came left from the right
                } else if ((above & 1) && !((me >> (3 + 0)) & 1)) {
                    cx -= 1;                             // came down from above
                } else {
                    cy -= 1;                             // came right from the left (the only one left)
                }
                if (lane == 0) path[t - 1] = cx | cy << 8;
            }
            __syncthreads();
            // commit: occupancy until T (parked on the goal from a on), the move planes, the schedule
            int* sched = write ? p.schedule + (size_t)c * (T + 1) * N * 2 : nullptr;
            for (int t = lane; t <= T; t += 64) {
                const int w = t <= a ? path[t] : (gx | gy << 8);
                const int x = w & 0xff, y = w >> 8;
                ws[mapf_word(H, t, 0, x)] |= 1ull << y;
                if (t < a) {
                    const int w1 = path[t + 1];
                    const int nx = w1 & 0xff, ny = w1 >> 8;
                    const int e = nx == x - 1 ? 0 : ny == y - 1 ? 1 : nx == x + 1 ? 2 : ny == y + 1 ? 3 : -1;
                    if (e >= 0) ws[mapf_word(H, t, 1 + e, x)] |= 1ull << y;
                }
                if (sched) {
                    sched[((size_t)t * N + i) * 2] = x;
                    sched[((size_t)t * N + i) * 2 + 1] = y;
                }
            }
            if (lane == 0) arr_l[i] = a;
            flow += a;
            mk = max(mk, a);
            __syncthreads();                             // the planes are complete before the next agent reads them
        }
    }
    if (summarise && lane == 0) {
        int* s = p.summary_ws + ((size_t)c * p.R + r) * 4;
        const bool solved = status == 0;
        s[0] = status;
        s[1] = solved ? flow : -1;
        s[2] = solved ? mk : -1;
        s[3] = failing;
    }
    if (write) {                                         // agents left unplanned: -1 everywhere
        __syncthreads();
        int* sched = p.schedule + (size_t)c * (T + 1) * N * 2;
        for (size_t j = lane; j < (size_t)(T + 1) * N; j += 64) {
            const int n = (int)(j % N);
            if (arr_l[n] < 0) {
                sched[2 * j] = -1;
                sched[2 * j + 1] = -1;
            }
        }
        for (int n = lane; n < N; n += 64) p.arrival[(size_t)c * N + n] = arr_l[n];
    }
}

// pass 0: items (case, restart) = it / R, it % R; pass 1: items = cases, restart = the selection's
__global__ __launch_bounds__(64) void mapf_plan_kernel(const MapfArgs p, int pass) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const long long items = pass ? p.C : (long long)p.C * p.R;
    unsigned long long* ws = p.slots_ws + (size_t)blockIdx.x * mapf_slot_words(p.H, p.T_max);
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int c = pass ? (int)it : (int)(it / p.R);
        const int r = pass ? p.restart[c] : (int)(it % p.R);
        mapf_item(p, c, r, pass == 1 || p.R == 1, pass == 0, ws, gnnpp_smem);
    }
}

// one thread per case: BAD_CASE when any restart is; else solved first, then smallest flowtime, smallest makespan,
// lowest restart (unsolved restarts carry flowtime = makespan = -1: the lowest unsolved one is kept).  The order is
// one 64-bit key per restart (flowtime, makespan; all ones when unsolved) and a strict minimum: the first form of this
// loop, with the comparisons spelled out on four running values, was compiled for gfx950 into code that did not carry
// the best flowtime from one restart to the next.
__global__ __launch_bounds__(64) void mapf_select_kernel(const MapfArgs p) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= p.C) return;
    bool bad = false;
    int best = -1;
    unsigned long long best_key = ~0ull;
    for (int r = 0; r < p.R; ++r) {
        const int* s = p.summary_ws + ((size_t)c * p.R + r) * 4;
        const int st = s[0];
        bad |= (st & GNNPP_MAPF_BAD_CASE) != 0;
        const unsigned long long key = st == 0 ? (unsigned long long)(unsigned)s[1] << 32 | (unsigned)s[2] : ~0ull;
        if (best < 0 || key < best_key) {
            best = r;
            best_key = key;
        }
    }
    const int* s = p.summary_ws + ((size_t)c * p.R + best) * 4;
    p.status[c] = bad ? GNNPP_MAPF_BAD_CASE : s[0];
    p.flowtime[c] = bad ? -1 : s[1];
    p.makespan[c] = bad ? -1 : s[2];
    p.failing[c] = bad ? -1 : s[3];
    p.restart[c] = bad ? -1 : best;
}

// GNNPP_OK or GNNPP_ERR_LAUNCH (arguments checked by gnnpp_mapf_solve)
int mapf_launch(const ::gnnpp_mapf& m, hipStream_t st) {
    MapfArgs a;
    static_cast<::gnnpp_mapf&>(a) = m;
    const long long items = (long long)a.C * a.R;
    a.summary_ws = reinterpret_cast<int*>(a.workspace);
    a.slots_ws = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(a.workspace) + mapf_summary_bytes(items));
    hipLaunchKernelGGL(mapf_plan_kernel, dim3(mapf_slots(items)), dim3(64), kMapfLdsBytes, st, a, 0);
    hipLaunchKernelGGL(mapf_select_kernel, dim3((a.C + 63) / 64), dim3(64), 0, st, a);
    if (a.R > 1)
        hipLaunchKernelGGL(mapf_plan_kernel, dim3(mapf_slots(a.C)), dim3(64), kMapfLdsBytes, st, a, 1);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

}  // namespace gnnpp
