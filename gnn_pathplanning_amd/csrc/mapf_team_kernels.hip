// Prioritized planning of MAPF cases for large maps and teams: the contract of mapf_kernels.hip
// (include/gnnpp.h, gnnpp_mapf) unchanged, for N <= GNNPP_ROLLOUT_MAX_TEAM agents on maps of up to
// GNNPP_MAPF_TEAM_MAX_SIDE rows and columns and horizons of up to GNNPP_MAPF_TEAM_MAX_STEPS.
//
// One WORKGROUP per (case, restart) item.  A map row is WR = ceil(W / 64) words; thread x * WR + j owns word j of row
// x (H * WR <= 1024 threads, rounded up to whole waves; the threads beyond H * WR only take part in the barriers).
// A persistent grid of at most kMapfTeamSlots workgroups strides over the items; each owns one workspace slot in
// global memory: per time step t = 0 .. T_max the six planes of mapf_kernels.hip (occupancy, four move planes indexed
// by the target cell, the reachable layer of the agent being planned), H * WR words each.
//
// Per agent:
//   t_min     every thread tests the goal's occupancy bit at its own t; the last hit is reduced over the waves' ballots
//             and then over the waves through LDS;
//   forward   one step = the own word's occupancy (t + 1) and move planes (t), loaded ONE STEP AHEAD of their use so the
//             loads are in flight across the barrier; the layer goes into a double-buffered LDS image, ONE barrier, then
//             the rows above / below (same word) and the neighbouring words of the own row (the carries of the one-bit
//             shifts) come back from the image.  Both workgroup-wide tests are made on layer t from LDS right behind the
//             barrier of step t: every thread reads the goal's word (arrival), and a flag any thread with a non-empty
//             word has raised before the barrier (layer empty; three flags in rotation: one is cleared for the next step
//             while this step's is raised);
//   walk back one wave; per hop ONE round of loads: nine lanes fetch the nine words a hop looks at (the layer at t - 1
//             at the cell and its four neighbours, the four move planes at the cell), one ballot collects their bits;
//   commit    occupancy, move planes and the schedule, parallel over t across the workgroup.
// A case is validated in O(N) per thread: the thread that owns a word sees every start and goal that falls into it
// (duplicates, obstacles), the order is checked by writing k to seen[order[k]] and reading it back.
//
// Launches as in mapf_kernels.hip: plan pass 0 over all items -> mapf_select_kernel (the same kernel: the summary
// layout is the same) -> plan pass 1 for R > 1.  No atomics, one writer per output, no host synchronisation.
#include "../../include/gnnpp.h"
#include "gnnpp_common.h"

namespace gnnpp {

constexpr int kMapfTeamSlots = 256;             // persistent workgroups at most: one per CU
constexpr int kMapfTeamMaxWaves = 16;

__host__ __device__ inline int mapf_team_row_words(int W) { return (W + 63) >> 6; }
inline int mapf_team_threads(int H, int W) { return (H * mapf_team_row_words(W) + 63) & ~63; }
__host__ __device__ inline size_t mapf_team_slot_words(int H, int W, int T) {
    return (size_t)(T + 1) * kMapfPlanes * H * mapf_team_row_words(W);
}
inline size_t mapf_team_slot_bytes(int H, int W, int T) { return mapf_team_slot_words(H, W, T) * sizeof(unsigned long long); }
inline size_t mapf_team_workspace_bytes(int C, int R, int H, int W, int T) {
    const long long items = (long long)C * R;
    return mapf_summary_bytes(items) +
           (size_t)(items < kMapfTeamSlots ? items : kMapfTeamSlots) * mapf_team_slot_bytes(H, W, T);
}
// workgroups of a call whose workspace has `bytes` bytes: min(items, kMapfTeamSlots, slots that fit); 0: not even one
inline int mapf_team_slots(long long items, int R, int C, int H, int W, int T, size_t bytes) {
    const size_t head = mapf_summary_bytes((long long)C * R);
    if (bytes < head) return 0;
    size_t fit = (bytes - head) / mapf_team_slot_bytes(H, W, T);
    if (fit > (size_t)kMapfTeamSlots) fit = kMapfTeamSlots;
    return (long long)fit < items ? (int)fit : (int)items;
}
// LDS: image [2][threads] u64 | flags: alive [4] int, bad [1], pad [3], last [16] int | path [T_max + 1] int | arrival [N]
inline size_t mapf_team_lds_bytes(int threads, int T, int N) {
    return (size_t)2 * threads * 8 + (8 + kMapfTeamMaxWaves) * 4 + (size_t)(T + 1) * 4 + (size_t)N * 4;
}

// One (case, restart) item; the arguments as mapf_item's.  HW = H * WR words per plane.
__device__ void mapf_team_item(const MapfArgs& p, int c, int r, bool write, bool summarise, unsigned long long* ws,
                               char* smem) {
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int N = p.N, H = p.H, W = p.W, T = p.T_max;
    const int WR = mapf_team_row_words(W), HW = H * WR;
    const int x = tid / WR, j = tid - x * WR;
    const bool active = tid < HW;
    unsigned long long* img = reinterpret_cast<unsigned long long*>(smem);
    int* alive = reinterpret_cast<int*>(smem + (size_t)2 * nth * 8);
    int* bad_l = alive + 4;
    int* last_l = alive + 8;
    int* path = last_l + kMapfTeamMaxWaves;
    int* arr_l = path + (T + 1);
    const unsigned char* grid = p.grid + (p.grid_batched ? (size_t)c * H * W : 0);
    const int* st = p.start + (size_t)c * N * 2;
    const int* gl = p.goal + (size_t)c * N * 2;
    const int* ord = (r >= 0 && p.order) ? p.order + ((size_t)c * p.R + r) * N : nullptr;
    const size_t plane_words = (size_t)kMapfPlanes * HW;            // words of one time step

    __syncthreads();                                     // (the previous item's readers of the LDS are done)
    unsigned long long free_w = 0ull;
    if (active) {
        const int y1 = min(W, 64 * j + 64);
        for (int y = 64 * j; y < y1; ++y)
            if (grid[x * W + y] == 0) free_w |= 1ull << (y & 63);
    }
    // ---- validation: seen[order[k]] = k (arr_l as seen), then every thread looks at all starts and goals
    bool bad = r < 0;
    if (tid == 0) bad_l[0] = 0;
    if (ord && r >= 0)
        for (int k = tid; k < N; k += nth) {
            const int i = ord[k];
            if (i >= 0 && i < N) arr_l[i] = k;
        }
    __syncthreads();
    if (r >= 0) {
        if (ord)
            for (int k = tid; k < N; k += nth) {
                const int i = ord[k];
                bad |= i < 0 || i >= N || arr_l[i] != k;     // N entries in range, no two alike: a permutation
            }
        for (int n = tid; n < N; n += nth) {
            const int sx = st[2 * n], sy = st[2 * n + 1], gx = gl[2 * n], gy = gl[2 * n + 1];
            bad |= sx < 0 || sx >= H || sy < 0 || sy >= W || gx < 0 || gx >= H || gy < 0 || gy >= W;
        }
        unsigned long long smap = 0ull, gmap = 0ull;     // starts / goals in the own word
        for (int n = 0; n < N; ++n) {
            const int sx = st[2 * n], sy = st[2 * n + 1], gx = gl[2 * n], gy = gl[2 * n + 1];
            if (active && sx == x && sy >= 0 && (sy >> 6) == j) {
                const unsigned long long b = 1ull << (sy & 63);
                bad |= (smap & b) != 0ull || (free_w & b) == 0ull;
                smap |= b;
            }
            if (active && gx == x && gy >= 0 && (gy >> 6) == j) {
                const unsigned long long b = 1ull << (gy & 63);
                bad |= (gmap & b) != 0ull || (free_w & b) == 0ull;
                gmap |= b;
            }
        }
    }
    if (bad) bad_l[0] = 1;
    __syncthreads();
    bad = bad_l[0] != 0;
    __syncthreads();                                     // (arr_l was the order check's scratch)
    for (int n = tid; n < N; n += nth) arr_l[n] = -1;

    int status = 0, failing = -1, flow = 0, mk = 0;
    if (bad) {
        status = GNNPP_MAPF_BAD_CASE;
    } else {
        for (size_t i = tid; i < (size_t)(T + 1) * plane_words; i += nth) ws[i] = 0ull;
        __syncthreads();
        for (int k = 0; k < N; ++k) {
            const int i = ord ? ord[k] : k;
            const int sx = st[2 * i], sy = st[2 * i + 1], gx = gl[2 * i], gy = gl[2 * i + 1];
            const int gidx = gx * WR + (gy >> 6);
            const unsigned long long gbit = 1ull << (gy & 63);
            // ---- t_min: one more than the last t <= T at which an earlier agent holds the goal
            int last = -1;
            for (int base = 0; base <= T; base += nth) {
                const int t = base + tid;
                const bool hit = t <= T && (ws[(size_t)t * plane_words + gidx] & gbit) != 0ull;
                const unsigned long long m = __ballot(hit);
                if (m) last = base + wave * 64 + 63 - __builtin_clzll(m);
            }
            if (lane == 0) last_l[wave] = last;
            if (tid == 0) {
                alive[0] = 0;
                alive[1] = 0;
                alive[2] = 0;
            }
            __syncthreads();
            for (int w = 0; w < (nth >> 6); ++w) last = max(last, last_l[w]);
            const int tmin = last + 1;
            // ---- forward: reachable layers until the goal is in one at t >= tmin
            unsigned long long R = (active && x == sx && j == (sy >> 6)) ? 1ull << (sy & 63) : 0ull;
            int a = -1;
            if (tmin <= T) {
                const unsigned long long* wp = ws + tid;             // the own word of plane 0 at step t
                unsigned long long occ = ~0ull, m0 = 0ull, m1 = 0ull, m2 = 0ull, m3 = 0ull;
                if (active && T > 0) {
                    occ = wp[plane_words];
                    m0 = wp[HW];
                    m1 = wp[2 * HW];
                    m2 = wp[3 * HW];
                    m3 = wp[4 * HW];
                }
                int f = 0;                                           // t % 3: the step's "layer not empty" flag
                for (int t = 0;; ++t) {
                    unsigned long long* buf = img + (size_t)nth * (t & 1);       // (double-buffered: one barrier per step)
                    buf[tid] = R;
                    if (active) ws[(size_t)t * plane_words + (size_t)kMapfReach * HW + tid] = R;
                    if (R != 0ull) alive[f] = 1;
                    const int fn = f == 2 ? 0 : f + 1;
                    if (tid == 0) alive[fn] = 0;
                    // the planes of step t + 1: in flight across the barrier and this step's arithmetic
                    unsigned long long occ_n = ~0ull, n0 = 0ull, n1 = 0ull, n2 = 0ull, n3 = 0ull;
                    if (active && t + 1 < T) {
                        const unsigned long long* q = wp + (size_t)(t + 1) * plane_words;
                        occ_n = q[plane_words];
                        n0 = q[HW];
                        n1 = q[2 * HW];
                        n2 = q[3 * HW];
                        n3 = q[4 * HW];
                    }
                    __syncthreads();
                    if (t >= tmin && (buf[gidx] & gbit) != 0ull) {
                        a = t;
                        break;
                    }
                    if (alive[f] == 0 || t == T) break;
                    unsigned long long Rn = 0ull;
                    if (active) {
                        const unsigned long long below = x + 1 < H ? buf[tid + WR] : 0ull;     // row x+1 moves up
                        const unsigned long long above = x > 0 ? buf[tid - WR] : 0ull;         // row x-1 moves down
                        const unsigned long long nextw = j + 1 < WR ? buf[tid + 1] : 0ull;
                        const unsigned long long prevw = j > 0 ? buf[tid - 1] : 0ull;
                        const unsigned long long from_right = (R >> 1) | (nextw << 63);        // moves left
                        const unsigned long long from_left = (R << 1) | (prevw >> 63);         // moves right
                        // entering cell a by d is a swap when a's occupant moves by -d (up <-> down, left <-> right)
                        Rn = R | (below & ~m2) | (from_right & ~m3) | (above & ~m0) | (from_left & ~m1);
                        Rn &= free_w & ~occ;
                    }
                    R = Rn;
                    occ = occ_n;
                    m0 = n0;
                    m1 = n1;
                    m2 = n2;
                    m3 = n3;
                    f = fn;
                }
            }
            if (a < 0) {
                status = GNNPP_MAPF_NO_PATH;
                failing = i;
                break;
            }
            // ---- walk back from (goal, a): stop, then the cell that entered by up, left, down, right
            __syncthreads();                             // the layers are in memory
            if (wave == 0) {
                int cx = gx, cy = gy;
                if (lane == 0) path[a] = gx | gy << 8;
                for (int t = a; t > 0; --t) {
                    // lane 0: layer at the cell, 1: below, 2: right, 3: above, 4: left; lanes 5 .. 8: move plane lane - 5
                    const int lx = lane == 1 ? cx + 1 : lane == 3 ? cx - 1 : cx;
                    const int ly = lane == 2 ? cy + 1 : lane == 4 ? cy - 1 : cy;
                    bool bit = false;
                    if (lane < 9 && lx >= 0 && lx < H && ly >= 0 && ly < W) {
                        const int plane = lane < 5 ? kMapfReach : lane - 4;
                        const unsigned long long v =
                            ws[(size_t)(t - 1) * plane_words + (size_t)plane * HW + lx * WR + (ly >> 6)];
                        bit = ((v >> (ly & 63)) & 1ull) != 0ull;
                    }
                    const unsigned v = (unsigned)__ballot(bit);
                    if (v & 1u) {
                    } else if ((v & 2u) && !(v & (1u << (5 + 2)))) {
                        cx += 1;                         // came up from below (a swap if the occupant moves down)
                    } else if ((v & 4u) && !(v & (1u << (5 + 3)))) {
                        cy += 1;                         // came left from the right
                    } else if ((v & 8u) && !(v & (1u << (5 + 0)))) {
                        cx -= 1;                         // came down from above
                    } else {
                        cy -= 1;                         // came right from the left (the only one left)
                    }
                    if (lane == 0) path[t - 1] = cx | cy << 8;
                }
            }
            __syncthreads();
            // ---- commit: occupancy until T (parked on the goal from a on), the move planes, the schedule
            int* sched = write ? p.schedule + (size_t)c * (T + 1) * N * 2 : nullptr;
            for (int t = tid; t <= T; t += nth) {
                const int w = t <= a ? path[t] : (gx | gy << 8);
                const int px = w & 0xff, py = w >> 8;
                unsigned long long* cell = ws + (size_t)t * plane_words + px * WR + (py >> 6);
                cell[0] |= 1ull << (py & 63);
                if (t < a) {
                    const int w1 = path[t + 1];
                    const int nx = w1 & 0xff, ny = w1 >> 8;
                    const int e = nx == px - 1 ? 0 : ny == py - 1 ? 1 : nx == px + 1 ? 2 : ny == py + 1 ? 3 : -1;
                    if (e >= 0) cell[(size_t)(1 + e) * HW] |= 1ull << (py & 63);
                }
                if (sched) {
                    sched[((size_t)t * N + i) * 2] = px;
                    sched[((size_t)t * N + i) * 2 + 1] = py;
                }
            }
            if (tid == 0) arr_l[i] = a;
            flow += a;
            mk = max(mk, a);
            __syncthreads();                             // the planes are complete before the next agent reads them
        }
    }
    if (summarise && tid == 0) {
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
        for (int n = tid; n < N; n += nth) p.arrival[(size_t)c * N + n] = arr_l[n];
        if (status != 0)
            for (size_t jj = tid; jj < (size_t)(T + 1) * N; jj += nth) {
                const int n = (int)(jj % N);
                if (arr_l[n] < 0) {
                    sched[2 * jj] = -1;
                    sched[2 * jj + 1] = -1;
                }
            }
    }
}

// pass 0: items (case, restart) = it / R, it % R; pass 1: items = cases, restart = the selection's
__global__ __launch_bounds__(1024) void mapf_team_plan_kernel(const MapfArgs p, int pass) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const long long items = pass ? p.C : (long long)p.C * p.R;
    unsigned long long* ws = p.slots_ws + (size_t)blockIdx.x * mapf_team_slot_words(p.H, p.W, p.T_max);
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int c = pass ? (int)it : (int)(it / p.R);
        const int r = pass ? p.restart[c] : (int)(it % p.R);
        mapf_team_item(p, c, r, pass == 1 || p.R == 1, pass == 0, ws, gnnpp_smem);
    }
}

// GNNPP_OK or GNNPP_ERR_LAUNCH (arguments checked by gnnpp_mapf_team_solve; slots >= 1 workgroups = workspace slots)
int mapf_team_launch(const ::gnnpp_mapf& m, int slots, hipStream_t st) {
    MapfArgs a;
    static_cast<::gnnpp_mapf&>(a) = m;
    const long long items = (long long)a.C * a.R;
    a.summary_ws = reinterpret_cast<int*>(a.workspace);
    a.slots_ws = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(a.workspace) + mapf_summary_bytes(items));
    const int threads = mapf_team_threads(a.H, a.W);
    const size_t lds = mapf_team_lds_bytes(threads, a.T_max, a.N);
    hipLaunchKernelGGL(mapf_team_plan_kernel, dim3(slots), dim3(threads), lds, st, a, 0);
    hipLaunchKernelGGL(mapf_select_kernel, dim3((a.C + 63) / 64), dim3(64), 0, st, a);
    if (a.R > 1)
        hipLaunchKernelGGL(mapf_team_plan_kernel, dim3(slots < a.C ? slots : a.C), dim3(threads), lds, st, a, 1);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

}  // namespace gnnpp
