// Goal distances and planning orders for the MAPF solver (include/gnnpp_mapf_distance.h): what the
// planning orders of mapf_kernels.hip / mapf_team_kernels.hip are built from, computed on the device.
//
// mapf_distance_kernel    one ITEM per (case, agent): a breadth-first search over the static map, bit-parallel in the
//     word layout of mapf_team_kernels.hip -- a map row is WR = ceil(W / 64) words, thread x * WR + j of the item owns
//     word j of row x (H * WR <= 1024 threads).  Layers only grow: R_0 = {start}, R_{t+1} = (R_t | its four shifts) &
//     free.  A horizontal step is a one-bit shift with the carry taken from the neighbouring word of the row, a vertical
//     step reads the same word of the rows above and below; all four come from a double-buffered LDS image of the layer
//     (ONE barrier per step).  The free mask has no bit at columns >= W, so nothing leaves the map.
//     An item ends at the first t whose layer holds the goal (dist = t), at the first t whose layer gained no bit
//     (dist = -1), and in any case at t = H W; the loop bound H W + 1 is a constant of the launch.  Both tests are
//     made on LDS right behind the step's barrier: every thread of the item reads the goal's word and a flag any thread
//     whose word gained a bit has raised before the barrier (three flags in rotation, as in the team solver: one is
//     cleared for the next step while this step's is raised).
//     Items per workgroup: an item of H * WR <= 64 threads (every map of up to 64 x 64 cells) takes ONE WAVE, and a
//     workgroup holds kMapfDistWaveItems = 4 of them -- 256 threads, so thousands of small searches fill the chip with
//     whole workgroups; a larger item has a workgroup of its own (its threads rounded up to whole waves).  The items of
//     a workgroup finish at different steps: a finished item's threads keep walking through the barriers with their
//     layer frozen, and the workgroup leaves the loop one step after a flag that every still-searching item raises
//     stays down -- read from LDS behind the barrier, so the decision is uniform and every barrier is reached by every
//     thread.  A persistent grid of at most kMapfDistGrid workgroups strides over the batches of items.
//     Registers and LDS only: no workspace, no atomics, thread 0 of an item is the one writer of its dist.
// mapf_distance_bounds_kernel   one wave per case: max and sum of its distances (-1 when one is negative).
// mapf_order_kernel       one workgroup per (case, restart): the N sort keys in LDS, thread i counts the keys that sort
//     before its own (smaller key, or the same key and a smaller index: O(N) broadcast reads) and writes
//     order[rank] = i.  Ranks are distinct, so every slot is written exactly once; no sort network, no atomics.
#include "../../include/gnnpp_mapf_distance.h"
#include "gnnpp_common.h"

namespace gnnpp {

constexpr int kMapfDistGrid = 1024;             // persistent workgroups at most: four per CU
constexpr int kMapfDistWaveItems = 4;           // items of one wave or less in a workgroup
constexpr int kMapfOrderRules = 32;             // restarts per launch of the order kernel: two bits of a 64-bit word each

struct MapfDistArgs {
    const unsigned char* grid;
    int grid_batched;
    const int* start;
    const int* goal;
    int C, N, H, W;
    int* dist;
    int* lower_makespan;
    int* lower_flowtime;
};

inline int mapf_dist_item_threads(int H, int W) { return (H * ((W + 63) >> 6) + 63) & ~63; }
inline int mapf_dist_group_items(int H, int W, long long items) {
    if (H * ((W + 63) >> 6) > 64) return 1;
    return items < kMapfDistWaveItems ? (int)items : kMapfDistWaveItems;
}
// LDS: image [2][threads] u64 | run [4] int (three in rotation) | grew [3][kMapfDistWaveItems] int
inline size_t mapf_dist_lds_bytes(int threads) { return (size_t)2 * threads * 8 + (4 + 3 * kMapfDistWaveItems) * 4; }

// G items per workgroup, blockDim.x / G threads each (whole waves)
__global__ __launch_bounds__(1024) void mapf_distance_kernel(const MapfDistArgs p, int G) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int tid = threadIdx.x, nth = blockDim.x;
    const int N = p.N, H = p.H, W = p.W;
    const int WR = (W + 63) >> 6, HW = H * WR, steps = H * W;
    const int gth = nth / G, g = tid / gth, lt = tid - g * gth;      // the item's threads, the item, the thread in it
    const int x = lt / WR, j = lt - x * WR;
    const bool active = lt < HW;
    unsigned long long* img = reinterpret_cast<unsigned long long*>(gnnpp_smem);
    int* run = reinterpret_cast<int*>(gnnpp_smem + (size_t)2 * nth * 8);
    int* grew = run + 4;
    const long long items = (long long)p.C * N, batches = (items + G - 1) / G;
    int c_have = -1;                                                 // the case free_w was built from
    unsigned long long free_w = 0ull;

    for (long long b = blockIdx.x; b < batches; b += gridDim.x) {
        const long long it = b * G + g;
        const bool have = it < items;
        const int c = have ? (int)(it / N) : 0;
        __syncthreads();                                 // (the previous batch's readers of the LDS are done)
        if (tid == 0) run[0] = 0;
        if (lt == 0) grew[g] = 0;
        if (have && active && (c_have < 0 || (p.grid_batched && c != c_have))) {
            const unsigned char* grid = p.grid + (p.grid_batched ? (size_t)c * H * W : 0);
            free_w = 0ull;
            const int y1 = min(W, 64 * j + 64);
            for (int y = 64 * j; y < y1; ++y)
                if (grid[x * W + y] == 0) free_w |= 1ull << (y & 63);
            c_have = c;
        }
        int sx = 0, sy = 0, gx = 0, gy = 0;
        bool ok = false;
        if (have) {
            sx = p.start[2 * it];
            sy = p.start[2 * it + 1];
            gx = p.goal[2 * it];
            gy = p.goal[2 * it + 1];
            ok = sx >= 0 && sx < H && sy >= 0 && sy < W && gx >= 0 && gx < H && gy >= 0 && gy < W;
            if (ok) {
                const unsigned char* grid = p.grid + (p.grid_batched ? (size_t)c * H * W : 0);
                ok = grid[sx * W + sy] == 0 && grid[gx * W + gy] == 0;
            }
        }
        int d = ok ? GNNPP_MAPF_DIST_UNREACHABLE : GNNPP_MAPF_DIST_INVALID;
        bool searching = ok;                             // uniform over the item's threads
        const int gidx = ok ? g * gth + gx * WR + (gy >> 6) : 0;
        const unsigned long long gbit = 1ull << (gy & 63);
        unsigned long long R = (ok && active && x == sx && j == (sy >> 6)) ? 1ull << (sy & 63) : 0ull;
        bool gained = R != 0ull;
        __syncthreads();
        int f = 0;                                       // t % 3: the step's flags
        for (int t = 0; t <= steps + 1; ++t) {
            unsigned long long* buf = img + (size_t)nth * (t & 1);   // (double-buffered: one barrier per step)
            buf[tid] = R;
            if (searching) {
                run[f] = 1;
                if (gained) grew[f * kMapfDistWaveItems + g] = 1;
            }
            const int fn = f == 2 ? 0 : f + 1;
            if (tid == 0) run[fn] = 0;
            if (lt == 0) grew[fn * kMapfDistWaveItems + g] = 0;
            __syncthreads();
            if (run[f] == 0) break;                      // no item of the workgroup is searching any more
            if (searching) {
                if ((buf[gidx] & gbit) != 0ull) {
                    d = t;
                    searching = false;
                } else if (grew[f * kMapfDistWaveItems + g] == 0 || t >= steps) {
                    searching = false;                   // the layer stopped growing: no path
                }
            }
            unsigned long long Rn = R;
            if (searching && active) {
                const unsigned long long below = x + 1 < H ? buf[tid + WR] : 0ull;
                const unsigned long long above = x > 0 ? buf[tid - WR] : 0ull;
                const unsigned long long nextw = j + 1 < WR ? buf[tid + 1] : 0ull;
                const unsigned long long prevw = j > 0 ? buf[tid - 1] : 0ull;
                Rn = (R | below | above | (R >> 1) | (nextw << 63) | (R << 1) | (prevw >> 63)) & free_w;
            }
            gained = Rn != R;
            R = Rn;
            f = fn;
        }
        if (have && lt == 0) p.dist[it] = d;
    }
}

// one wave per case; LDS: [3][64] int
__global__ __launch_bounds__(64) void mapf_distance_bounds_kernel(const MapfDistArgs p) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    int* red = reinterpret_cast<int*>(gnnpp_smem);
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < p.C; c += gridDim.x) {
        int mx = 0, sum = 0, neg = 0;
        for (int n = tid; n < p.N; n += 64) {
            const int d = p.dist[(size_t)c * p.N + n];
            neg |= d < 0;
            mx = max(mx, d);
            sum += max(d, 0);
        }
        red[tid] = mx;
        red[64 + tid] = sum;
        red[128 + tid] = neg;
        __syncthreads();
        if (tid == 0) {
            for (int l = 1; l < 64; ++l) {
                mx = max(mx, red[l]);
                sum += red[64 + l];
                neg |= red[128 + l];
            }
            p.lower_makespan[c] = neg ? -1 : mx;
            p.lower_flowtime[c] = neg ? -1 : sum;
        }
        __syncthreads();
    }
}

// GNNPP_OK or GNNPP_ERR_LAUNCH (arguments checked by gnnpp_mapf_distances)
int mapf_distance_launch(const MapfDistArgs& a, hipStream_t st) {
    const long long items = (long long)a.C * a.N;
    const int G = mapf_dist_group_items(a.H, a.W, items);
    const int threads = G * mapf_dist_item_threads(a.H, a.W);
    const long long batches = (items + G - 1) / G;
    hipLaunchKernelGGL(mapf_distance_kernel, dim3((unsigned)(batches < kMapfDistGrid ? batches : kMapfDistGrid)),
                       dim3(threads), mapf_dist_lds_bytes(threads), st, a, G);
    hipLaunchKernelGGL(mapf_distance_bounds_kernel, dim3(a.C < kMapfDistGrid ? a.C : kMapfDistGrid), dim3(64),
                       3 * 64 * sizeof(int), st, a);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

struct MapfOrderArgs {
    const int* dist;
    int C, N, R;
    int r0, nr;                     // this launch ranks restarts r0 .. r0 + nr - 1
    unsigned long long rules;       // rule of restart r0 + k: bits 2 k, 2 k + 1
    unsigned seed;
    int* order;
};

// the sort key of agent i under a rule (ascending; ties by index): see include/gnnpp_mapf_distance.h
__device__ __forceinline__ unsigned mapf_order_key(int rule, int d, unsigned seed, int c, int r, int i) {
    if (rule == GNNPP_MAPF_ORDER_LONGEST_FIRST) return d < 0 ? 0u : 1u + (0x7fffffffu - (unsigned)d);
    if (rule == GNNPP_MAPF_ORDER_SHORTEST_FIRST) return d < 0 ? 0u : 1u + (unsigned)d;
    if (rule == GNNPP_MAPF_ORDER_HASHED)
        return hash_u32(seed ^ hash_u32((unsigned)c * 0x9E3779B9u + (unsigned)r * 0x85EBCA6Bu + (unsigned)i));
    return (unsigned)i;
}

__global__ __launch_bounds__(1024) void mapf_order_kernel(const MapfOrderArgs p) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    unsigned* key = reinterpret_cast<unsigned*>(gnnpp_smem);         // [N]
    const int tid = threadIdx.x, nth = blockDim.x, N = p.N;
    const int k = (int)(blockIdx.x % (unsigned)p.nr), c = (int)(blockIdx.x / (unsigned)p.nr), r = p.r0 + k;
    const int rule = (int)((p.rules >> (2 * k)) & 3ull);
    const bool by_dist = rule == GNNPP_MAPF_ORDER_LONGEST_FIRST || rule == GNNPP_MAPF_ORDER_SHORTEST_FIRST;
    for (int i = tid; i < N; i += nth)
        key[i] = mapf_order_key(rule, by_dist ? p.dist[(size_t)c * N + i] : 0, p.seed, c, r, i);
    __syncthreads();
    int* out = p.order + ((size_t)c * p.R + r) * N;
    for (int i = tid; i < N; i += nth) {
        const unsigned ki = key[i];
        int rank = 0;
        for (int jj = 0; jj < N; ++jj) {
            const unsigned kj = key[jj];
            rank += (kj < ki || (kj == ki && jj < i)) ? 1 : 0;
        }
        out[rank] = i;
    }
}

// GNNPP_OK or GNNPP_ERR_LAUNCH (arguments and rules checked by gnnpp_mapf_orders)
int mapf_order_launch(const int* dist, int C, int N, int R, const int* rules, unsigned seed, int* order, hipStream_t st) {
    MapfOrderArgs a;
    a.dist = dist;
    a.C = C;
    a.N = N;
    a.R = R;
    a.seed = seed;
    a.order = order;
    for (int r0 = 0; r0 < R; r0 += kMapfOrderRules) {
        a.r0 = r0;
        a.nr = R - r0 < kMapfOrderRules ? R - r0 : kMapfOrderRules;
        a.rules = 0ull;
        for (int k = 0; k < a.nr; ++k) a.rules |= (unsigned long long)rules[r0 + k] << (2 * k);
        hipLaunchKernelGGL(mapf_order_kernel, dim3((unsigned)((long long)C * a.nr)), dim3((N + 63) & ~63),
                           (size_t)N * sizeof(unsigned), st, a);
    }
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

}  // namespace gnnpp
