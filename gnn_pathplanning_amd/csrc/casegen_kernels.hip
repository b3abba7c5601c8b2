// MAPF cases generated on the device (include/gnnpp_casegen.h): a hashed or caller-given map, closed to
// its largest free component, and N start and goal cells of that component ranked by counter hashes.
//
// casegen_kernel    one WORKGROUP per case, in the word layout of mapf_team_kernels.hip / mapf_distance_kernels.hip: a map
//     row is WR = ceil(W / 64) words, thread x * WR + j owns word j of row x (H * WR <= 1024 threads, rounded up to whole
//     waves); a persistent grid of at most kCasegenGrid workgroups strides over the cases.  Registers and LDS only: no
//     workspace, no atomics on global memory, one writer per output element.
//     Raw map: every thread builds its word from the hashes of its cells or from grid_in; no bit at columns >= W.
//     Closure: repeated floods.  One flood is the layer growth of mapf_distance_kernel -- R <- (R | its four shifts) & U
//     through a double-buffered LDS image, ONE barrier per step, until no word gained a bit (three flags in rotation: one
//     is cleared for the next step while this step's is raised) -- started at the lowest cell of U, the free cells no
//     flood has visited yet: thread order is q order, so that is the lowest set bit of the first thread with U != 0.  A
//     workgroup-wide popcount of the flood decides whether it replaces the best component so far, only when STRICTLY
//     larger: floods come in the order of their lowest q, so ties stay with the lowest q.  The loop leaves as soon as the
//     unvisited cells are no more than the best size (a component among them cannot be strictly larger), and its trip
//     count is at most the number of free cells; a flood's step count is bounded by the cells it could still take.
//     Selection of the M smallest keys of the kept cells: a binary radix select from the top bit of the key down.
//     Every thread holds a candidate mask of its word; a round hashes the candidates only, counts workgroup-wide those
//     whose bit is 0, and either narrows the candidates to them or takes them all and goes on among the others -- the
//     candidates halve every round, so a thread hashes about two words' worth of cells per stream, and the loop leaves
//     as soon as every candidate left is needed.  hash_u32 is a bijection of the 32-bit values, so the keys of a stream
//     of a case are pairwise distinct: after 32 rounds one candidate is left, and the q of the contract's (key, q) order
//     never decides.  The selected (key, q) pairs are appended to an LDS list (the slot comes from an LDS counter: the
//     order of the list is arbitrary, its ranks are not) and ranked by counting as in mapf_order_kernel: thread i counts
//     the entries that sort before its own and writes slot `rank`.
//     Fix-up of goals on starts: found in parallel, applied by one thread over the LDS list, only in a case that has one.
//     Every loop bound and every exit decision is workgroup-uniform: a count or a flag read from LDS behind a barrier.
#include "../../include/gnnpp_casegen.h"
#include "gnnpp_common.h"

namespace gnnpp {

constexpr int kCasegenGrid = 1024;              // persistent workgroups at most
constexpr int kCasegenWaves = 16;               // waves of a workgroup at most

struct CasegenArgs {
    const unsigned char* grid_in;
    int grid_in_batched;
    unsigned threshold, seed;
    int C, N, H, W;
    unsigned char* grid;
    int* start;
    int* goal;
    int* cells;
    int* status;
};

inline int casegen_threads(int H, int W) { return (H * ((W + 63) >> 6) + 63) & ~63; }
// LDS: image [2][threads] u64 | lkey [L] u32 | lq [L] | sq [N] | gq [L] (L = max(N, 2)) | part [2][2][kCasegenWaves] |
// grew [3], slots [2], fix [1], pad [2]
inline size_t casegen_lds_bytes(int threads, int N) {
    const int L = N < 2 ? 2 : N;
    return (size_t)2 * threads * 8 + (size_t)(3 * L + N) * 4 + (4 * kCasegenWaves + 8) * 4;
}

// include/gnnpp_casegen.h: key(s, c, q)
__device__ __forceinline__ unsigned casegen_key(unsigned seed, int s, int c, int q) {
    return hash_u32(seed ^ hash_u32((unsigned)c * 0x9E3779B9u + (unsigned)s * 0x85EBCA6Bu + (unsigned)q));
}

// Sum of v over the workgroup, in every thread: a wave butterfly (a wave's count is at most 64 * 64, exact in fp32), the
// waves' sums through LDS.  ONE barrier: the partial sums alternate between two buffers (`k` counts the reductions of the
// workgroup), and a buffer is rewritten only behind the barrier of the reduction after the one that read it.
__device__ __forceinline__ int casegen_sum(int v, int* part, int& k) {
    const int tid = threadIdx.x, nw = blockDim.x >> 6;
    const int s = (int)wave_sum((float)v);
    int* pk = part + (k & 1) * 2 * kCasegenWaves;
    if ((tid & 63) == 0) pk[tid >> 6] = s;
    __syncthreads();
    int sum = 0;
    for (int w = 0; w < nw; ++w) sum += pk[w];
    ++k;
    return sum;
}

// The lowest thread of the workgroup with `has`, in every thread (0x7fffffff: none); buffers and barrier as casegen_sum.
__device__ __forceinline__ int casegen_first(bool has, int* part, int& k) {
    const int tid = threadIdx.x, nw = blockDim.x >> 6;
    const unsigned long long m = __ballot(has);
    int* pk = part + (k & 1) * 2 * kCasegenWaves + kCasegenWaves;
    if ((tid & 63) == 0) pk[tid >> 6] = m != 0ull ? (tid & ~63) + __ffsll((long long)m) - 1 : 0x7fffffff;
    __syncthreads();
    int first = 0x7fffffff;
    for (int w = 0; w < nw; ++w) first = min(first, pk[w]);
    ++k;
    return first;
}

// The thread's word of the M smallest key(s, c, q) among the `cells` kept cells K (M <= cells), see the head.
__device__ __forceinline__ unsigned long long casegen_select(unsigned long long K, unsigned seed, int s, int c, int q0,
                                                             int M, int cells, int* part, int& k) {
    unsigned long long cand = K, sel = 0ull;
    int need = M, ncand = cells;                         // 1 <= need <= ncand, both uniform
    for (int r = 0; r < 32 && ncand != need; ++r) {
        unsigned long long zero = 0ull;                  // the candidates whose bit of this round is 0
        for (unsigned long long m = cand; m != 0ull; m &= m - 1ull) {
            const int b = __ffsll((long long)m) - 1;
            if (((casegen_key(seed, s, c, q0 + b) >> (31 - r)) & 1u) == 0u) zero |= 1ull << b;
        }
        const int n0 = casegen_sum(__popcll(zero), part, k);
        if (n0 >= need) {                                // the M-th smallest has a 0 here
            cand = zero;
            ncand = n0;
        } else {                                         // all of them are taken
            sel |= zero;
            cand &= ~zero;
            need -= n0;
            ncand -= n0;
        }
    }
    return sel | cand;
}

// Append the thread's selected cells to the list (lkey, lq); the caller's barrier publishes it.
__device__ __forceinline__ void casegen_append(unsigned long long sel, unsigned seed, int s, int c, int q0, unsigned* lkey,
                                               int* lq, int* slot) {
    for (unsigned long long m = sel; m != 0ull; m &= m - 1ull) {
        const int q = q0 + __ffsll((long long)m) - 1;
        const int at = __hip_atomic_fetch_add(slot, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (on LDS)
        lkey[at] = casegen_key(seed, s, c, q);
        lq[at] = q;
    }
}

// rank of entry i among the M of the list: the keys are distinct, so the ranks are
__device__ __forceinline__ int casegen_rank(const unsigned* lkey, int M, int i) {
    const unsigned ki = lkey[i];
    int rank = 0;
    for (int e = 0; e < M; ++e) rank += lkey[e] < ki ? 1 : 0;
    return rank;
}

__global__ __launch_bounds__(1024) void casegen_kernel(const CasegenArgs p) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int tid = threadIdx.x, nth = blockDim.x;
    const int N = p.N, H = p.H, W = p.W, L = N < 2 ? 2 : N;
    const int WR = (W + 63) >> 6, HW = H * WR, cells_all = H * W;
    const int x = tid / WR, j = tid - x * WR;
    const bool active = tid < HW;
    const int q0 = x * W + 64 * j;                                   // the cell of the word's bit 0
    unsigned long long* img = reinterpret_cast<unsigned long long*>(gnnpp_smem);
    unsigned* lkey = reinterpret_cast<unsigned*>(gnnpp_smem + (size_t)2 * nth * 8);
    int* lq = reinterpret_cast<int*>(lkey + L);
    int* sq = lq + L;
    int* gq = sq + N;
    int* part = gq + L;
    int* grew = part + 4 * kCasegenWaves;
    int* slots = grew + 3;
    int* fix = slots + 2;
    int k = 0;                                                       // reductions so far (casegen_sum)

    for (int c = blockIdx.x; c < p.C; c += gridDim.x) {
        __syncthreads();                                 // (the previous case's readers of the LDS are done)
        if (tid == 0) {
            grew[0] = 0;
            slots[0] = 0;
            slots[1] = 0;
            fix[0] = 0;
        }
        // ---- the raw map --------------------------------------------------------------------------------------
        unsigned long long free_w = 0ull;
        if (active) {
            const int y1 = min(W, 64 * j + 64) - 64 * j;
            if (p.grid_in != nullptr) {
                const unsigned char* g = p.grid_in + (p.grid_in_batched ? (size_t)c * cells_all : 0) + q0;
                for (int b = 0; b < y1; ++b)
                    if (g[b] == 0) free_w |= 1ull << b;
            } else {
                for (int b = 0; b < y1; ++b)
                    if (!(casegen_key(p.seed, 0, c, q0 + b) < p.threshold)) free_w |= 1ull << b;
            }
        }
        // ---- closure: the largest component, the lowest q among equals ------------------------------------------
        unsigned long long U = free_w, best = 0ull;      // not yet visited; the best component so far
        int best_n = 0, f = 0;                           // f: the step's flag, in rotation
        int un = casegen_sum(__popcll(U), part, k);      // cells of U (the barrier also publishes the cleared flags)
        while (un > best_n) {
            const int first = casegen_first(U != 0ull, part, k);
            unsigned long long R = tid == first ? U & (~U + 1ull) : 0ull;
            bool gained = R != 0ull;
            for (int t = 0; t <= un; ++t) {              // at most un - 1 steps gain a cell
                unsigned long long* buf = img + (size_t)nth * (t & 1);   // (double-buffered: one barrier per step)
                buf[tid] = R;
                if (gained) grew[f] = 1;
                const int fn = f == 2 ? 0 : f + 1;
                if (tid == 0) grew[fn] = 0;
                __syncthreads();
                const bool any = grew[f] != 0;
                f = fn;
                if (!any) break;                         // no word gained a bit: the component is complete
                unsigned long long Rn = R;
                if (active) {
                    const unsigned long long below = x + 1 < H ? buf[tid + WR] : 0ull;
                    const unsigned long long above = x > 0 ? buf[tid - WR] : 0ull;
                    const unsigned long long nextw = j + 1 < WR ? buf[tid + 1] : 0ull;
                    const unsigned long long prevw = j > 0 ? buf[tid - 1] : 0ull;
                    Rn = (R | below | above | (R >> 1) | (nextw << 63) | (R << 1) | (prevw >> 63)) & U;
                }
                gained = Rn != R;
                R = Rn;
            }
            const int n = casegen_sum(__popcll(R), part, k);
            if (n > best_n) {
                best = R;
                best_n = n;
            }
            U &= ~R;
            un -= n;
        }
        // ---- grid, cells ------------------------------------------------------------------------------------------
        img[tid] = best;
        __syncthreads();
        unsigned char* gout = p.grid + (size_t)c * cells_all;
        for (int q = tid; q < cells_all; q += nth) {
            const int xx = q / W, yy = q - xx * W;
            gout[q] = (img[xx * WR + (yy >> 6)] >> (yy & 63)) & 1ull ? 0 : 1;
        }
        int* start = p.start + (size_t)c * N * 2;
        int* goal = p.goal + (size_t)c * N * 2;
        const bool too_small = best_n < N || best_n < 2;
        if (tid == 0) {
            p.cells[c] = best_n;
            p.status[c] = too_small ? GNNPP_CASEGEN_TOO_SMALL : GNNPP_CASEGEN_OK;
        }
        if (too_small) {                                 // uniform
            for (int i = tid; i < 2 * N; i += nth) {
                start[i] = -1;
                goal[i] = -1;
            }
            continue;
        }
        // ---- starts: the N smallest of stream 1, ranked ---------------------------------------------------------
        unsigned long long sel = casegen_select(best, p.seed, 1, c, q0, N, best_n, part, k);
        casegen_append(sel, p.seed, 1, c, q0, lkey, lq, slots);
        __syncthreads();
        for (int i = tid; i < N; i += nth) {
            const int rank = casegen_rank(lkey, N, i), q = lq[i];
            sq[rank] = q;
            start[2 * rank] = q / W;
            start[2 * rank + 1] = q - (q / W) * W;
        }
        __syncthreads();                                 // (the list is free again)
        // ---- goals: the N smallest of stream 2 (two for a single agent), ranked, fixed up -------------------------
        const int M = N == 1 ? 2 : N;
        sel = casegen_select(best, p.seed, 2, c, q0, M, best_n, part, k);
        casegen_append(sel, p.seed, 2, c, q0, lkey, lq, slots + 1);
        __syncthreads();
        for (int i = tid; i < M; i += nth) gq[casegen_rank(lkey, M, i)] = lq[i];
        __syncthreads();
        for (int i = tid; i < N; i += nth)
            if (gq[i] == sq[i]) fix[0] = 1;
        __syncthreads();
        if (fix[0] != 0) {                               // uniform; rare: an agent drew its own start
            if (tid == 0) {
                if (N == 1) {
                    gq[0] = gq[1];
                } else {
                    for (int i = 0; i < N; ++i) {
                        if (gq[i] != sq[i]) continue;
                        const int e = i + 1 < N ? i + 1 : 0, g = gq[i];
                        gq[i] = gq[e];
                        gq[e] = g;
                    }
                }
            }
            __syncthreads();
        }
        for (int i = tid; i < N; i += nth) {
            const int q = gq[i];
            goal[2 * i] = q / W;
            goal[2 * i + 1] = q - (q / W) * W;
        }
    }
}

// GNNPP_OK or GNNPP_ERR_LAUNCH (arguments checked by gnnpp_casegen)
int casegen_launch(const CasegenArgs& a, hipStream_t st) {
    const int threads = casegen_threads(a.H, a.W);
    hipLaunchKernelGGL(casegen_kernel, dim3(a.C < kCasegenGrid ? a.C : kCasegenGrid), dim3(threads),
                       casegen_lds_bytes(threads, a.N), st, a);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

}  // namespace gnnpp
