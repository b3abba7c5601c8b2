// MAPF schedules audited on the device (include/gnnpp_mapf_audit.h): STATE, VERTEX, MOVE and SWAP
// offences of a schedule, the agents' arrivals and the costs.  Unlike the solvers an audit has no dependence between time
// steps: the offences of a transition t -> t + 1 follow from two layers of positions, so the work is cut into items.
//
// mapf_audit_kernel    one item is (case, chunk of GNNPP_MAPF_AUDIT_CHUNK transitions): chunk k OWNS the layers
//     k CHUNK .. k CHUNK + CHUNK - 1 (counts them) and the transitions that start on them; it also classifies the layer
//     (k + 1) CHUNK, which shields its last transition, without counting it -- so a transition across a seam is examined
//     exactly once and the layer on a seam is counted once.  One WORKGROUP per item, one thread per agent (rounded up to
//     whole waves); a persistent grid of at most kAuditGrid workgroups strides over the C x (T_max / CHUNK + 1) items.
//     No N^2 scan and no atomics: an OWNER TABLE in LDS, 16 bits per cell (128 KB at 256 x 256; the dynamic LDS request
//     is sized to the map).  Every agent stores its index at its cell, a barrier, then it reads the entry back: a reader
//     that finds another index shares its cell; it marks itself and the index it found in a per-agent flag array (every
//     writer of a flag writes 1).  Whoever won the race for the cell, the agents on it are all marked: the losers by
//     themselves, the winner by a loser.  A swap is one look at owner_t[pos_{t+1}[i]] and that agent's next cell.  The
//     table is never cleared, not even at the start: an entry is only believed when the agent it names really stands on
//     the cell (pos_t[j] == cell, read from the LDS copy of the layer), which a stale or uninitialised entry cannot
//     pass unless it happens to be right.  The look is taken BEFORE layer t + 1 overwrites the table and used only when
//     both layers turn out clean (then owner_t held every agent of layer t, each alone on its cell: exact).
//     Racing plain stores go through __hip_atomic_store, relaxed.  Five barriers per layer; every branch around a barrier
//     is workgroup-uniform (a flag read from LDS behind a barrier).
//     Partials of an item, to the workspace: per agent the last owned t off its goal (-1: none), and a header of the
//     counts per class, the agents off their start (chunk 0) and the smallest key (t << 12 | class << 10 | agent) flagged.
// mapf_audit_final_kernel    one workgroup per case: reduces the partials of the case's chunks in chunk order, finds
//     `other` of the one reported pair by a scan over the N agents of that layer, and writes every output, those of
//     skipped cases too.
// Sums and minima over a workgroup go through the wave butterfly on floats (every value is an integer below 2^24: exact).
#include "../../include/gnnpp_mapf_audit.h"
#include "gnnpp_common.h"

namespace gnnpp {

constexpr int kAuditChunk = GNNPP_MAPF_AUDIT_CHUNK;
constexpr int kAuditGrid = 2048;                // persistent workgroups at most (either kernel)
constexpr int kAuditWaves = 16;                 // waves of a workgroup at most
constexpr int kAuditHdr = 8;                    // ints of an item's header: counts [4], off start, key, 2 unused
constexpr int kAuditNone = 0xffffff;            // "no key" / "no agent": above every key, exact as a float

struct MapfAuditArgs {
    const unsigned char* grid;
    int grid_batched;
    const int* start;
    const int* goal;
    const int* schedule;
    const int* steps;
    int C, N, H, W, T_max;
    int* status;
    int* arrival;
    int* makespan;
    int* flowtime;
    int* counts;
    int* first;
    int* ws;                                    // [C][chunks][kAuditHdr + N]
};

inline int mapf_audit_threads(int N) { return (N + 63) & ~63; }
inline int mapf_audit_chunks(int T_max) { return T_max / kAuditChunk + 1; }
inline size_t mapf_audit_ws_bytes(int C, int N, int T_max) {
    return (size_t)C * mapf_audit_chunks(T_max) * (kAuditHdr + N) * sizeof(int);
}
// LDS: owner [H W] u16, rounded up to whole ints | pos [2][threads] | vflag [threads] | lflag [3][CHUNK + 1] |
// part [kAuditWaves][8]
inline size_t mapf_audit_lds_bytes(int threads, int H, int W) {
    return (size_t)((H * W + 1) / 2 + 3 * threads + 3 * (kAuditChunk + 1) + 8 * kAuditWaves) * sizeof(int);
}

__device__ __forceinline__ void audit_raise(int* flag) {
    __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // (on LDS; every writer writes 1)
}

__global__ __launch_bounds__(1024) void mapf_audit_kernel(const MapfAuditArgs p) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int tid = threadIdx.x, nth = blockDim.x, nw = nth >> 6;
    const int N = p.N, H = p.H, W = p.W, cells = H * W;
    const int K = p.T_max / kAuditChunk + 1;
    const bool active = tid < N;
    unsigned short* owner = reinterpret_cast<unsigned short*>(gnnpp_smem);
    int* pos = reinterpret_cast<int*>(gnnpp_smem) + (cells + 1) / 2;
    int* vflag = pos + 2 * nth;
    int* lflag = vflag + nth;                            // [layer of the item][STATE, VERTEX, MOVE of the transition from it]
    int* part = lflag + 3 * (kAuditChunk + 1);
    const long long items = (long long)p.C * K;

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int c = (int)(item / K), k = (int)(item - (long long)c * K);
        int L = p.steps != nullptr ? p.steps[c] : p.T_max;
        if (L > p.T_max) L = p.T_max;
        const int t0 = k * kAuditChunk;
        if (L < 0 || t0 > L) continue;                   // uniform: a skipped case, or a chunk beyond the last row
        const int t1 = min(t0 + kAuditChunk, L);         // the last layer the item looks at
        __syncthreads();                                 // (the previous item's readers of the LDS are done)
        for (int f = tid; f < 3 * (kAuditChunk + 1); f += nth) lflag[f] = 0;
        vflag[tid] = 0;
        __syncthreads();                                 // (the flags are down before the first layer raises one)
        const unsigned char* grid = p.grid + (p.grid_batched ? (size_t)c * cells : 0);
        const int* sched = p.schedule + ((size_t)c * (p.T_max + 1) * N + (active ? tid : 0)) * 2;
        int gx = 0, gy = 0;
        if (active) {
            gx = p.goal[((size_t)c * N + tid) * 2];
            gy = p.goal[((size_t)c * N + tid) * 2 + 1];
        }
        int cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0, off_start = 0, key = kAuditNone, lastoff = -1;
        int px = 0, py = 0, pcell = -1;
        bool prev_clean = false;
        int nx = 0, ny = 0;                              // the next layer, loaded one layer ahead
        if (active) {
            nx = sched[(size_t)t0 * N * 2];
            ny = sched[(size_t)t0 * N * 2 + 1];
        }
        for (int l = 0; t0 + l <= t1; ++l) {
            const int t = t0 + l;
            const int x = nx, y = ny;
            if (active && t < t1) {
                nx = sched[(size_t)(t + 1) * N * 2];
                ny = sched[(size_t)(t + 1) * N * 2 + 1];
            }
            // ---- STATE of layer t -------------------------------------------------------------------------------
            const bool on = x >= 0 && x < H && y >= 0 && y < W;
            const int cell = on ? x * W + y : -1;
            const bool sbad = active && (!on || grid[cell] != 0);
            int* P = pos + (l & 1) * nth;
            const int* Pprev = pos + ((l & 1) ^ 1) * nth;
            P[tid] = active && !sbad ? cell : -1;
            if (sbad) audit_raise(lflag + 3 * l);
            __syncthreads();                             // 1: the layer's cells and its STATE flag
            const bool layer_state = lflag[3 * l] != 0;
            // ---- the swap of t - 1 -> t, looked up while the table still holds layer t - 1 -----------------------------
            bool swapc = false;
            if (l > 0 && active && prev_clean && !layer_state && cell != pcell) {
                const int j = owner[cell];
                swapc = j < N && Pprev[j] == cell && P[j] == pcell;
            }
            __syncthreads();                             // 2: the table is free for layer t
            // ---- VERTEX of layer t ----------------------------------------------------------------------------------
            if (active && !layer_state)
                __hip_atomic_store(owner + cell, (unsigned short)tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();                             // 3
            if (active && !layer_state) {
                const int o = owner[cell];
                if (o != tid) {                          // o < N: an agent of this layer wrote it behind barrier 2
                    audit_raise(vflag + tid);
                    audit_raise(vflag + o);
                    audit_raise(lflag + 3 * l + 1);
                }
            }
            __syncthreads();                             // 4
            const bool vbad = vflag[tid] != 0;
            if (vbad) vflag[tid] = 0;                    // (its next writers come behind barrier 3 of the next layer)
            const bool clean = !layer_state && lflag[3 * l + 1] == 0;
            // ---- MOVE and SWAP of t - 1 -> t ------------------------------------------------------------------------
            if (l > 0 && prev_clean && clean) {          // uniform
                const int dx = x - px, dy = y - py;
                const bool mbad = active && (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) > 1;
                if (mbad) audit_raise(lflag + 3 * (l - 1) + 2);
                __syncthreads();                         // 5
                if (mbad) {
                    ++cnt2;
                    key = min(key, (t - 1) << 12 | GNNPP_MAPF_AUDIT_CLASS_MOVE << 10 | tid);
                } else if (swapc && lflag[3 * (l - 1) + 2] == 0) {
                    ++cnt3;
                    key = min(key, (t - 1) << 12 | GNNPP_MAPF_AUDIT_CLASS_SWAP << 10 | tid);
                }
            }
            // ---- what the item owns of layer t ------------------------------------------------------------------------
            if (l < kAuditChunk && active) {
                if (sbad) {
                    ++cnt0;
                    key = min(key, t << 12 | GNNPP_MAPF_AUDIT_CLASS_STATE << 10 | tid);
                }
                if (vbad) {
                    ++cnt1;
                    key = min(key, t << 12 | GNNPP_MAPF_AUDIT_CLASS_VERTEX << 10 | tid);
                }
                if (x != gx || y != gy) lastoff = t;
                if (t == 0 && p.start != nullptr &&
                    (x != p.start[((size_t)c * N + tid) * 2] || y != p.start[((size_t)c * N + tid) * 2 + 1]))
                    off_start = 1;
            }
            px = x;
            py = y;
            pcell = cell;
            prev_clean = clean;
        }
        // ---- the item's partials --------------------------------------------------------------------------------------
        int* ws = p.ws + (size_t)item * (kAuditHdr + N);
        if (active) ws[kAuditHdr + tid] = lastoff;
        const int s0 = (int)wave_sum((float)cnt0), s1 = (int)wave_sum((float)cnt1), s2 = (int)wave_sum((float)cnt2);
        const int s3 = (int)wave_sum((float)cnt3), s4 = (int)wave_sum((float)off_start), kmin = (int)wave_min((float)key);
        if ((tid & 63) == 0) {
            int* pw = part + (tid >> 6) * 8;
            pw[0] = s0;
            pw[1] = s1;
            pw[2] = s2;
            pw[3] = s3;
            pw[4] = s4;
            pw[5] = kmin;
        }
        __syncthreads();
        if (tid < kAuditHdr) {
            int v = tid == 5 ? kAuditNone : 0;
            if (tid < 5)
                for (int w = 0; w < nw; ++w) v += part[w * 8 + tid];
            else if (tid == 5)
                for (int w = 0; w < nw; ++w) v = min(v, part[w * 8 + 5]);
            ws[tid] = v;
        }
    }
}

__global__ __launch_bounds__(1024) void mapf_audit_final_kernel(const MapfAuditArgs p) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    int* part = reinterpret_cast<int*>(gnnpp_smem);      // [kAuditWaves][4]
    int* part2 = part + kAuditWaves * 4;                 // [kAuditWaves]
    const int tid = threadIdx.x, nw = blockDim.x >> 6;
    const int N = p.N, Kmax = p.T_max / kAuditChunk + 1;
    const bool active = tid < N;
    for (int c = blockIdx.x; c < p.C; c += gridDim.x) {
        __syncthreads();                                 // (the previous case's readers of the LDS are done)
        int L = p.steps != nullptr ? p.steps[c] : p.T_max;
        if (L > p.T_max) L = p.T_max;
        int* arrival = p.arrival + (size_t)c * N;
        if (L < 0) {                                     // uniform: a skipped case
            if (active) arrival[tid] = -1;
            if (tid < 4) {
                p.counts[(size_t)c * 4 + tid] = -1;
                p.first[(size_t)c * 4 + tid] = -1;
            }
            if (tid == 0) {
                p.status[c] = GNNPP_MAPF_AUDIT_SKIPPED;
                p.makespan[c] = -1;
                p.flowtime[c] = -1;
            }
            continue;
        }
        const int K = L / kAuditChunk + 1;
        const int* ws = p.ws + (size_t)c * Kmax * (kAuditHdr + N);
        // ---- arrivals and costs -------------------------------------------------------------------------------------
        int arr = 0;
        if (active) {
            int last = -1;
            for (int k = 0; k < K; ++k) last = max(last, ws[(size_t)k * (kAuditHdr + N) + kAuditHdr + tid]);
            arr = last + 1 > L ? -1 : last + 1;
            arrival[tid] = arr;
        }
        const int away = (int)wave_sum(arr < 0 ? 1.0f : 0.0f);
        const int amax = (int)wave_max((float)(arr < 0 ? 0 : arr));
        const int asum = (int)wave_sum((float)(arr < 0 ? 0 : arr));
        if ((tid & 63) == 0) {
            part[(tid >> 6) * 4] = away;
            part[(tid >> 6) * 4 + 1] = amax;
            part[(tid >> 6) * 4 + 2] = asum;
        }
        // ---- the chunks' headers, in chunk order (every thread: the addresses are uniform) ---------------------------------
        int cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0, off_start = 0, key = kAuditNone;
        for (int k = 0; k < K; ++k) {
            const int* h = ws + (size_t)k * (kAuditHdr + N);
            cnt0 += h[0];
            cnt1 += h[1];
            cnt2 += h[2];
            cnt3 += h[3];
            off_start += h[4];
            key = min(key, h[5]);
        }
        // ---- `other` of the reported pair ---------------------------------------------------------------------------------
        const int ft = key >> 12, fc = (key >> 10) & 3, fa = key & 1023;
        int cand = kAuditNone;
        if (key != kAuditNone && active && tid != fa &&
            (fc == GNNPP_MAPF_AUDIT_CLASS_VERTEX || fc == GNNPP_MAPF_AUDIT_CLASS_SWAP)) {
            const int* row = p.schedule + ((size_t)c * (p.T_max + 1) + ft) * N * 2;
            const int ax = row[2 * fa], ay = row[2 * fa + 1], jx = row[2 * tid], jy = row[2 * tid + 1];
            if (fc == GNNPP_MAPF_AUDIT_CLASS_VERTEX) {
                if (jx == ax && jy == ay) cand = tid;
            } else {                                     // (a SWAP is reported for a transition: ft < L)
                const int* next = row + (size_t)N * 2;
                if (jx == next[2 * fa] && jy == next[2 * fa + 1] && next[2 * tid] == ax && next[2 * tid + 1] == ay)
                    cand = tid;
            }
        }
        const int cmin = (int)wave_min((float)cand);
        if ((tid & 63) == 0) part2[tid >> 6] = cmin;
        __syncthreads();
        if (tid < 4) {
            p.counts[(size_t)c * 4 + tid] = tid == 0 ? cnt0 : tid == 1 ? cnt1 : tid == 2 ? cnt2 : cnt3;
            int other = kAuditNone;
            for (int w = 0; w < nw; ++w) other = min(other, part2[w]);
            if (other == kAuditNone) other = -1;
            p.first[(size_t)c * 4 + tid] = key == kAuditNone ? -1 : tid == 0 ? ft : tid == 1 ? fc : tid == 2 ? fa : other;
        }
        if (tid == 0) {
            int any_away = 0, mk = 0, fl = 0;
            for (int w = 0; w < nw; ++w) {
                any_away += part[w * 4];
                mk = max(mk, part[w * 4 + 1]);
                fl += part[w * 4 + 2];
            }
            int st = (cnt0 != 0 ? GNNPP_MAPF_AUDIT_STATE : 0) | (cnt1 != 0 ? GNNPP_MAPF_AUDIT_VERTEX : 0) |
                     (cnt2 != 0 ? GNNPP_MAPF_AUDIT_MOVE : 0) | (cnt3 != 0 ? GNNPP_MAPF_AUDIT_SWAP : 0);
            if (off_start != 0) st |= GNNPP_MAPF_AUDIT_BAD_START;
            if (any_away != 0) st |= GNNPP_MAPF_AUDIT_NOT_AT_GOAL;
            p.status[c] = st;
            p.makespan[c] = any_away != 0 ? -1 : mk;
            p.flowtime[c] = any_away != 0 ? -1 : fl;
        }
    }
}

// GNNPP_OK or GNNPP_ERR_LAUNCH (arguments checked by gnnpp_mapf_audit)
int mapf_audit_launch(const MapfAuditArgs& a, hipStream_t st) {
    const int threads = mapf_audit_threads(a.N);
    const long long items = (long long)a.C * mapf_audit_chunks(a.T_max);
    static LdsAttrOnce once;                             // (the owner table of a 256 x 256 map takes 128 KB)
    set_lds_attr_once(once, reinterpret_cast<const void*>(&mapf_audit_kernel),
                      (int)mapf_audit_lds_bytes(1024, GNNPP_MAPF_TEAM_MAX_SIDE, GNNPP_MAPF_TEAM_MAX_SIDE));
    hipLaunchKernelGGL(mapf_audit_kernel, dim3((unsigned)(items < kAuditGrid ? items : kAuditGrid)), dim3(threads),
                       mapf_audit_lds_bytes(threads, a.H, a.W), st, a);
    hipLaunchKernelGGL(mapf_audit_final_kernel, dim3(a.C < kAuditGrid ? a.C : kAuditGrid), dim3(threads),
                       kAuditWaves * 5 * sizeof(int), st, a);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

}  // namespace gnnpp
