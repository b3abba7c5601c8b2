// Forward graph filter (+ ReLU, + action head) for TEAM graphs of up to GNNPP_ROLLOUT_MAX_TEAM = 1024 nodes (gfx950).
//
//   y[b,n,:] = bias + sum_e sum_k W[:,e,k,:] . z_{e,k}[b,n,:],   z_{e,0} = x,
//   z_{e,k}[b,n,:] = sum_m S[b,e,m,n] * z_{e,k-1}[b,m,:]          (node n gathers COLUMN n of S)
//
// The same function as lsigf_kernel / policy_filter_kernel, for graphs whose rows do not fit one workgroup's LDS.
// Those kernels keep a whole graph in one workgroup; 8 graphs of 1024 nodes would run on 8 of the 256 CUs.  Here a
// graph is spread over many workgroups and the tap signals travel through a caller-provided workspace:
//
//   1. team_lists_kernel, once per call: a workgroup owns a strip of 16 columns of one S slab and reads it as 64-byte
//      row segments (coalesced whatever the symmetry of S; fp64 -> fp32 on load like `S.float()`).  Its four waves take
//      a quarter of the rows each, all loads of a wave in flight at once, and a ballot + prefix popcount gives every
//      non-zero its slot: per column a count, then uint16 row indices and fp32 weights in ASCENDING row order, padded
//      with (index 0, weight 0) to a multiple of four entries.  Shared S: one set of lists for the batch.
//   2. team_shift_kernel, one launch per tap k = 1 .. K-2: a half wave per node, one float4 of the features per lane
//      (lsigf_kernel's layout), an exact fp32 fmaf chain over the node's list in list order; z_k goes to the
//      workspace.  The grid covers E * B * N nodes.
//   3. team_tail_kernel, one launch: a workgroup owns a tile of 16 or 32 rows of one graph.  Per tap it brings its
//      rows of z_{e,k} into LDS -- a copy for k < K-1, the LAST shift (the same gather) for k = K-1 -- as bf16x3 planes
//      (GNNPP_PREC_FP32: six v_mfma_f32_16x16x32_bf16 per 32 channels) or fp32 rows (GNNPP_PREC_FP32_MFMA), double
//      buffered over the taps, and contracts them with the packed fragments of gnnpp_filter_pack (no second pack
//      format); bias and ReLU on the accumulators, then the store of y [B,N,F] or the action head of
//      policy_filter_kernel (each wave multiplies its own 16-feature tiles, the partial logits are summed through LDS
//      in the fixed order mt = 0 .. MT-1) and the store of logits [N,B,5].
//
// No atomics, no allocation, no host synchronisation; every output and workspace element has exactly one writer, so
// two calls give the same bytes.  Nothing but kernel launches: capturable in a HIP graph.
//
// Workspace (team_layout; every region starts 16-byte aligned, `graphs` = (s_batched ? B : 1) * E, Np = N rounded up
// to a multiple of 4, Gz = G rounded up to a multiple of 4):
//   cnt  int32  [graphs][N]            degree of column n                                  (K > 1)
//   idx  uint16 [graphs][N][Np]        row indices of the non-zeros of column n, ascending  (K > 1; the dense worst
//   val  fp32   [graphs][N][Np]        their weights                                         case: no degree bound)
//   z    fp32   [E][K-2][B][N][Gz]     z_{e,k} for k = 1 .. K-2, node-major                 (K > 2)
#include "gnnpp_common.h"

namespace gnnpp {

constexpr int kTeamMaxNodes = 1024;            // = GNNPP_ROLLOUT_MAX_TEAM (the indices are uint16 anyway)
constexpr int kTeamZs = 136;                   // LDS row stride of an fp32 tile row in floats (128 + 8, as lsigf_kernel)
constexpr int kTeamPRow = 3 * 256 + 32;        // LDS row stride of a bf16x3 tile row in bytes (as policy_filter_kernel)

struct TeamLayout { size_t cnt, idx, val, z, total; int Np, Gz; };

inline TeamLayout team_layout(int B, int N, int G, int K, int E, int s_batched) {
    TeamLayout L;
    L.Np = (N + 3) & ~3;
    L.Gz = (G + 3) & ~3;
    const size_t graphs = K > 1 ? (size_t)(s_batched ? B : 1) * E : 0;
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    size_t o = 0;
    L.cnt = o; o += up(graphs * N * sizeof(int));
    L.idx = o; o += up(graphs * N * L.Np * sizeof(unsigned short));
    L.val = o; o += up(graphs * N * L.Np * sizeof(float));
    L.z = o;   o += K > 2 ? up((size_t)E * (K - 2) * B * N * L.Gz * sizeof(float)) : 0;
    L.total = o ? o : 16;                      // (K = 1 needs none; the pointer is still required)
    return L;
}

struct TeamArgs {
    const float* x;        // [B,N,G] node-major
    const void* S;         // [B,E,N,N] | [E,N,N], fp32 or fp64
    const float* wpk;      // fp32 fragments of gnnpp_filter_pack
    const float* wpk_b;    // bf16x3 fragments (inside the same packed buffer)
    const float* bias;     // [F] | [F,N] | nullptr
    float* y;              // [B,N,F] or nullptr (head only)
    const float* act_w;    // [5,F] or nullptr
    const float* act_b;    // [5]
    float* logits;         // [N,B,5]
    int* cnt;
    unsigned short* idx;
    float* val;
    float* z;
    int B, N, G, F, K, E;
    int NG, KB, MT;        // ceil(G/16), ceil(G/32), ceil(F/16)
    int Np, Gz;
    int s_is_f64, s_batched, relu, bias_per_node;
    int x_vec;             // x rows can be read 16 bytes at a time (G % 4 == 0, 16-byte aligned base)
    int y_vec;             // ... y rows written 16 bytes at a time
};

// ---- 1. neighbour lists -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void team_lists_kernel(const TeamArgs p) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    int* wcnt = reinterpret_cast<int*>(gnnpp_smem);               // [4 waves][16 columns]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, r4 = lane >> 4;
    const int N = p.N;
    const int strips = (N + 15) >> 4;
    const int g = blockIdx.x / strips, strip = blockIdx.x - g * strips;     // g = (graph of the batch) * E + e
    const int col = strip * 16 + c;
    const bool cv = col < N;
    const int Q = (((N + 3) >> 2) + 3) & ~3;                     // rows per wave: a multiple of 4, <= 256
    const int nsteps = Q >> 2;                                    // <= 64, workgroup-uniform
    const int row0 = wave * Q;
    const size_t sbase = (size_t)g * N * N;

    // every load of the wave is issued before the first use: lane (r4, c) holds S[row0 + 4 s + r4][col], s = 0 .. 63
    float v[64];
#pragma unroll
    for (int s = 0; s < 64; ++s) {
        float t = 0.f;
        if (s < nsteps) {
            const int row = row0 + 4 * s + r4;
            if (cv && row < N) {
                const size_t i = sbase + (size_t)row * N + col;
                t = p.s_is_f64 ? (float)reinterpret_cast<const double*>(p.S)[i]
                               : reinterpret_cast<const float*>(p.S)[i];
            }
        }
        v[s] = t;
    }
    // lanes c, c + 16, c + 32, c + 48 hold four consecutive rows of column c
    const unsigned long long cmask = 0x0001000100010001ull << c;
    const unsigned long long below = cmask & ((1ull << lane) - 1ull);       // ... those of smaller rows than this lane's
    int mine = 0;                                                 // non-zeros of the column in this wave's rows
#pragma unroll
    for (int s = 0; s < 64; ++s)
        if (s < nsteps) mine += __popcll(__ballot(v[s] != 0.f) & cmask);
    if (r4 == 0) wcnt[wave * 16 + c] = mine;
    __syncthreads();
    int pos = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int n = wcnt[w * 16 + c];
        if (w < wave) pos += n;
        total += n;
    }
    const size_t lcol = (size_t)g * N + (cv ? col : 0);
    unsigned short* il = p.idx + lcol * p.Np;
    float* wl = p.val + lcol * p.Np;
#pragma unroll
    for (int s = 0; s < 64; ++s)
        if (s < nsteps) {
            const bool nz = v[s] != 0.f;                           // (false for every lane of a column >= N)
            const unsigned long long bal = __ballot(nz);
            if (nz) {
                const int slot = pos + __popcll(bal & below);
                il[slot] = (unsigned short)(row0 + 4 * s + r4);
                wl[slot] = v[s];
            }
            pos += __popcll(bal & cmask);
        }
    if (cv && wave == 0) {
        if (r4 == 0) p.cnt[lcol] = total;
        const int slot = total + r4;                               // padding to a multiple of four entries (<= 3)
        if (slot < ((total + 3) & ~3)) { il[slot] = 0; wl[slot] = 0.f; }
    }
}

// ---- the gather of one node by a half wave ------------------------------------------------------------------------
// four floats of a row at `col`; columns >= G read as zero
__device__ __forceinline__ v4f team_load4(const float* __restrict__ row, int col, int G, bool vec) {
    v4f r = vzero();
    if (vec) {
        if (col < G) r = *reinterpret_cast<const v4f*>(row + col);
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (col + u < G) r[u] = row[col + u];
    }
    return r;
}

// sum over the list (ascending rows m) of w * zsrc[m][col .. col + 4): an fmaf chain in list order, four entries per
// trip (one 8-byte read of the indices, one 16-byte read of the weights, four row reads in flight); the entries of
// the padding carry weight 0 and row 0
__device__ __forceinline__ v4f team_gather(const unsigned short* __restrict__ il, const float* __restrict__ wl,
                                           int deg, const float* __restrict__ zsrc, int stride, int col, int G,
                                           bool vec) {
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    v4f acc = vzero();
    for (int d = 0; d < deg; d += 4) {
        const v2u pk = *reinterpret_cast<const v2u*>(il + d);
        const v4f w = *reinterpret_cast<const v4f*>(wl + d);
        const unsigned m[4] = {pk[0] & 0xffffu, pk[0] >> 16, pk[1] & 0xffffu, pk[1] >> 16};
        v4f zv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) zv[u] = team_load4(zsrc + (size_t)m[u] * stride, col, G, vec);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc[0] = fmaf(w[u], zv[u][0], acc[0]);
            acc[1] = fmaf(w[u], zv[u][1], acc[1]);
            acc[2] = fmaf(w[u], zv[u][2], acc[2]);
            acc[3] = fmaf(w[u], zv[u][3], acc[3]);
        }
    }
    return acc;
}

// where z_{e,k} of graph b lives (k = 0: x itself; 1 <= k <= K-2: the workspace)
struct TeamSrc { const float* rows; int stride, G; bool vec; };
__device__ __forceinline__ TeamSrc team_signal(const TeamArgs& p, int e, int k, int b) {
    TeamSrc s;
    if (k == 0) {
        s.rows = p.x + (size_t)b * p.N * p.G; s.stride = p.G; s.G = p.G; s.vec = p.x_vec != 0;
    } else {
        s.rows = p.z + (((size_t)e * (p.K - 2) + (k - 1)) * p.B + b) * p.N * p.Gz;
        s.stride = p.Gz; s.G = p.Gz; s.vec = true;
    }
    return s;
}

// ---- 2. one shift z_{e,k-1} -> z_{e,k}, 1 <= k <= K-2 ---------------------------------------------------------------
__global__ __launch_bounds__(256) void team_shift_kernel(const TeamArgs p, int k) {
    const int tid = threadIdx.x, hl = tid & 31;
    const size_t node = (size_t)blockIdx.x * 8 + (tid >> 5);      // (e, b, n)
    const size_t per_e = (size_t)p.B * p.N;
    if (node >= per_e * p.E) return;
    const int e = (int)(node / per_e);
    const int bn = (int)(node - (size_t)e * per_e);
    const int b = bn / p.N, n = bn - b * p.N;
    const TeamSrc src = team_signal(p, e, k - 1, b);
    const size_t lcol = ((size_t)(p.s_batched ? b : 0) * p.E + e) * p.N + n;
    const int col = 4 * hl;
    const v4f acc = team_gather(p.idx + lcol * p.Np, p.val + lcol * p.Np, p.cnt[lcol], src.rows, src.stride, col,
                                src.G, src.vec);
    if (col < p.Gz) {                                             // (columns G .. Gz-1 are written as zero)
        float* dst = p.z + ((((size_t)e * (p.K - 2) + (k - 1)) * p.B + b) * p.N + n) * p.Gz;
        *reinterpret_cast<v4f*>(dst + col) = acc;
    }
}

// ---- 3. last shift + contraction + epilogue -------------------------------------------------------------------------
// RT = 16-row MFMA tiles per workgroup; MODE 2 = bf16x3 planes (GNNPP_PREC_FP32), 1 = exact fp32 MFMA.
// Wave w owns the 16-feature output tiles mt = w and w + 4 for all RT row tiles.
// SAVED (lsigf_team_train_kernel.hip): every tap signal, the last one included, is a copy from p.z laid out as
// zs [E*K][B*N][G] with row stride G -- no gather here; p.x_vec then says whether THOSE rows can be read 16 bytes at a time.
template <int RT, int MODE, bool SAVED>
__device__ __forceinline__ void team_tail_body(const TeamArgs& p) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    constexpr int R = 16 * RT;
    constexpr int kBuf = MODE == 2 ? R * kTeamPRow : R * kTeamZs * 4;       // bytes of one tap's tile
    constexpr int NA = MODE == 2 ? 12 : 8;                                     // 16-byte A pieces per (tap, mt)
    float* const part_sums = reinterpret_cast<float*>(gnnpp_smem + 2 * kBuf); // [8 mt][R][8]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = lane & 15, q = lane >> 4, hl = tid & 31;
    const int N = p.N, K = p.K;
    const int tiles = (N + R - 1) / R;
    const int b = blockIdx.x / tiles, r0 = (blockIdx.x - b * tiles) * R;
    const bool has[2] = {wave < p.MT, wave + 4 < p.MT};
    const int nblk = MODE == 2 ? p.KB : p.NG;                                  // A blocks per (tap, mt)

    v4f acc[2][RT], acc2[2][RT];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < RT; ++t) { acc[j][t] = vzero(); acc2[j][t] = vzero(); }

    int tap = 0;
    for (int e = 0; e < p.E; ++e)
        for (int k = 0; k < K; ++k, ++tap) {
            // this tap's A fragments, in flight while the tile is staged
            v4f A[2][NA];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int mt = wave + 4 * j;
                const float* wt = (MODE == 2 ? p.wpk_b + ((size_t)tap * p.MT + mt) * nblk * 768
                                             : p.wpk + ((size_t)tap * p.MT + mt) * nblk * 256) + lane * 4;
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    const int blk = MODE == 2 ? i / 3 : i;
                    A[j][i] = (has[j] && blk < nblk) ? *reinterpret_cast<const v4f*>(wt + i * 256) : vzero();
                }
            }
            // the workgroup's rows of z_{e,k}: a half wave per row, four features per lane
            char* const buf = gnnpp_smem + (tap & 1) * kBuf;
            const bool last_shift = !SAVED && K > 1 && k == K - 1;
            TeamSrc src;
            if (SAVED) {
                src.rows = p.z + ((size_t)tap * p.B + b) * N * p.G; src.stride = p.G; src.G = p.G; src.vec = p.x_vec != 0;
            } else {
                src = team_signal(p, e, last_shift ? k - 1 : k, b);
            }
            const size_t lbase = ((size_t)(p.s_batched ? b : 0) * p.E + e) * N;
            for (int i = tid >> 5; i < R; i += 8) {
                const int row = r0 + i;
                v4f v = vzero();
                if (row < N) {
                    if (last_shift) {
                        const size_t lcol = lbase + row;
                        v = team_gather(p.idx + lcol * p.Np, p.val + lcol * p.Np, p.cnt[lcol], src.rows, src.stride,
                                        4 * hl, src.G, src.vec);
                    } else {
                        v = team_load4(src.rows + (size_t)row * src.stride, 4 * hl, src.G, src.vec);
                    }
                }
                if (MODE == 2) {
                    v2f pl[3];
                    b3_split4(v, pl);
#pragma unroll
                    for (int pp = 0; pp < 3; ++pp)
                        *reinterpret_cast<v2f*>(buf + i * kTeamPRow + pp * 256 + 8 * hl) = pl[pp];
                } else {
                    *reinterpret_cast<v4f*>(reinterpret_cast<float*>(buf) + i * kTeamZs + 4 * hl) = v;
                }
            }
            __syncthreads();       // the tile is visible; the other buffer is free (its readers passed this barrier)
            // D[f, row] += W_{e,k}[f, g] z_{e,k}[row, g]
            if (MODE == 2) {
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) {
                    if (kb < nblk) {
                        v8b Bp[RT][3];
#pragma unroll
                        for (int t = 0; t < RT; ++t)
#pragma unroll
                            for (int pp = 0; pp < 3; ++pp)
                                Bp[t][pp] = as_b8(*reinterpret_cast<const v4f*>(buf + (t * 16 + a) * kTeamPRow +
                                                                                kb * 64 + q * 16 + pp * 256));
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            if (has[j]) {
#pragma unroll
                                for (int t = 0; t < RT; ++t)
#pragma unroll
                                    for (int term = 0; term < kB3Terms; ++term) {
                                        const v8b Ap = as_b8(A[j][(3 * kb + b3_term_a(term)) % NA]);
                                        if (term == kB3Terms - 1) acc[j][t] = mfma16b(Ap, Bp[t][0], acc[j][t]);
                                        else acc2[j][t] = mfma16b(Ap, Bp[t][b3_term_b(term)], acc2[j][t]);
                                    }
                            }
                    }
                }
            } else {
                const float* zt = reinterpret_cast<const float*>(buf);
#pragma unroll
                for (int gg = 0; gg < 8; ++gg) {
                    if (gg < nblk) {
                        v4f Bf[RT];
#pragma unroll
                        for (int t = 0; t < RT; ++t)
                            Bf[t] = *reinterpret_cast<const v4f*>(zt + (t * 16 + a) * kTeamZs + gg * 16 + q * 4);
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            if (has[j]) {
#pragma unroll
                                for (int s = 0; s < 4; ++s)
#pragma unroll
                                    for (int t = 0; t < RT; ++t)
                                        acc[j][t] = mfma16(A[j][gg % NA][s], Bf[t][s], acc[j][t]);
                            }
                    }
                }
            }
        }

    // ---- epilogue: bias (+ ReLU) on the accumulators; y store and / or this wave's part of the head ----------------
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (!has[j]) continue;
        const int mt = wave + 4 * j;
        const int f0 = mt * 16 + q * 4;
        v4f bv = vzero(), A5 = vzero();
        if (p.bias && !p.bias_per_node) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (f0 + r < p.F) bv[r] = p.bias[f0 + r];
        }
        if (p.act_w && a < 5) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (f0 + r < p.F) A5[r] = p.act_w[a * p.F + f0 + r];
        }
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            const int rl = t * 16 + a, row = r0 + rl;
            if (p.bias && p.bias_per_node && row < N) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (f0 + r < p.F) bv[r] = p.bias[(size_t)(f0 + r) * N + row];
            }
            v4f v = (MODE == 2 ? acc[j][t] + acc2[j][t] : acc[j][t]) + bv;
            if (p.relu) v = vrelu(v);
            if (p.y && row < N) {
                float* dst = p.y + ((size_t)b * N + row) * p.F + f0;
                if (p.y_vec) {
                    if (f0 < p.F) *reinterpret_cast<v4f*>(dst) = v;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (f0 + r < p.F) dst[r] = v[r];
                }
            }
            if (p.act_w) {
                const v4f d = mfma16x4(A5, v, vzero());            // d[r] = logit part a5 = 4 q + r of this lane's row
                float* ps = part_sums + (mt * R + rl) * 8;
                if (q == 0) *reinterpret_cast<v4f*>(ps) = d;
                else if (q == 1) ps[4] = d[0];
            }
        }
    }
    if (p.act_w) {
        __syncthreads();
        for (int i = tid; i < R * 5; i += 256) {
            const int rl = i / 5, a5 = i - rl * 5, row = r0 + rl;
            if (row < N) {
                float s = part_sums[rl * 8 + a5];
                for (int m = 1; m < p.MT; ++m) s += part_sums[(m * R + rl) * 8 + a5];
                p.logits[((size_t)row * p.B + b) * 5 + a5] = s + p.act_b[a5];
            }
        }
    }
}

template <int RT, int MODE>
__global__ __launch_bounds__(256) void team_tail_kernel(const TeamArgs p) {
    team_tail_body<RT, MODE, false>(p);
}

template <int RT, int MODE>
static hipError_t team_tail_launch(const TeamArgs& a, hipStream_t st) {
    constexpr int R = 16 * RT;
    constexpr size_t smem = 2 * (size_t)(MODE == 2 ? R * kTeamPRow : R * kTeamZs * 4) + 8 * R * 8 * sizeof(float);
    const int tiles = (a.N + R - 1) / R;
    hipLaunchKernelGGL((team_tail_kernel<RT, MODE>), dim3(a.B * tiles), dim3(256), smem, st, a);
    return hipGetLastError();
}

// team_lists_kernel on its own (gnnpp_team_lists_from_dense): `a` carries S, s_is_f64 and N; the lists of `graphs`
// slabs go to `lists` (the head of team_layout for that many graphs).
int team_lists_launch(TeamArgs a, void* lists, int graphs, hipStream_t st) {
    const TeamLayout L = team_layout(graphs, a.N, 1, 2, 1, 1);
    char* base = static_cast<char*>(lists);
    a.cnt = reinterpret_cast<int*>(base + L.cnt);
    a.idx = reinterpret_cast<unsigned short*>(base + L.idx);
    a.val = reinterpret_cast<float*>(base + L.val);
    a.Np = L.Np;
    hipLaunchKernelGGL(team_lists_kernel, dim3(graphs * ((a.N + 15) / 16)), dim3(256), 4 * 16 * sizeof(int), st, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// `a` carries the call's pointers, sizes and flags; fills in the derived fields and enqueues lists, shifts and tail.
// The caller has validated everything (nothing here can fail but a launch).
// lists != nullptr: the caller's neighbour lists (the same layout as the head of the workspace, which then goes unused)
// stand in for S and no list launch is made.
int team_launch(TeamArgs a, void* workspace, int precision, hipStream_t st, const void* lists = nullptr) {
    const TeamLayout L = team_layout(a.B, a.N, a.G, a.K, a.E, a.s_batched);
    char* ws = static_cast<char*>(workspace);
    char* lb = lists ? static_cast<char*>(const_cast<void*>(lists)) : ws;       // (read only when it is the caller's)
    a.cnt = reinterpret_cast<int*>(lb + L.cnt);
    a.idx = reinterpret_cast<unsigned short*>(lb + L.idx);
    a.val = reinterpret_cast<float*>(lb + L.val);
    a.z = reinterpret_cast<float*>(ws + L.z);
    a.Np = L.Np; a.Gz = L.Gz;
    a.NG = (a.G + 15) / 16; a.KB = (a.G + 31) / 32; a.MT = (a.F + 15) / 16;
    a.wpk_b = a.wpk + filter_packed_b3_offset(a.G, a.F, a.K, a.E);
    a.x_vec = (a.G & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
    a.y_vec = a.y && (a.F & 3) == 0 && (reinterpret_cast<uintptr_t>(a.y) & 15) == 0;
    if (a.K > 1 && !lists) {
        const int graphs = (a.s_batched ? a.B : 1) * a.E, strips = (a.N + 15) / 16;
        hipLaunchKernelGGL(team_lists_kernel, dim3(graphs * strips), dim3(256), 4 * 16 * sizeof(int), st, a);
        if (hipGetLastError() != hipSuccess) return -3;
    }
    const size_t nodes = (size_t)a.E * a.B * a.N;
    for (int k = 1; k + 1 < a.K; ++k) {
        hipLaunchKernelGGL(team_shift_kernel, dim3((unsigned)((nodes + 7) / 8)), dim3(256), 0, st, a, k);
        if (hipGetLastError() != hipSuccess) return -3;
    }
    // 32-row tiles halve the tap fragments a graph pulls from L2; 16-row tiles when those would leave CUs idle
    const bool wide = (size_t)a.B * ((a.N + 31) / 32) >= 256;
    hipError_t err;
    if (precision == kPrecFp32Mfma) err = wide ? team_tail_launch<2, 1>(a, st) : team_tail_launch<1, 1>(a, st);
    else err = wide ? team_tail_launch<2, 2>(a, st) : team_tail_launch<1, 2>(a, st);
    return err == hipSuccess ? 0 : -3;
}

}  // namespace gnnpp
