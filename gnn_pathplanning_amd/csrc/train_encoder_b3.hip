// The train-mode encoder's convolutions on bf16x3 planes (opt-in training precision; include/gnnpp_train_b3.h).
//
// conv_b3_kernel<H, W> is conv_mfma_kernel<H, W> (train_encoder.hip) with the same GEMM statement (conv_geom: rows =
// output channels, or (channel, position) for the dense 2x2 form; columns = (image, position); contraction = (tap,
// channel); the input gradient = the same shape with the transposed, flipped kernel), the same grid, the same column
// tiles per wave, the same epilogue (bias, store [N][B][C][P], per-workgroup BatchNorm (mean, M2) partials in the same
// slots) -- and another arithmetic: both operands as three exact bf16 planes (gnnpp_common.h "bf16x3"), the six plane
// products of b3_term_a / b3_term_b, small terms first, on v_mfma_f32_16x16x32_bf16 with fp32 accumulation.  96
// matrix-pipe cycles per 32 contraction elements against the 256 of eight v_mfma_f32_16x16x4_f32.
//
// How the 32-deep k-step (lane l holds k = 8 (l >> 4) + e, e = 0..7, of row / column l & 15) maps onto (tap, channel):
//   5x5 layers   one k-step per tap: k = channel of the stage (CC = 32), nine k-steps per stage;
//   dense 2x2    k = (input channel, input position) of the stage in memory order (CC = 256): eight k-steps per stage;
//   11x11 layer  ONE k-step for the whole contraction: k = tap * 3 + channel for k < 27, k = 27..31 exact zeros on both
//                sides (a zero weight plane AND a zero activation: nothing of the observations reaches those slots).
// Activation planes are made while a stage's images go to LDS (commit): the staging thread splits each fp32 value once
// (b3_split2) and writes the planes k-innermost, [plane][position][KS = CC + 8 bf16], so the B operand of any (tap,
// k-step) is ONE 16-byte read per plane at the lane's column offset plus a compile-time constant; the MFMA loop is
// ds_read_b128 + MFMA and converts nothing.  Row pitch KS * 2 = 80 B (5x5) / 528 B (dense): consecutive positions sit
// 5 / 33 sixteen-byte slots apart, so the sixteen lanes of a ds_read_b128 group (eight consecutive columns of two
// neighbouring k-octets) fall on sixteen slots with at most one pair sharing one (2-way in that group; a pitch of 64 B
// would put every fourth position on one slot).  The 11x11 layer keeps its two zero-bordered fp32 images in LDS as the
// fp32 kernel does; each lane gathers the eight (tap, channel) values of its column ONCE, splits them in registers and
// feeds its six MFMAs: every (column, k-octet) belongs to exactly one lane of the workgroup, so nothing is split twice
// and the planes never need to exist in LDS.
// Weight planes come pre-split from pack_train_weights_b3_kernel (one launch per weight version, a buffer of its own).
// Deterministic: one writer per output, fixed reduction orders, no atomics.
// Out of scope: the weight gradient (conv_wgrad_all_kernel) stays on the fp32 MFMA.
#include "gnnpp_common.h"

namespace gnnpp {

// k-steps of 32 per LDS stage of a geometry
__host__ __device__ inline int conv_b3_steps(const ConvGeom& g) { return g.H == 11 ? 1 : g.TAPS * g.CC / 32; }
// one k-step of one 16-row tile: [plane 3][lane 64][8 bf16] = 3 KB
constexpr size_t kB3StepBytes = 3 * 64 * 16;
__host__ __device__ inline size_t conv_b3_pack_bytes(int l, bool input_grad) {
    if (l == 0 && input_grad) return 0;
    const ConvGeom g = conv_geom(l, input_grad, 1);
    return (size_t)(g.M / 16) * g.nchunk * conv_b3_steps(g) * kB3StepBytes;
}
struct TrainPackB3Layout { size_t wt[kTrainLayers], wtb[kTrainLayers], total; };   // bytes
inline TrainPackB3Layout train_pack_b3_layout() {
    TrainPackB3Layout w;
    size_t o = 0;
    for (int l = 0; l < kTrainLayers; ++l) {
        w.wt[l] = o;  o += conv_b3_pack_bytes(l, false);
        w.wtb[l] = o; o += conv_b3_pack_bytes(l, true);
    }
    w.total = o;
    return w;
}

// ---- weights as bf16x3 A fragments: block ((mt * nchunk + ch) * SPS + s) = [plane][lane][e]: A[m = mt*16 + (lane & 15)]
// [k = 8 (lane >> 4) + e of k-step s of stage ch], 0 where the slot holds no contraction element.  One launch for the
// nine packs (blockIdx.y = layer * 2 + {0: forward, 1: input gradient}); a thread splits two neighbouring k slots.
struct TrainPackB3Ptrs { const float* w[kTrainLayers]; unsigned* fwd[kTrainLayers]; unsigned* ig[kTrainLayers]; };
__global__ void pack_train_weights_b3_kernel(const TrainPackB3Ptrs p) {
    const int l = blockIdx.y >> 1;
    const bool ig = blockIdx.y & 1;
    if (ig && l == 0) return;                                        // (no input gradient of the observations)
    const TrainLayerDims d = train_layer(l);
    const ConvGeom g = conv_geom(l, ig, 1);
    const int SPS = conv_b3_steps(g);
    const float* w = p.w[l];
    unsigned* out = ig ? p.ig[l] : p.fwd[l];
    const int total = (g.M / 16) * g.nchunk * SPS * 256;             // pairs
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int ep = i & 3, lane = (i >> 2) & 63, blk = i >> 8;
        const int s = blk % SPS, ch = (blk / SPS) % g.nchunk, mt = blk / (SPS * g.nchunk);
        const int m = mt * 16 + (lane & 15);
        float v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int kk = 8 * (lane >> 4) + 2 * ep + h;
            int tap, c;
            if (g.H == 11) { tap = kk / 3; c = kk < 27 ? kk - tap * 3 : g.Ck; }
            else if (g.RPC == 1) { tap = s; c = ch * g.CC + kk; }
            else { tap = 0; c = ch * g.CC + s * 32 + kk; }
            v[h] = 0.f;
            if (c < g.Ck) {
                int co, ci, t;
                if (g.RPC == 1) {                                    // the 3x3 convolution
                    co = ig ? c : m; ci = ig ? m : c; t = ig ? 8 - tap : tap;
                } else {                                             // dense 2x2: positions po (output), pi (input)
                    const int row_ch = m >> 2, row_p = m & 3, k_ch = c >> 2, k_p = c & 3;
                    co = ig ? k_ch : row_ch; ci = ig ? row_ch : k_ch;
                    const int po = ig ? k_p : row_p, pi = ig ? row_p : k_p;
                    t = ((pi >> 1) - (po >> 1) + 1) * 3 + ((pi & 1) - (po & 1) + 1);
                }
                v[h] = w[((long)co * d.Cin + ci) * 9 + t];
            }
        }
        unsigned ph, pm, pl;
        b3_split2(v[0], v[1], ph, pm, pl);
        unsigned* o = out + (size_t)blk * (kB3StepBytes / 4) + lane * 4 + ep;
        o[0] = ph;
        o[256] = pm;
        o[512] = pl;
    }
}

int train_pack_b3_launch(const float* const* conv_w, void* pack, hipStream_t st) {
    const TrainPackB3Layout PL = train_pack_b3_layout();
    TrainPackB3Ptrs pk = {};
    char* base = static_cast<char*>(pack);
    for (int l = 0; l < kTrainLayers; ++l) {
        pk.w[l] = conv_w[l];
        pk.fwd[l] = reinterpret_cast<unsigned*>(base + PL.wt[l]);
        pk.ig[l] = reinterpret_cast<unsigned*>(base + PL.wtb[l]);
    }
    hipLaunchKernelGGL(pack_train_weights_b3_kernel, dim3(128, 2 * kTrainLayers), dim3(256), 0, st, pk);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---- the convolution on v_mfma_f32_16x16x32_bf16 ------------------------------------------------------------------
// grid = (N * chunks_per_agent, M / 16), block = 256, as conv_mfma_kernel: a workgroup owns 16 output rows and the IB
// images [b0, b0 + IB) of agent n; wave w holds the accumulators of column tiles w, w + 4, ...  LDS: the stage's A
// fragments [SPS][plane][lane] (16 bytes each), then the activations (file comment).  D register r: (row 4q + r, column i).
constexpr int conv_b3_ks(int cc) { return cc + 8; }                 // bf16 between two positions' rows of a plane
template <int H, int W>
__global__ __launch_bounds__(256) void conv_b3_kernel(const float* __restrict__ x, const v4f* __restrict__ wp,
                                                      const float* __restrict__ bias, float* __restrict__ y,
                                                      float* __restrict__ part, int B, int Ck, int M, long x_sn,
                                                      long x_sb, int chunks, int nchunk) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    constexpr bool kDense = H == 1 && W == 1, kL0 = H == 11;
    constexpr int P = H * W, TAPS = kDense ? 1 : 9, RPC = kDense ? 4 : 1;
    constexpr int PP = kDense ? 1 : (H + 2) * (W + 2);
    constexpr int IB = kDense ? kDenseIB : H == 5 ? 4 : 2, CC = kDense ? 256 : H == 5 ? 32 : 4;
    constexpr int SPS = kL0 ? 1 : TAPS * CC / 32, NT = (IB * P + 15) / 16, TN = (NT + 3) / 4;
    constexpr int NPOS = IB * PP, KS = conv_b3_ks(CC), PLANE = NPOS * KS;     // (bf16 units; unused by the 11x11 layer)
    constexpr int RS0 = IB * PP;                                              // 11x11: floats between two channels' images
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, q = lane >> 4;
    const int n = blockIdx.x / chunks, chunk = blockIdx.x - n * chunks;
    const int b0 = chunk * IB, nimg = min(IB, B - b0);
    const int m0 = blockIdx.y * 16;
    v4f* wsm = reinterpret_cast<v4f*>(gnnpp_smem);                            // [SPS][3][64]
    unsigned short* xp = reinterpret_cast<unsigned short*>(wsm + SPS * 192);  // [3][NPOS][KS] bf16
    float* xs0 = reinterpret_cast<float*>(wsm + SPS * 192);                   // 11x11: [3][RS0] fp32, zero-bordered
    int cb[TN], cimg[TN], cp[TN];
    bool cv[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) {
        const int col = (wave + 4 * t) * 16 + i16;
        cv[t] = col < nimg * P;
        cimg[t] = cv[t] ? col / P : 0;
        cp[t] = cv[t] ? col - cimg[t] * P : 0;
        cb[t] = cimg[t] * PP + (kDense ? 0 : (cp[t] / W + 1) * (W + 2) + cp[t] % W + 1);     // position of the column
    }
    v4f acc[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) acc[t] = vzero();

    // Staging in two phases, as conv_mfma_kernel: issue() puts every load of a stage in flight, commit() splits the
    // values and scatters the planes into LDS.  The next stage's issue() runs BEFORE this stage's MFMAs.
    const float* xa = x + n * x_sn + (long)b0 * x_sb;
    constexpr int NWV = (SPS * 192 + 255) / 256;                 // 16-byte A-fragment loads per thread
    constexpr int XE = kL0 ? 3 * IB * P : CC * IB * P;           // image elements of a full stage
    constexpr int NXV = kL0 ? (XE + 255) / 256 : (XE / 4 + 255) / 256;
    v4f wv[NWV];
    v4f xv[kL0 ? 1 : NXV];
    float xsc[kL0 ? NXV : 1];
    auto issue = [&](int ch) {
        const v4f* wsrc = wp + ((long)(blockIdx.y * nchunk + ch) * SPS) * 192;
#pragma unroll
        for (int u = 0; u < NWV; ++u) {
            const int i = tid + u * 256;
            wv[u] = wsrc[i < SPS * 192 ? i : 0];
        }
        if constexpr (kL0) {
#pragma unroll
            for (int u = 0; u < NXV; ++u) {
                const int e = tid + u * 256;
                const int im = e / (3 * P), r = e - im * (3 * P);
                const bool ok = e < XE && im < nimg;
                xsc[u] = xa[ok ? (long)im * x_sb + r : 0];
            }
        } else {
            const int c0 = ch * CC;
#pragma unroll
            for (int u = 0; u < NXV; ++u) {
                const int e = (tid + u * 256) * 4;
                const int im = e / (CC * P), r = e - im * (CC * P);
                const bool ok = e < XE && im < nimg;
                xv[u] = *reinterpret_cast<const v4f*>(xa + (ok ? (long)im * x_sb + (long)c0 * P + r : 0));
            }
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int u = 0; u < NWV; ++u) {
            const int i = tid + u * 256;
            if (i < SPS * 192) wsm[i] = wv[u];
        }
        if constexpr (kL0) {
#pragma unroll
            for (int u = 0; u < NXV; ++u) {
                const int e = tid + u * 256;
                const int im = e / (3 * P), r = e - im * (3 * P);
                const int cl = r / P, pp = r - cl * P;
                if (e < XE && im < nimg) xs0[cl * RS0 + im * PP + (pp / W + 1) * (W + 2) + pp % W + 1] = xsc[u];
            }
        } else {
#pragma unroll
            for (int u = 0; u < NXV; ++u) {
                const int e = (tid + u * 256) * 4;
                const int im = e / (CC * P), r = e - im * (CC * P);
                if (e < XE && im < nimg) {
                    unsigned h[2], m[2], l[2];
                    b3_split2(xv[u][0], xv[u][1], h[0], m[0], l[0]);
                    b3_split2(xv[u][2], xv[u][3], h[1], m[1], l[1]);
                    if constexpr (kDense) {                      // four neighbouring k slots of image im: 8 bytes per plane
                        typedef unsigned v2u __attribute__((ext_vector_type(2)));
                        unsigned short* o = xp + im * KS + r;
                        const v2u hv = {h[0], h[1]}, mv = {m[0], m[1]}, lv = {l[0], l[1]};
                        *reinterpret_cast<v2u*>(o) = hv;
                        *reinterpret_cast<v2u*>(o + PLANE) = mv;
                        *reinterpret_cast<v2u*>(o + 2 * PLANE) = lv;
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int cl = (r + k) / P, pp = (r + k) - cl * P;
                            unsigned short* o = xp + (im * PP + (pp / W + 1) * (W + 2) + pp % W + 1) * KS + cl;
                            const int sh = (k & 1) * 16;
                            o[0] = (unsigned short)(h[k >> 1] >> sh);
                            o[PLANE] = (unsigned short)(m[k >> 1] >> sh);
                            o[2 * PLANE] = (unsigned short)(l[k >> 1] >> sh);
                        }
                    }
                }
            }
        }
    };
    issue(0);
    if constexpr (kL0) {
        for (int i = tid; i < 3 * RS0; i += 256) xs0[i] = 0.f;   // borders / a missing image stay zero
    } else if constexpr (!kDense) {
        v4f* z = reinterpret_cast<v4f*>(xp);                     // borders / missing images stay zero (all three planes)
        for (int i = tid; i < 3 * PLANE / 8; i += 256) z[i] = vzero();
    }                                                            // (dense: a column only ever reads its own image's row)
    __syncthreads();
    commit();
    __syncthreads();
    for (int ch = 0; ch < nchunk; ++ch) {
        if (ch + 1 < nchunk) issue(ch + 1);
        if constexpr (kL0) {
            // k = 8 q + e = tap * 3 + channel: this lane's eight slots, the same for all of its columns
            int goff[8];
            bool gv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int kk = 8 * q + e, tap = kk / 3, c = kk - tap * 3;
                gv[e] = kk < 27;
                goff[e] = gv[e] ? c * RS0 + (tap / 3 - 1) * (W + 2) + (tap % 3 - 1) : 0;
            }
            v4f a[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) a[pl] = wsm[pl * 64 + lane];
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                v4f lo, hi, b[3];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    lo[e] = gv[e] ? xs0[cb[t] + goff[e]] : 0.f;
                    hi[e] = gv[e + 4] ? xs0[cb[t] + goff[e + 4]] : 0.f;
                }
                b3_split8(lo, hi, b);
#pragma unroll
                for (int term = 0; term < kB3Terms; ++term)
                    acc[t] = mfma16b(as_b8(a[b3_term_a(term)]), as_b8(b[b3_term_b(term)]), acc[t]);
            }
        } else {
#pragma unroll
            for (int s = 0; s < SPS; ++s) {
                const int off = kDense ? s * 32 : ((s / 3 - 1) * (W + 2) + (s % 3 - 1)) * KS;
                v4f a[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) a[pl] = wsm[(s * 3 + pl) * 64 + lane];
#pragma unroll
                for (int t = 0; t < TN; ++t) {
                    const unsigned short* bp = xp + cb[t] * KS + off + q * 8;
                    v4f b[3];
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) b[pl] = *reinterpret_cast<const v4f*>(bp + pl * PLANE);
#pragma unroll
                    for (int term = 0; term < kB3Terms; ++term)
                        acc[t] = mfma16b(as_b8(a[b3_term_a(term)]), as_b8(b[b3_term_b(term)]), acc[t]);
                }
            }
        }
        if (ch + 1 < nchunk) {
            __syncthreads();                                     // every wave is done reading this stage
            commit();
            __syncthreads();
        }
    }

    // ---- epilogue: conv_mfma_kernel's, statement for statement
    const int C = M / RPC;
    float bv[4], s1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + 4 * q + r;
        bv[r] = bias ? bias[m / RPC] : 0.f;
#pragma unroll
        for (int t = 0; t < TN; ++t) {
            const float v = acc[t][r] + bv[r];
            if (cv[t]) {
                y[(((long)n * B + b0 + cimg[t]) * M + m) * P + cp[t]] = v;
                s1[RPC == 1 ? r : 0] += acc[t][r];
            }
        }
    }
    if (part) {
        constexpr int NS = RPC == 1 ? 4 : 1;                     // channel slots per lane
        __syncthreads();                                         // the A fragments are dead: reuse their LDS
        float* red = reinterpret_cast<float*>(wsm);              // wave sums [4][16] at 0 and 64, means [16] at 128
        auto wg_sum = [&](const float (&s)[4], int base) {       // -> red[base + w * 16 + slot] of every wave
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                float a = s[k];
#pragma unroll
                for (int msk = 1; msk < 16; msk <<= 1) a += __shfl_xor(a, msk);
                if (i16 == 0) red[base + wave * 16 + (RPC == 1 ? 4 * q + k : q)] = a;
            }
        };
        auto waves = [&](int base) { return red[base + tid] + red[base + 16 + tid] + red[base + 32 + tid] + red[base + 48 + tid]; };
        const float cnt = (float)(nimg * P * RPC);               // values of one channel in this workgroup
        wg_sum(s1, 0);
        __syncthreads();
        if (tid < 16 / RPC) red[128 + tid] = waves(0) / cnt;
        __syncthreads();
        float s2[4] = {0.f, 0.f, 0.f, 0.f}, sd[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float mu = red[128 + (RPC == 1 ? 4 * q + r : q)];       // (of the accumulators)
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                const float d = acc[t][r] - mu;
                if (cv[t]) {
                    sd[RPC == 1 ? r : 0] += d;
                    s2[RPC == 1 ? r : 0] = fmaf(d, d, s2[RPC == 1 ? r : 0]);
                }
            }
        }
        wg_sum(sd, 0);
        wg_sum(s2, 64);
        __syncthreads();
        if (tid < 16 / RPC) {
            const float dsum = waves(0), dmean = dsum / cnt;
            float* o = part + (((long)n * chunks + chunk) * C + m0 / RPC + tid) * 2;
            o[0] = (bias ? bias[m0 / RPC + tid] : 0.f) + (red[128 + tid] + dmean);
            o[1] = fmaxf(waves(64) - dsum * dmean, 0.f);
        }
    }
}

// LDS of a workgroup: the stage's A fragments + the activations (planes, or the 11x11 layer's fp32 images)
inline size_t conv_b3_smem_bytes(const ConvGeom& g) {
    const size_t a = (size_t)conv_b3_steps(g) * kB3StepBytes;
    if (g.H == 11) return a + (size_t)3 * g.IB * (g.H + 2) * (g.W + 2) * sizeof(float);
    const size_t npos = g.TAPS == 1 ? g.IB : (size_t)g.IB * (g.H + 2) * (g.W + 2);
    return a + 3 * npos * conv_b3_ks(g.CC) * 2;
}

// pack_b3: the caller's gnnpp_train_pack_b3 buffer of the CURRENT weights
void conv_b3_launch(int l, bool input_grad, const float* x, const void* pack_b3, const float* bias, float* y,
                    float* part, int N, int B, long sn, long sb, hipStream_t st) {
    const ConvGeom g = conv_geom(l, input_grad, B);
    const TrainPackB3Layout PL = train_pack_b3_layout();
    const v4f* wpack = reinterpret_cast<const v4f*>(static_cast<const char*>(pack_b3) + (input_grad ? PL.wtb[l] : PL.wt[l]));
    const dim3 grid(N * g.chunks_per_agent, g.M / 16);
    const size_t smem = conv_b3_smem_bytes(g);
#define GNNPP_CONV_B3(HH, WW)                                                                                  \
    do {                                                                                                       \
        static LdsAttrOnce once;                               /* (the 5x5 and dense stages use 75 KB of LDS) */ \
        set_lds_attr_once(once, reinterpret_cast<const void*>(&conv_b3_kernel<HH, WW>), (int)smem);            \
        hipLaunchKernelGGL((conv_b3_kernel<HH, WW>), grid, dim3(256), smem, st, x, wpack, bias, y, part, B,    \
                           g.Ck, g.M, sn, sb, g.chunks_per_agent, g.nchunk);                                   \
    } while (0)
    if (g.H == 11) GNNPP_CONV_B3(11, 11);
    else if (g.H == 5) GNNPP_CONV_B3(5, 5);
    else GNNPP_CONV_B3(1, 1);
#undef GNNPP_CONV_B3
}

}  // namespace gnnpp
