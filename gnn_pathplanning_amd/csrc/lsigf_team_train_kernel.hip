// Training on neighbour lists for TEAM graphs of up to 1024 nodes (gfx950): what the backward pass of the team filter
// (lsigf_team_kernel.hip) needs beyond the forward kernels.
//
//   1. team_transpose_kernel (gnnpp_team_lists_transpose): the lists of S^T from the lists of S, in the same
//      cnt | idx | val format.  The input gradient of the filter is the filter on S^T:
//      dx = sum_k W_k^T . dy . (S^T)^k.  The structure of team_lists_kernel: a workgroup owns a strip of 16 OUTPUT
//      columns [m0, m0 + 16) of one graph; a lane owns an INPUT column n, the workgroup's four waves a quarter of the
//      input columns each, in ascending n.  List(n) is sorted, so a lower-bound search finds its at most 16 entries
//      inside the strip; per strip column a ballot + prefix popcount gives every hit its slot, behind the hits of the
//      waves before (counted in a first pass, exchanged through LDS).  Output column m therefore holds every n with m in
//      list(n) in ascending n with the same weight, then (0, 0.0f) up to a multiple of four entries.  No dense matrix.
//   2. team_save_shift_kernel + team_tail_saved_kernel (gnnpp_lsigf_team_lists_fwd_save): the forward that KEEPS every
//      tap signal z_{e,k} in zs [E*K][B*N][G] (node-major, row stride G: the layout gnnpp_lsigf_fwd_save documents and
//      the tap-gradient GEMM reads).  One shift launch per k = 1 .. K-1 (the first also copies x into tap (e, 0)), each
//      the same team_gather chain as team_shift_kernel; the tail (team_tail_body<.., SAVED>) stages all K taps as
//      copies from zs.  Same gather order, contraction, bias and ReLU: y has the bytes of gnnpp_lsigf_team_lists_fwd.
//   3. gnnpp_lsigf_team_lists_input_grad is team_launch itself on (dy, lists of S^T, taps of h.permute(3,1,2,0)) with
//      the exact fp32 MFMA contraction: no kernel of its own.
//
// No atomics, no allocation, no host synchronisation, one writer per element: two calls give the same bytes.  Nothing
// but launches.  Included from gnnpp_api.hip after lsigf_team_kernel.hip.

namespace gnnpp {

struct TeamTransposeArgs {
    const int* cnt; const unsigned short* idx; const float* val;       // lists of S
    int* cnt_t; unsigned short* idx_t; float* val_t;                   // lists of S^T
    int N, Np;
};

// ---- 1. lists of S -> lists of S^T ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void team_transpose_kernel(const TeamTransposeArgs p) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    int* wcnt = reinterpret_cast<int*>(gnnpp_smem);               // [4 waves][16 strip columns]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = p.N, Np = p.Np;
    const int strips = (N + 15) >> 4;
    const int g = blockIdx.x / strips, m0 = (blockIdx.x - g * strips) * 16;
    const int Q = (((N + 3) >> 2) + 63) & ~63;                    // input columns per wave: a multiple of 64, <= 256
    const int chunks = Q >> 6;                                     // <= 4, workgroup-uniform
    const size_t gbase = (size_t)g * N;
    const unsigned long long below = (1ull << lane) - 1ull;

    // pass 1: per chunk, where list(n) enters the strip and which of the strip's 16 rows it holds
    int lo[4];
    unsigned has[4];
    int mine[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) mine[c] = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        lo[s] = 0; has[s] = 0u;
        if (s < chunks) {
            const int n = wave * Q + s * 64 + lane;
            if (n < N) {
                int deg = p.cnt[gbase + n];
                deg = deg < 0 ? 0 : (deg > N ? N : deg);
                const unsigned short* il = p.idx + (gbase + n) * Np;
                int a = 0, b = deg;                                // lower bound of m0 in il[0 .. deg)
                while (a < b) {
                    const int mid = (a + b) >> 1;
                    if ((int)il[mid] < m0) a = mid + 1; else b = mid;
                }
                lo[s] = a;
                for (int j = a; j < deg && j < a + 16; ++j) {
                    const int d = (int)il[j] - m0;
                    if (d < 0 || d >= 16) break;
                    has[s] |= 1u << d;
                }
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) mine[c] += __popcll(__ballot((has[s] >> c) & 1u));
        }
    }
    if (lane < 16) {
        int v = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) v = lane == c ? mine[c] : v;
        wcnt[wave * 16 + lane] = v;
    }
    __syncthreads();

    // pass 2: every hit goes to its slot of output column m0 + c
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int m = m0 + c;
        int pos = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int k = wcnt[w * 16 + c];
            if (w < wave) pos += k;
            total += k;
        }
        const size_t ocol = (gbase + (m < N ? m : 0)) * Np;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (s < chunks) {
                const bool hit = (has[s] >> c) & 1u;
                const unsigned long long bal = __ballot(hit);
                const int slot = pos + __popcll(bal & below);
                if (hit && m < N && slot < Np) {
                    const int n = wave * Q + s * 64 + lane;
                    p.idx_t[ocol + slot] = (unsigned short)n;
                    p.val_t[ocol + slot] = p.val[(gbase + n) * Np + lo[s] + __popc(has[s] & ((1u << c) - 1u))];
                }
                pos += __popcll(bal);
            }
        if (wave == 0 && m < N) {
            if (total > N) total = N;                              // (cannot happen on valid lists)
            if (lane == 0) p.cnt_t[gbase + m] = total;
            const int slot = total + lane;                         // padding to a multiple of four entries (<= 3)
            if (lane < 3 && slot < ((total + 3) & ~3)) { p.idx_t[ocol + slot] = 0; p.val_t[ocol + slot] = 0.f; }
        }
    }
}

int team_transpose_launch(const void* lists, void* lists_t, int graphs, int N, hipStream_t st) {
    const TeamLayout L = team_layout(graphs, N, 1, 2, 1, 1);
    const char* in = static_cast<const char*>(lists);
    char* out = static_cast<char*>(lists_t);
    TeamTransposeArgs a;
    a.cnt = reinterpret_cast<const int*>(in + L.cnt);
    a.idx = reinterpret_cast<const unsigned short*>(in + L.idx);
    a.val = reinterpret_cast<const float*>(in + L.val);
    a.cnt_t = reinterpret_cast<int*>(out + L.cnt);
    a.idx_t = reinterpret_cast<unsigned short*>(out + L.idx);
    a.val_t = reinterpret_cast<float*>(out + L.val);
    a.N = N; a.Np = L.Np;
    hipLaunchKernelGGL(team_transpose_kernel, dim3(graphs * ((N + 15) / 16)), dim3(256), 4 * 16 * sizeof(int), st, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---- 2. the forward that keeps the tap signals ----------------------------------------------------------------------
// one shift z_{e,k-1} -> z_{e,k} inside zs (p.z), 1 <= k <= K-1: team_shift_kernel's half wave per node and gather chain.
// k == 1 reads x and also writes its copy, tap (e, 0); k == 0 (the launch of a K = 1 filter) only copies.
__global__ __launch_bounds__(256) void team_save_shift_kernel(const TeamArgs p, int k, int zs_vec) {
    const int tid = threadIdx.x, hl = tid & 31;
    const size_t node = (size_t)blockIdx.x * 8 + (tid >> 5);      // (e, b, n)
    const size_t per_e = (size_t)p.B * p.N;
    if (node >= per_e * p.E) return;
    const int e = (int)(node / per_e);
    const int bn = (int)(node - (size_t)e * per_e);
    const int b = bn / p.N, n = bn - b * p.N;
    const int col = 4 * hl, G = p.G;
    auto store = [&](int tap, const v4f& v) {
        float* dst = p.z + (((size_t)tap * p.B + b) * p.N + n) * G + col;
        if (zs_vec) {
            if (col < G) *reinterpret_cast<v4f*>(dst) = v;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (col + u < G) dst[u] = v[u];
        }
    };
    const float* xg = p.x + (size_t)b * p.N * G;
    if (k <= 1) store(e * p.K, team_load4(xg + (size_t)n * G, col, G, p.x_vec != 0));
    if (k == 0) return;
    const float* src = k == 1 ? xg : p.z + ((size_t)(e * p.K + k - 1) * p.B + b) * p.N * G;
    const size_t lcol = ((size_t)(p.s_batched ? b : 0) * p.E + e) * p.N + n;
    store(e * p.K + k, team_gather(p.idx + lcol * p.Np, p.val + lcol * p.Np, p.cnt[lcol], src, G, col, G,
                                   k == 1 ? p.x_vec != 0 : zs_vec != 0));
}

template <int RT, int MODE>
__global__ __launch_bounds__(256) void team_tail_saved_kernel(const TeamArgs p) {
    team_tail_body<RT, MODE, true>(p);
}

template <int RT, int MODE>
static hipError_t team_tail_saved_launch(const TeamArgs& a, hipStream_t st) {
    constexpr int R = 16 * RT;
    constexpr size_t smem = 2 * (size_t)(MODE == 2 ? R * kTeamPRow : R * kTeamZs * 4) + 8 * R * 8 * sizeof(float);
    const int tiles = (a.N + R - 1) / R;
    hipLaunchKernelGGL((team_tail_saved_kernel<RT, MODE>), dim3(a.B * tiles), dim3(256), smem, st, a);
    return hipGetLastError();
}

// `a` as for team_launch (validated by the caller); lists: the caller's block (nullptr at K = 1); zs [E*K][B*N][G].
int team_save_launch(TeamArgs a, const void* lists, float* zs, int precision, hipStream_t st) {
    const TeamLayout L = team_layout(a.B, a.N, a.G, a.K, a.E, a.s_batched);
    char* lb = static_cast<char*>(const_cast<void*>(lists));      // (read only)
    a.cnt = reinterpret_cast<int*>(lb + L.cnt);
    a.idx = reinterpret_cast<unsigned short*>(lb + L.idx);
    a.val = reinterpret_cast<float*>(lb + L.val);
    a.z = zs;
    a.Np = L.Np; a.Gz = L.Gz;
    a.NG = (a.G + 15) / 16; a.KB = (a.G + 31) / 32; a.MT = (a.F + 15) / 16;
    a.wpk_b = a.wpk + filter_packed_b3_offset(a.G, a.F, a.K, a.E);
    a.x_vec = (a.G & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
    a.y_vec = a.y && (a.F & 3) == 0 && (reinterpret_cast<uintptr_t>(a.y) & 15) == 0;
    const int zs_vec = (a.G & 3) == 0 && (reinterpret_cast<uintptr_t>(zs) & 15) == 0;
    const size_t nodes = (size_t)a.E * a.B * a.N;
    for (int k = a.K > 1 ? 1 : 0; k < a.K; ++k) {
        hipLaunchKernelGGL(team_save_shift_kernel, dim3((unsigned)((nodes + 7) / 8)), dim3(256), 0, st, a, k, zs_vec);
        if (hipGetLastError() != hipSuccess) return -3;
    }
    a.x_vec = zs_vec;                                              // the tail reads zs only (team_tail_body<.., SAVED>)
    const bool wide = (size_t)a.B * ((a.N + 31) / 32) >= 256;      // team_launch's rule
    hipError_t err;
    if (precision == kPrecFp32Mfma) err = wide ? team_tail_saved_launch<2, 1>(a, st) : team_tail_saved_launch<1, 1>(a, st);
    else err = wide ? team_tail_saved_launch<2, 2>(a, st) : team_tail_saved_launch<1, 2>(a, st);
    return err == hipSuccess ? 0 : -3;
}

}  // namespace gnnpp
