// gnnpp_rollout_lists: the communication graph of rollout_team_gso_kernel, delivered as the per-column neighbour
// lists the team filter gathers from (team_layout of lsigf_team_kernel.hip: cnt | idx | val, graphs = B) instead of
// the N^2 floats of a dense S.  Any 1 <= N <= GNNPP_ROLLOUT_MAX_TEAM.
//
// One workgroup per episode, thread t = agent t = column t (the relation is symmetric: column t is row t).  The same
// statement as rollout_team_gso_kernel -- the same dist2_bound, the same /= 1.1 then *= 1.1 growth sequence,
// inv = sqrt(1.0 / deg) in fp64, weight (float)(inv[i] * inv[n]) -- in the order the lists invite:
//   1. the positions go to LDS;
//   2. thread t scans i = 0 .. N-1 in ascending order (every thread reads the same cell: an LDS broadcast) and
//      writes its own index list, four uint16 per 8-byte store; cnt is the degree.  The last, partial store carries
//      zeros behind the entries: the padding of the indices;
//   3. connectivity: level-synchronous search from node 0 over the LISTS: an unreached thread tests its own cnt
//      neighbours against the frontier's bit set in LDS, sixteen independent tests per trip.  With grow = 1 the lists
//      are rebuilt only when the integer threshold changes;
//   4. inv[] in LDS, a barrier, then thread t walks its list once more and writes val, 16 bytes per store, zeros in
//      the padding.
// A thread reads back only the indices it wrote itself.  No atomics, one writer per element: two calls give the same
// bytes.  Included from gnnpp_api.hip after rollout_team_kernels.hip and lsigf_team_kernel.hip.

namespace gnnpp {

// size of a lists block: the head of the team workspace (K > 1, one graph per `graphs`)
inline size_t team_lists_bytes(int graphs, int N) { return team_layout(graphs, N, 1, 2, 1, 1).z; }

// bit m of an N-bit agent set, read as 32-bit words
__device__ __forceinline__ bool team_bit(const unsigned* set, unsigned m) { return (set[m >> 5] >> (m & 31)) & 1u; }

__global__ __launch_bounds__(1024) void rollout_team_lists_kernel(const RolloutArgs p, int grow, int* cnt_out,
                                                                  unsigned short* idx_out, float* val_out, int Np) {
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    typedef int v2i __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int N = p.N, b = blockIdx.x, t = threadIdx.x, nw = blockDim.x >> 6;
    v2i* pl = reinterpret_cast<v2i*>(gnnpp_smem);                                   // [N] (row, col)
    double* inv = reinterpret_cast<double*>(gnnpp_smem + round16((size_t)8 * N));   // [N]
    unsigned long long* fr[2] = {reinterpret_cast<unsigned long long*>(inv + N), nullptr};
    fr[1] = fr[0] + kTeamWords;
    unsigned long long* words = fr[1] + kTeamWords;                                 // [kTeamWords]
    const int* pos = p.pos + (size_t)b * N * 2;
    const bool live = t < N;
    const size_t lcol = (size_t)b * N + (live ? t : 0);
    unsigned short* il = idx_out + lcol * Np;                                       // 8-byte aligned (Np % 4 == 0)
    float* wl = val_out + lcol * Np;                                                // 16-byte aligned
    int mx = 0, my = 0;
    if (live) {
        mx = pos[2 * t]; my = pos[2 * t + 1];
        v2i q; q[0] = mx; q[1] = my;
        pl[t] = q;
    }
    __syncthreads();
    double r = p.radius[b];
    if (grow) r = r / 1.1;
    unsigned Tu = 0u;
    int cnt = 0;
    bool built = false, connected = false;
    // Termination with grow: as in rollout_team_gso_kernel (the bound reaches 65535^2, the largest d2 of two cells).
    for (;;) {
        if (grow) r = r * 1.1;
        const unsigned Tn = dist2_bound(r);              // d2 < 2^32 - 1: a map of 65 536 cells can be 1 x 65 536
        if (!built || Tn != Tu) {                        // (workgroup-uniform)
            Tu = Tn;
            built = true;
            cnt = 0;
            if (live) {
                unsigned long long pk = 0ull;            // the last four entries, the newest in the top 16 bits
#pragma unroll 4
                for (int i = 0; i < N; ++i) {
                    const v2i q = pl[i];
                    if (i != t && dist2(q[0], q[1], mx, my) <= Tu) {
                        pk = (pk >> 16) | ((unsigned long long)i << 48);
                        ++cnt;
                        if ((cnt & 3) == 0) {
                            v2u w; w[0] = (unsigned)pk; w[1] = (unsigned)(pk >> 32);
                            *reinterpret_cast<v2u*>(il + cnt - 4) = w;
                        }
                    }
                }
                if (cnt & 3) {                           // the tail and, behind it, the zeros of the padding
                    pk >>= 16 * (4 - (cnt & 3));
                    v2u w; w[0] = (unsigned)pk; w[1] = (unsigned)(pk >> 32);
                    *reinterpret_cast<v2u*>(il + (cnt & ~3)) = w;
                }
            }
        }
        bool in_r = t == 0;                              // reached set; the frontier starts as {0}
        int cur = 0;
        {
            const unsigned long long m = __ballot(in_r);
            if ((t & 63) == 0) fr[0][t >> 6] = m;
        }
        __syncthreads();
        for (;;) {
            bool join = false;
            if (live && !in_r) {
                const unsigned* f32 = reinterpret_cast<const unsigned*>(fr[cur]);
                for (int d = 0; d < cnt && !join; d += 16) {
                    v2u pk[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {        // (a group behind the list is not read: it may lie past the block)
                        v2u z; z[0] = 0u; z[1] = 0u;
                        pk[u] = d + 4 * u < cnt ? *reinterpret_cast<const v2u*>(il + d + 4 * u) : z;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {        // (the padding's index 0 is not a neighbour)
                        const int e = d + 4 * u;
                        join |= e < cnt && team_bit(f32, pk[u][0] & 0xffffu);
                        join |= e + 1 < cnt && team_bit(f32, pk[u][0] >> 16);
                        join |= e + 2 < cnt && team_bit(f32, pk[u][1] & 0xffffu);
                        join |= e + 3 < cnt && team_bit(f32, pk[u][1] >> 16);
                    }
                }
            }
            in_r |= join;
            const unsigned long long m = __ballot(join);
            if ((t & 63) == 0) fr[cur ^ 1][t >> 6] = m;
            __syncthreads();
            bool any = false;
            for (int w = 0; w < nw; ++w) any |= fr[cur ^ 1][w] != 0ull;
            cur ^= 1;                                    // (the old frontier is rewritten only after a barrier)
            if (!any) break;
        }
        connected = !team_any(live && !in_r, words, t, nw);
        if (connected || !grow) break;
    }
    if (live) inv[t] = inv_sqrt_degree(cnt);
    __syncthreads();
    if (live) {
        cnt_out[lcol] = cnt;
        const double it = inv[t];
        for (int d = 0; d < cnt; d += 4) {
            const v2u pk = *reinterpret_cast<const v2u*>(il + d);
            const unsigned m[4] = {pk[0] & 0xffffu, pk[0] >> 16, pk[1] & 0xffffu, pk[1] >> 16};
            v4f w;
#pragma unroll
            for (int u = 0; u < 4; ++u) w[u] = d + u < cnt ? (float)(inv[m[u]] * it) : 0.f;
            *reinterpret_cast<v4f*>(wl + d) = w;
        }
    }
    if (t == 0) {
        p.radius[b] = r;
        if (p.connected) p.connected[b] = connected;
    }
}

// rollout_team_lists_kernel as a device body, for the streamed seat of rollout_team_stream_kernels.hip: the same statement,
// the same order of operations, the same stores.  Thread t of nt = team_threads(N), every thread of the workgroup calls it,
// `smem` = team_gso_smem(N) bytes of LDS.  Reads pos[b] and radius[b]; writes columns [b * N, (b + 1) * N) of the block,
// radius[b], connected[b].  The kernel above keeps its own text: called through this body it measured 2.6 % slower at
// 8 x 1024 agents, so only the new kernel calls it.  A change to one is a change to both; the streamed
// seat's tests hold the body to the kernel bit for bit.
__device__ __forceinline__ void team_lists_body(const RolloutArgs& p, int b, int t, int nt, int grow, char* smem,
                                                int* cnt_out, unsigned short* idx_out, float* val_out, int Np) {
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    typedef int v2i __attribute__((ext_vector_type(2)));
    const int N = p.N, nw = nt >> 6;
    v2i* pl = reinterpret_cast<v2i*>(smem);                                         // [N] (row, col)
    double* inv = reinterpret_cast<double*>(smem + round16((size_t)8 * N));         // [N]
    unsigned long long* fr[2] = {reinterpret_cast<unsigned long long*>(inv + N), nullptr};
    fr[1] = fr[0] + kTeamWords;
    unsigned long long* words = fr[1] + kTeamWords;                                 // [kTeamWords]
    const int* pos = p.pos + (size_t)b * N * 2;
    const bool live = t < N;
    const size_t lcol = (size_t)b * N + (live ? t : 0);
    unsigned short* il = idx_out + lcol * Np;                                       // 8-byte aligned (Np % 4 == 0)
    float* wl = val_out + lcol * Np;                                                // 16-byte aligned
    int mx = 0, my = 0;
    if (live) {
        mx = pos[2 * t]; my = pos[2 * t + 1];
        v2i q; q[0] = mx; q[1] = my;
        pl[t] = q;
    }
    __syncthreads();
    double r = p.radius[b];
    if (grow) r = r / 1.1;
    unsigned Tu = 0u;
    int cnt = 0;
    bool built = false, connected = false;
    // Termination with grow: as in rollout_team_gso_kernel (the bound reaches 65535^2, the largest d2 of two cells).
    for (;;) {
        if (grow) r = r * 1.1;
        const unsigned Tn = dist2_bound(r);              // d2 < 2^32 - 1: a map of 65 536 cells can be 1 x 65 536
        if (!built || Tn != Tu) {                        // (workgroup-uniform)
            Tu = Tn;
            built = true;
            cnt = 0;
            if (live) {
                unsigned long long pk = 0ull;            // the last four entries, the newest in the top 16 bits
#pragma unroll 4
                for (int i = 0; i < N; ++i) {
                    const v2i q = pl[i];
                    if (i != t && dist2(q[0], q[1], mx, my) <= Tu) {
                        pk = (pk >> 16) | ((unsigned long long)i << 48);
                        ++cnt;
                        if ((cnt & 3) == 0) {
                            v2u w; w[0] = (unsigned)pk; w[1] = (unsigned)(pk >> 32);
                            *reinterpret_cast<v2u*>(il + cnt - 4) = w;
                        }
                    }
                }
                if (cnt & 3) {                           // the tail and, behind it, the zeros of the padding
                    pk >>= 16 * (4 - (cnt & 3));
                    v2u w; w[0] = (unsigned)pk; w[1] = (unsigned)(pk >> 32);
                    *reinterpret_cast<v2u*>(il + (cnt & ~3)) = w;
                }
            }
        }
        bool in_r = t == 0;                              // reached set; the frontier starts as {0}
        int cur = 0;
        {
            const unsigned long long m = __ballot(in_r);
            if ((t & 63) == 0) fr[0][t >> 6] = m;
        }
        __syncthreads();
        for (;;) {
            bool join = false;
            if (live && !in_r) {
                const unsigned* f32 = reinterpret_cast<const unsigned*>(fr[cur]);
                for (int d = 0; d < cnt && !join; d += 16) {
                    v2u pk[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {        // (a group behind the list is not read: it may lie past the block)
                        v2u z; z[0] = 0u; z[1] = 0u;
                        pk[u] = d + 4 * u < cnt ? *reinterpret_cast<const v2u*>(il + d + 4 * u) : z;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {        // (the padding's index 0 is not a neighbour)
                        const int e = d + 4 * u;
                        join |= e < cnt && team_bit(f32, pk[u][0] & 0xffffu);
                        join |= e + 1 < cnt && team_bit(f32, pk[u][0] >> 16);
                        join |= e + 2 < cnt && team_bit(f32, pk[u][1] & 0xffffu);
                        join |= e + 3 < cnt && team_bit(f32, pk[u][1] >> 16);
                    }
                }
            }
            in_r |= join;
            const unsigned long long m = __ballot(join);
            if ((t & 63) == 0) fr[cur ^ 1][t >> 6] = m;
            __syncthreads();
            bool any = false;
            for (int w = 0; w < nw; ++w) any |= fr[cur ^ 1][w] != 0ull;
            cur ^= 1;                                    // (the old frontier is rewritten only after a barrier)
            if (!any) break;
        }
        connected = !team_any(live && !in_r, words, t, nw);
        if (connected || !grow) break;
    }
    if (live) inv[t] = inv_sqrt_degree(cnt);
    __syncthreads();
    if (live) {
        cnt_out[lcol] = cnt;
        const double it = inv[t];
        for (int d = 0; d < cnt; d += 4) {
            const v2u pk = *reinterpret_cast<const v2u*>(il + d);
            const unsigned m[4] = {pk[0] & 0xffffu, pk[0] >> 16, pk[1] & 0xffffu, pk[1] >> 16};
            v4f w;
#pragma unroll
            for (int u = 0; u < 4; ++u) w[u] = d + u < cnt ? (float)(inv[m[u]] * it) : 0.f;
            *reinterpret_cast<v4f*>(wl + d) = w;
        }
    }
    if (t == 0) {
        p.radius[b] = r;
        if (p.connected) p.connected[b] = connected;
    }
}

// `lists`: a block of team_lists_bytes(a.B, a.N) bytes, 16-byte aligned (validated by the caller)
int rollout_team_lists_launch(const RolloutArgs& a, int grow, void* lists, hipStream_t st) {
    const TeamLayout L = team_layout(a.B, a.N, 1, 2, 1, 1);
    char* base = static_cast<char*>(lists);
    hipLaunchKernelGGL(rollout_team_lists_kernel, dim3(a.B), dim3(team_threads(a.N)), team_gso_smem(a.N), st, a, grow,
                       reinterpret_cast<int*>(base + L.cnt), reinterpret_cast<unsigned short*>(base + L.idx),
                       reinterpret_cast<float*>(base + L.val), L.Np);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace gnnpp
