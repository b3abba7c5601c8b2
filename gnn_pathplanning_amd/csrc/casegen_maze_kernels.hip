// The reference's maze maps on the device, bit for bit (include/gnnpp_casegen_maze.h): numpy's legacy
// MT19937 stream and randint's masked rejection, and the sequential wall walk of CasesGen.mapGen on top of them.
//
// casegen_maze_kernel    one WAVE per map (a map is one sequential walk: the parallelism is across maps), kMazeWaves waves
//     per workgroup that share nothing -- the kernel has no workgroup barrier, and a wave past the last map leaves at once.
//     Per wave in LDS: the map as a bit grid in the word layout of casegen_kernel / mapf_team_kernels.hip (a row is WR =
//     ceil(W / 64) words, word j of row y at y * WR + j, bit x & 63), the 624 state words, and a block of 624 tempered words.
//     Seeding is a chain of 623 dependent steps; the seed is wave-uniform, so the chain runs once per wave on the scalar
//     unit, each lane keeps the words of its own index and the state is stored 64 words at a time.
//     Refill: the twist is word k <- f(mt[k], mt[k + 1], mt[k + 397 mod 624]); it runs across the lanes in three phases,
//     k < 227 (reads old words only), 227 <= k < 454 (reads the new words k - 227 of the first phase) and k >= 454 (the new
//     words of the second, and for k = 623 the new mt[0]).  Inside a phase every read comes before every write; each phase
//     stores its state words and their tempered form.
//     Walk: lane 0 alone, as a state machine in registers that takes at most one word per trip: (wall, step, x, y) and
//     which draw is pending -- the wall's column, its row, or a step's neighbour pick.  A rejected word leaves the state
//     as it is.  When the block is spent the lane leaves the loop, the wave refills, and the walk resumes where it was.
//     Hand-offs (state -> walking lane, walking lane -> the byte writers) are ordered by wave barriers in wave-uniform
//     control flow, never by an assumption about lanes running in step; the exit test is lane 0's flag read by every lane.
//     Output: the wave turns the bit grid into bytes, 16 per lane and store (the bytes before the first and after the last
//     16-byte boundary of the map one by one): every byte of the map is written, by one lane.
#include "../../include/gnnpp_casegen_maze.h"
#include "gnnpp_common.h"

namespace gnnpp {

constexpr int kMazeWaves = 4;                   // waves (maps) of a workgroup
constexpr int kMtWords = 624, kMtShift = 397, kMtPhase = kMtWords - kMtShift;     // 227: the length of a refill phase

struct CasegenMazeArgs {
    const unsigned* seeds;
    unsigned seed0;
    int C, H, W, walls, steps;
    unsigned char* grid;
    int* words;
};

// LDS of one wave: bits [H * WR] u64 | mt [624] u32 | out [624] u32
__host__ __device__ inline size_t casegen_maze_wave_bytes(int H, int W) { return (size_t)H * ((W + 63) >> 6) * 8 + 2 * kMtWords * 4; }

__device__ __forceinline__ unsigned maze_temper(unsigned y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    return y ^ (y >> 18);
}

// The next 624 words: mt twisted in place, out = their tempered form.  Every lane of the wave takes part.
__device__ __forceinline__ void maze_refill(unsigned* mt, unsigned* out, int lane) {
    for (int ph = 0; ph < 3; ++ph) {
        const int k0 = ph * kMtPhase, k1 = ph == 2 ? kMtWords : k0 + kMtPhase;
        unsigned v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + 64 * r + lane;
            v[r] = 0u;
            if (k < k1) {
                const unsigned y = (mt[k] & 0x80000000u) | (mt[k + 1 == kMtWords ? 0 : k + 1] & 0x7fffffffu);
                v[r] = mt[k < kMtPhase ? k + kMtShift : k - kMtPhase] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
        }
        __builtin_amdgcn_wave_barrier();                 // all reads of a phase precede its writes
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + 64 * r + lane;
            if (k < k1) {
                mt[k] = v[r];
                out[k] = maze_temper(v[r]);
            }
        }
        __builtin_amdgcn_wave_barrier();                 // the phase's words precede the next phase's (the walk's) reads
    }
}

__global__ __launch_bounds__(kMazeWaves * 64) void casegen_maze_kernel(const CasegenMazeArgs p) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long c = (long long)blockIdx.x * kMazeWaves + wave;
    if (c >= p.C) return;                                // (the whole wave; nothing below waits for another wave)
    const int H = p.H, W = p.W, WR = (W + 63) >> 6, HW = H * WR, walls = p.walls, steps = p.steps;
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(gnnpp_smem + (size_t)wave * casegen_maze_wave_bytes(H, W));
    unsigned* mt = reinterpret_cast<unsigned*>(bits + HW);
    unsigned* out = mt + kMtWords;

    for (int i = lane; i < HW; i += 64) bits[i] = 0ull;
    // ---- init_genrand(seed): mt[0] = seed, mt[i] = 1812433253 * (mt[i-1] ^ (mt[i-1] >> 30)) + i ---------------------------
    unsigned sx = p.seeds != nullptr ? p.seeds[c] : p.seed0 + (unsigned)c;
    for (int b = 0; b < kMtWords; b += 64) {
        unsigned mine = 0u;
#pragma unroll 1
        for (int j = 0; j < 64; j += 16) {               // (16 steps unrolled: their words stay in scalar registers)
            const int rel = lane - j;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (e == rel) mine = sx;
                sx = 1812433253u * (sx ^ (sx >> 30)) + (unsigned)(b + j + e + 1);
            }
        }
        if (b + lane < kMtWords) mt[b + lane] = mine;
    }
    __builtin_amdgcn_wave_barrier();                     // the cleared map precedes lane 0's first cell

    // ---- the walk (lane 0), a refill (the wave) whenever the block is spent -------------------------------------------
    int wall = 0, step = -2, x = 0, y = 0;               // step: -2 the column is pending, -1 the row, >= 0 a pick
    int at = kMtWords, nwords = 0, done = 0;             // the first word needs a refill, as in numpy
    for (;;) {
        if (lane == 0) {
            for (;;) {
                if (step >= steps) {                     // (the column and the row are never behind `steps` >= 0)
                    ++wall;
                    step = -2;
                }
                if (wall >= walls) {
                    done = 1;
                    break;
                }
                int rng, nl = 0, nr = 0, nu = 0, nd = 0;
                if (step == -2) {
                    rng = (W >> 1) - 1;
                } else if (step == -1) {
                    rng = (H >> 1) - 1;
                } else {
                    nl = x > 1;
                    nr = x < W - 2;
                    nu = y > 1;
                    nd = y < H - 2;
                    rng = nl + nr + nu + nd - 2;         // randint(0, len - 1): 0 .. len - 2
                }
                unsigned v = 0u;
                if (rng > 0) {                           // rng == 0 draws no word
                    if (at == kMtWords) break;           // the block is spent
                    unsigned mask = (unsigned)rng;       // rng <= 127
                    mask |= mask >> 1;
                    mask |= mask >> 2;
                    mask |= mask >> 4;
                    v = out[at++] & mask;
                    ++nwords;
                    if (v > (unsigned)rng) continue;     // rejected: the same draw again
                }
                if (step == -2) {
                    x = 2 * (int)v;
                    step = -1;
                } else if (step == -1) {
                    y = 2 * (int)v;
                    bits[y * WR + (x >> 6)] |= 1ull << (x & 63);
                    step = 0;
                } else {
                    int k = (int)v, nx = x, ny = y;      // entry v of the list left, right, up, down
                    if (nl) { if (k == 0) nx = x - 2; --k; }
                    if (nr) { if (k == 0) nx = x + 2; --k; }
                    if (nu) { if (k == 0) ny = y - 2; --k; }
                    if (nd) { if (k == 0) ny = y + 2; --k; }
                    unsigned long long* cell = bits + ny * WR + (nx >> 6);
                    if (((*cell >> (nx & 63)) & 1ull) == 0ull) {
                        *cell |= 1ull << (nx & 63);
                        const int mx = (x + nx) >> 1, my = (y + ny) >> 1;
                        bits[my * WR + (mx >> 6)] |= 1ull << (mx & 63);
                        x = nx;
                        y = ny;
                    }
                    ++step;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();                 // lane 0's cells precede the byte writers' reads
        if (__builtin_amdgcn_readlane(done, 0) != 0) break;
        maze_refill(mt, out, lane);
        at = 0;
    }
    if (lane == 0 && p.words != nullptr) p.words[c] = nwords;

    // ---- grid: bits -> bytes ------------------------------------------------------------------------------------------
    const int cells = H * W;
    unsigned char* g = p.grid + (size_t)c * cells;
    const int head = min(cells, (int)((16u - (unsigned)(reinterpret_cast<size_t>(g) & 15u)) & 15u));
    const int nvec = (cells - head) >> 4, tail = head + 16 * nvec;
    {                                                    // at most 15 bytes in front and 15 behind: one lane each
        const int q = lane < head ? lane : tail + lane - head;
        if (q < cells) {
            const int yy = q / W, xx = q - yy * W;
            g[q] = (unsigned char)((bits[yy * WR + (xx >> 6)] >> (xx & 63)) & 1ull);
        }
    }
    for (int i = lane; i < nvec; i += 64) {
        const int q = head + 16 * i;
        int yy = q / W, xx = q - yy * W;
        unsigned long long word = bits[yy * WR + (xx >> 6)];
        unsigned b4[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            b4[b >> 2] |= (unsigned)((word >> (xx & 63)) & 1ull) << (8 * (b & 3));
            if (++xx == W) {
                xx = 0;
                ++yy;
            }
            if ((xx & 63) == 0 && yy < H) word = bits[yy * WR + (xx >> 6)];
        }
        const v4u bytes = {b4[0], b4[1], b4[2], b4[3]};
        *reinterpret_cast<v4u*>(g + q) = bytes;
    }
}

// GNNPP_OK or GNNPP_ERR_LAUNCH (arguments checked by gnnpp_casegen_maze)
int casegen_maze_launch(const CasegenMazeArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(casegen_maze_kernel, dim3((unsigned)(((long long)a.C + kMazeWaves - 1) / kMazeWaves)), dim3(kMazeWaves * 64),
                       kMazeWaves * casegen_maze_wave_bytes(a.H, a.W), st, a);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

}  // namespace gnnpp
