// The communication graph of a set of agent positions: its arithmetic, stated once for every kernel that builds one, and
// the ONE-WAVE form of the build (N <= 128: lane l holds agents l and l + 64, adjacency rows as 128-bit masks in
// registers), which rollout_kernels.hip and expert_kernels.hip call and give their own thread mappings and stores.
//
// The statement (multiRobotSim.computeAdjacencyMatrix, utils/multirobotsim_dcenlocal.py:320-365):
//   * A_ij = (pdist_ij < R), zero diagonal (:338-339, :354-355).  Positions are integers, so the test is the integer
//     one d2_ij <= dist2_bound(R) -- dist2_threshold evaluates the reference's fp64 comparison once per radius;
//   * at step 0 R /= 1.1 once, then R *= 1.1 until the graph is connected (:334-340): rollout_radius_search.  The
//     expert transformers (DataTransformer_local_onlineExpert.py) start at radius0 and count the multiplications:
//     expert_radius_search.  Both repeat the fp64 multiplication, so the radius carries the reference's bits;
//   * connected <=> a level-synchronous search from node 0 reaches all N nodes -- the same boolean as the reference's
//     Laplacian-spectrum test (graph.isConnected, :340, :356): wave_connected;
//   * inv_i = deg_i ? sqrt(1.0 / deg_i) : 0.0 in fp64 (:342-346): inv_sqrt_degree;
//   * S_ij = A_ij ? (float)(inv_i * inv_j) : 0 (:347-348, then the `S.float()` of the planner): gso_store_S.
//
// The thread-per-agent kernels (N <= 1024: rollout_team_kernels.hip, rollout_team_lists_kernel.hip,
// expert_team_kernels.hip, expert_team_lists_kernel.hip) take dist2 / dist2_bound / inv_sqrt_degree from here and keep
// their own search and growth loops over N-bit frontier sets in LDS.
// Everything here is inlined into its callers; nothing adds LDS or a barrier.
#include "../../include/gnnpp.h"
#include "gnnpp_common.h"

namespace gnnpp {

constexpr int kMaxAgents = GNNPP_ROLLOUT_MAX_AGENTS;    // one-wave form
constexpr int kGrowthCap = 0xffff;            // expert step_info keeps k_t in 16 bits (1.1^65535 overflows fp64 long before)

typedef ::gnnpp_rollout RolloutArgs;      // the C-ABI struct itself (include/gnnpp.h)

// ---- common to every kernel ---------------------------------------------------------------------------------------
// Largest integer d2 with sqrt((double)d2) < R, i.e. the exact integer form of the reference's
// `distance < R` test on integer positions (-1 if none).  Evaluated with the same correctly rounded
// fp64 sqrt the reference's pdist uses, once per radius instead of once per agent pair.
// For R < 65536 only (dist2_bound decides the rest before any cast): there R <= 65536 - 2^-37, R * R < 2^32 and
// ceil(fl(R * R)) <= 2^32 converts exactly.  Beyond 2^63 (R >= 3.04e9, which the API accepts) the cast would be undefined.
__device__ __forceinline__ long long dist2_threshold(double R) {
    if (!(R > 0.0)) return -1;
    // start at ceil(fl(R*R)) >= the answer (the answer is < R^2 <= fl(R*R) (1 + 2^-53)) and walk down:
    // two square roots in the common case instead of four
    long long t = (long long)ceil(R * R);
    while (t >= 0 && !(sqrt((double)t) < R)) --t;
    return t;
}

// The threshold as the unsigned bound every `d2 <= T` test compares against, and the squared distance of two cells in
// the same unsigned word.  Coordinates lie in [0, 65535] (a map of 65 536 cells can be 1 x 65 536), so
// d2 <= 65535^2 + 0^2 = 4 294 836 225 < 2^32 - 1: neither the products nor the sum wrap, and the clamp to 0xffffffff
// never cuts a threshold below a distance that occurs.  r <= 0: the threshold is -1 and the bound 0 (no pair is at
// distance 0: agents stand on distinct cells).
// r >= 65536 (infinity included): the bound IS the clamp, decided on the double.  Every d2 an unsigned word holds is
// <= 2^32 - 1 and sqrt(2^32 - 1) = 65536 - 2^-17 - ... rounds to a double below 65536.0 (ulp 2^-37), so sqrt(d2) < r
// for all of them.  The walk-down gave the same word wherever its cast was defined (at r = 65536.0: 2^32 - 1 itself);
// below 65536 nothing changes, so every radius keeps the integer it had.
__device__ __forceinline__ unsigned dist2_bound(double r) {
    if (r >= 65536.0) return 0xffffffffu;
    const long long T = dist2_threshold(r);
    return T > 0xffffffffLL ? 0xffffffffu : T < 0 ? 0u : (unsigned)T;
}

__device__ __forceinline__ unsigned dist2(int ax, int ay, int bx, int by) {
    const unsigned dx = (unsigned)(ax - bx), dy = (unsigned)(ay - by);
    return dx * dx + dy * dy;
}

__device__ __forceinline__ double inv_sqrt_degree(int deg) { return deg ? sqrt(1.0 / (double)deg) : 0.0; }

// The rollout's radius: with grow, r /= 1.1 once and r *= 1.1 per trip until build(Tu) -- "build the graph at the
// bound Tu and tell me whether it is connected" -- says yes; without, one build at r.  Leaves the final radius in r and
// returns the last verdict.  A trip whose bound equals the last one built is not built again: same bound = same graph
// = still disconnected (otherwise the loop had ended), so nothing a caller keeps from its last build changes.
// Termination with grow: the bound reaches 65535^2 (the largest d2 of two cells, below the clamp of dist2_bound) after
// finitely many trips; from then on every pair is an edge and the graph is connected.
template <class Build>
__device__ __forceinline__ bool rollout_radius_search(double& r, bool grow, Build build) {
    if (grow) r = r / 1.1;
    unsigned Tu = 0u;
    bool built = false, connected = false;
    for (;;) {
        if (grow) r = r * 1.1;
        const unsigned Tn = dist2_bound(r);
        if (!built || Tn != Tu) {
            Tu = Tn;
            built = true;
            connected = build(Tu);
        }
        if (connected || !grow) break;
    }
    return connected;
}

// The expert schedules' radius: k = the number of multiplications by 1.1, starting from radius0, until build(Tu)
// says connected; at k = kGrowthCap it gives up and sets GNNPP_SCHEDULE_NO_RADIUS in status.  Skips equal bounds as above.
template <class Build>
__device__ __forceinline__ int expert_radius_search(double radius0, int& status, Build build) {
    double r = radius0;
    unsigned Tu = 0u;
    bool built = false;
    int k = 0;
    for (;;) {
        const unsigned Tn = dist2_bound(r);
        if (!built || Tn != Tu) {
            Tu = Tn;
            built = true;
            if (build(Tu)) break;
        }
        if (k == kGrowthCap) { status |= GNNPP_SCHEDULE_NO_RADIUS; break; }
        r = r * 1.1;
        ++k;
    }
    return k;
}

// ---- one-wave form: lane l of a wave holds agents l and l + 64 (teams of up to 128) ----------------------------------
__device__ __forceinline__ int lane_get(const int (&v)[2], int agent) {
    return __builtin_amdgcn_readlane(agent < 64 ? v[0] : v[1], agent & 63);
}

struct MaskPair { unsigned long long lo, hi; };

__device__ __forceinline__ MaskPair ballot2(bool p0, bool p1) {
    MaskPair m;
    m.lo = __ballot(p0);
    m.hi = __ballot(p1);
    return m;
}

struct WaveAgents {              // my two agents
    int px[2], py[2];
    bool live[2];
};

__device__ __forceinline__ WaveAgents wave_agents_load(const int* pos, int N, int lane) {
    WaveAgents A;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int n = lane + 64 * h;
        A.live[h] = n < N;
        A.px[h] = A.live[h] ? pos[2 * n] : -(1 << 20);        // dead lanes: far away from everything
        A.py[h] = A.live[h] ? pos[2 * n + 1] : -(1 << 20);
    }
    return A;
}

struct WaveRows { unsigned long long a0[2], a1[2]; };    // my two agents' adjacency rows: bits 0..63, bits 64..127

// Adjacency row i = ballot over the lanes of "d2(i, me) <= Tu", agent i's cell broadcast by readlane (the relation is
// symmetric: N ballots instead of N^2 / 64 lane-loops)
__device__ __forceinline__ MaskPair wave_adjacency_row(const WaveAgents& A, int i, int N, int lane, unsigned Tu) {
    const int bx = lane_get(A.px, i), by = lane_get(A.py, i);
    bool e[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        e[h] = A.live[h] && lane + 64 * h != i && dist2(A.px[h], A.py[h], bx, by) <= Tu;
    }
    return ballot2(e[0], N > 64 && e[1]);
}

// all N rows on one wave, each kept by the lane that holds its agent
__device__ __forceinline__ void wave_adjacency_rows(const WaveAgents& A, int N, int lane, unsigned Tu, WaveRows& rows) {
    for (int i = 0; i < N; ++i) {
        const MaskPair row = wave_adjacency_row(A, i, N, lane, Tu);
#pragma unroll
        for (int h = 0; h < 2; ++h) {                    // (constant indices: the rows stay in registers)
            if (lane + 64 * h == i) { rows.a0[h] = row.lo; rows.a1[h] = row.hi; }
        }
    }
}

// LEVEL-synchronous search from node 0: a node joins when its row meets the frontier -- one ballot pair per level
// (graph diameter) instead of one LDS round trip per node
__device__ __forceinline__ bool wave_connected(const WaveRows& rows, const bool (&live)[2], int N) {
    const bool two = N > 64;
    MaskPair R = {1ull, 0ull}, F = R;                              // reached set, frontier
    while (F.lo | F.hi) {
        const MaskPair nb = ballot2(live[0] && ((rows.a0[0] & F.lo) | (rows.a1[0] & F.hi)) != 0ull,
                                    two && live[1] && ((rows.a0[1] & F.lo) | (rows.a1[1] & F.hi)) != 0ull);
        F.lo = nb.lo & ~R.lo; F.hi = nb.hi & ~R.hi;
        R.lo |= nb.lo; R.hi |= nb.hi;
    }
    return __popcll(R.lo) + __popcll(R.hi) == N;
}

// inv [N] (LDS) <- fp64 D^-1/2 of my agents, 0 for isolated nodes
__device__ __forceinline__ void wave_store_inv(const WaveRows& rows, const bool (&live)[2], int lane, double* inv) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (live[h]) inv[lane + 64 * h] = inv_sqrt_degree(__popcll(rows.a0[h]) + __popcll(rows.a1[h]));
    }
}

// What a one-wave graph build leaves in LDS for gso_store: adj [N][2] (128-bit rows) | inv [N] | radius, flag
constexpr int kGsoSmemBytes = 2 * kMaxAgents * 8 + kMaxAgents * 8 + 32;

struct GsoLds {
    unsigned long long* adj;     // [N][2]
    double* inv;                 // [N]
    double* radius;              // [1]
    int* connected;              // [1]
};

__device__ __forceinline__ GsoLds gso_layout(char* smem) {
    GsoLds L;
    L.adj = reinterpret_cast<unsigned long long*>(smem);
    L.inv = reinterpret_cast<double*>(L.adj + 2 * kMaxAgents);
    L.radius = L.inv + kMaxAgents;
    L.connected = reinterpret_cast<int*>(L.radius + 1);
    return L;
}

// S [N][N] (and S64, when given) <- (inv_i * A_ij) * inv_j in fp64, rounded once for the fp32 copy; by all nt threads,
// nt / 16 rows in flight, 16 lanes per row.  After a barrier behind the build.
__device__ __forceinline__ void gso_store_S(const GsoLds& L, int N, float* S, double* S64, int tid, int nt) {
    for (int i = tid / 16; i < N; i += nt / 16) {
        const unsigned long long w0 = L.adj[2 * i], w1 = L.adj[2 * i + 1];
        const double ii = L.inv[i];
        for (int j = tid & 15; j < N; j += 16) {
            const bool on = j < 64 ? (w0 >> j) & 1ull : (w1 >> (j - 64)) & 1ull;
            S[i * N + j] = on ? (float)(ii * L.inv[j]) : 0.f;
            if (S64) S64[i * N + j] = on ? ii * L.inv[j] : 0.0;
        }
    }
}

}  // namespace gnnpp
