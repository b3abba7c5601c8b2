// Rollout simulator for teams of GNNPP_ROLLOUT_MAX_AGENTS < N <= GNNPP_ROLLOUT_MAX_TEAM agents per episode: the
// same observe / gso / move as rollout_kernels.hip (same reference lines, same bit-exact results), for teams too
// large for its one-wave kernels (lane l holds agents l and l + 64, 128-bit agent masks).  Teams of up to
// GNNPP_ROLLOUT_MAX_AGENTS agents never reach this file.
//
//   move     one workgroup per episode, thread t = agent t.  The per-agent work (planned cells, bumps, the
//            candidate sets of every collision pass, the swap loop, bookkeeping) is parallel; the reference's
//            order-dependent vertex-conflict loop is walked by wave 0 alone, from conflicting agent to conflicting
//            agent.  Every lookup it needs is O(1): agents stand on distinct cells and a cell can only be planned
//            by the agents on it and on its four neighbours, so an LDS map cell -> standing agent turns
//            "list_pos.count(pos)", "[j : allagents_pos[j] == pos]" and "list_nextpos.index(cur)" into five map
//            reads each.
//   gso      one workgroup per episode: radius (growth at step 0), level-synchronous connectivity search over
//            N-bit frontier bitsets, degrees and D^-1/2 in fp64, then S.
//   observe  rollout_observe_kernel's per-16-agent grid with the goals of all N agents staged in LDS.
// This file is included from gnnpp_api.hip after rollout_kernels.hip and uses its helpers.

namespace gnnpp {

constexpr int kMaxTeam = GNNPP_ROLLOUT_MAX_TEAM;
constexpr int kTeamWords = kMaxTeam / 64;               // 64-bit words of an N-bit agent set
constexpr int kTeamMaxCells = GNNPP_ROLLOUT_TEAM_MAX_CELLS;
constexpr int kTeamLdsBytes = 160 * 1024;
constexpr unsigned short kNoAgent = 0xffff;

__host__ __device__ inline int team_threads(int N) { return (N + 63) & ~63; }
__host__ __device__ inline size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

// (row, col) of a cell as one comparable word (rows and columns < 65536)
__device__ __forceinline__ unsigned team_key(int x, int y) { return ((unsigned)x << 16) | (unsigned)y; }

// The agent standing on the d-th cell around `key` (d = 0 the cell itself, 1..4 its neighbours), -1 if none.
// These five are exactly the agents that can plan the cell `key`.
__device__ __forceinline__ int team_stander(const unsigned short* idx, int H, int W, unsigned key, int d) {
    const int x = (int)(key >> 16) + (d == 1 ? -1 : d == 2 ? 1 : 0);
    const int y = (int)(key & 0xffffu) + (d == 3 ? -1 : d == 4 ? 1 : 0);
    if (x < 0 || x >= H || y < 0 || y >= W) return -1;
    const unsigned short a = idx[x * W + y];
    return a == kNoAgent ? -1 : (int)a;
}

// Workgroup-wide OR of a predicate: one ballot per wave, two barriers.  Every thread must call it.
__device__ __forceinline__ bool team_any(bool pred, unsigned long long* words, int tid, int nw) {
    const unsigned long long m = __ballot(pred);
    if ((tid & 63) == 0) words[tid >> 6] = m;
    __syncthreads();
    bool any = false;
    for (int w = 0; w < nw; ++w) any |= words[w] != 0ull;
    __syncthreads();
    return any;
}

// ---- move + collision shielding -------------------------------------------------------------------------------
struct TeamMoveLds {
    unsigned* ckey;                 // [N] current cell (fixed during the move)
    unsigned* lkey;                 // [N] list_pos of the reference == the live planned cell
    unsigned* skey;                 // [N] allagents_pos: the planned cells at the start of the pass
    int* last;                      // [N] lastAction
    unsigned short* idx;            // [H*W] agent standing on the cell, kNoAgent if none
    unsigned long long* todo;       // [kTeamWords] candidates of the vertex-conflict loop
    unsigned long long* words;      // [kTeamWords] ballots of team_any
    int* misc;                      // [4]
};

__host__ __device__ inline size_t team_move_smem(int N, int H, int W) {
    return round16((size_t)16 * N) + 2 * kTeamWords * 8 + 16 + round16((size_t)2 * H * W);
}

__device__ __forceinline__ TeamMoveLds team_move_layout(char* smem, int N) {
    TeamMoveLds L;
    L.ckey = reinterpret_cast<unsigned*>(smem);
    L.lkey = L.ckey + N;
    L.skey = L.lkey + N;
    L.last = reinterpret_cast<int*>(L.skey + N);
    L.todo = reinterpret_cast<unsigned long long*>(smem + round16((size_t)16 * N));
    L.words = L.todo + kTeamWords;
    L.misc = reinterpret_cast<int*>(L.words + kTeamWords);
    L.idx = reinterpret_cast<unsigned short*>(L.misc + 4);
    return L;
}

// number of agents whose list_pos is `key`
__device__ __forceinline__ int team_claims(const TeamMoveLds& L, int H, int W, unsigned key) {
    int n = 0;
#pragma unroll
    for (int d = 0; d < 5; ++d) {
        const int a = team_stander(L.idx, H, W, key, d);
        n += a >= 0 && L.lkey[a] == key;
    }
    return n;
}

// lowest set bit at or above `from` of the candidate set (wave 0, all lanes; -1 if none)
__device__ __forceinline__ int team_next_todo(const TeamMoveLds& L, int nw, int from, int lane) {
    unsigned long long w = 0ull;
    if (lane < nw) {
        const int lo = lane * 64;
        w = L.todo[lane];
        if (from >= lo + 64) w = 0ull;
        else if (from > lo) w &= ~0ull << (from - lo);
    }
    const unsigned long long nz = __ballot(w != 0ull);
    if (!nz) return -1;
    const int wi = __ffsll((long long)nz) - 1;
    const unsigned lo32 = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)w, wi);
    const unsigned hi32 = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(w >> 32), wi);
    const unsigned long long word = ((unsigned long long)hi32 << 32) | lo32;
    return wi * 64 + __ffsll((long long)word) - 1;
}

// The vertex-conflict loop of interRobotCollision (:476-522) on wave 0: the reference visits i = 0..N-1 and acts
// when list_pos[i] is claimed more than once.  The walk visits the candidates in ascending order and re-checks
// each with the live state, as the reference does when it reaches it.  Candidates: the agents whose cell was
// claimed twice at the start of the pass, plus -- whenever agents fall back to their current cells -- the
// claimants of those cells (list_pos only ever changes to the current cell of a stopped agent, so a new
// duplicate can only appear there).  Lanes 0..4 look at the five cells around a conflict cell.
__device__ bool team_vertex_walk(const RolloutArgs& p, int b, const TeamMoveLds& L, int nw, int lane, int& calls) {
    const int H = p.H, W = p.W;
    bool collision = false;
    for (int i = team_next_todo(L, nw, 0, lane); i >= 0; i = team_next_todo(L, nw, i + 1, lane)) {
        const unsigned pk = L.lkey[i];
        int a = -1;
        bool claim = false;
        if (lane < 5) {
            a = team_stander(L.idx, H, W, pk, lane);
            claim = a >= 0 && L.lkey[a] == pk;
        }
        if (__popcll(__ballot(claim)) <= 1) continue;
        collision = true;
        // collided = [j : allagents_pos[j] == pos] in ascending order; random.choice picks the k-th
        const bool in = lane < 5 && a >= 0 && L.skey[a] == pk;
        const unsigned long long im = __ballot(in);
        int rank = 0;
#pragma unroll
        for (int e = 0; e < 5; ++e) {
            const int ae = __builtin_amdgcn_readlane(a, e);
            rank += ((im >> e) & 1ull) && ae < a;
        }
        const int k = choose_mover(p, b, __popcll(im), calls);
        // one of them already stands still: all of them stop; otherwise all but the chosen one
        const bool all_stop = __ballot(in && L.last[a] == 4) != 0ull;
        const bool stop = in && (all_stop || rank != k);
        const bool back = stop && L.lkey[a] != L.ckey[a];
        if (stop) {
            L.last[a] = 4;
            L.lkey[a] = L.ckey[a];
        }
        __builtin_amdgcn_wave_barrier();                 // (the lanes' LDS writes precede the reads below)
        // the cells the stopped agents fell back to may now be claimed twice: their claimants become candidates
        for (unsigned long long bm = __ballot(back); bm; bm &= bm - 1) {
            const int s2 = __builtin_amdgcn_readlane(a, __ffsll((long long)bm) - 1);
            const unsigned c = L.ckey[s2];
            int a2 = -1;
            bool cl = false;
            if (lane < 5) {
                a2 = team_stander(L.idx, H, W, c, lane);
                cl = a2 >= 0 && L.lkey[a2] == c;
            }
            unsigned long long cm = __ballot(cl);
            if (__popcll(cm) > 1) {
                for (; cm; cm &= cm - 1) {
                    const int j = __builtin_amdgcn_readlane(a2, __ffsll((long long)cm) - 1);
                    if (lane == 0 && j > i) L.todo[j >> 6] |= 1ull << (j & 63);
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    return collision;
}

// One call of interRobotCollision (:462-555).  Every thread of the workgroup calls it; the result is uniform.
__device__ bool team_collision_pass(const RolloutArgs& p, int b, const TeamMoveLds& L, int t, int nw, int& calls) {
    const int N = p.N, H = p.H, W = p.W;
    const bool live = t < N;
    if (live) L.skey[t] = L.lkey[t];                     // allagents_pos: a snapshot, never updated
    __syncthreads();
    bool dup = false, stood = false;
    if (live) {
        const unsigned c = L.ckey[t];
        dup = team_claims(L, H, W, L.lkey[t]) > 1;      // my planned cell is claimed twice
#pragma unroll
        for (int d = 0; d < 5; ++d) {                    // somebody else plans the cell I stand on (swap candidate)
            const int a = team_stander(L.idx, H, W, c, d);
            stood |= a >= 0 && a != t && L.skey[a] == c;
        }
    }
    const unsigned long long dm = __ballot(dup);
    if ((t & 63) == 0) L.todo[t >> 6] = dm;
    if (!team_any(dup || stood, L.words, t, nw)) return false;   // (todo written before team_any's barrier)
    if (t < 64) {
        const bool c1 = team_vertex_walk(p, b, L, nw, t, calls);
        if (t == 0) L.misc[0] = c1;
    }
    __syncthreads();
    // position swaps (:524-553): s = list_nextpos.index(cur_i) is the lowest-index agent whose plan (at the start
    // of this loop) is my cell; if its cell is my plan, both stop.  Evaluated for all i at once on the snapshot:
    // an agent stopped earlier in the reference's loop can only re-select an already stopped pair (its plan is
    // then its own cell, which no other agent stands on), so the union of the stopped pairs is the same.
    bool swap = false;
    int s = -1;
    if (live) {
        const unsigned c = L.ckey[t];
#pragma unroll
        for (int d = 0; d < 5; ++d) {
            const int a = team_stander(L.idx, H, W, c, d);
            if (a >= 0 && L.lkey[a] == c && (s < 0 || a < s)) s = a;
        }
        swap = s >= 0 && s != t && L.ckey[s] == L.lkey[t];
    }
    const bool c1 = L.misc[0] != 0;
    __syncthreads();                                     // (every read of the snapshot precedes the stops)
    if (swap) {
        L.lkey[t] = L.ckey[t]; L.last[t] = 4;
        L.lkey[s] = L.ckey[s]; L.last[s] = 4;            // (several threads may stop s: the same values)
    }
    return team_any(swap, L.words, t, nw) || c1;
}

// multiRobotSim.move (:562-723) for one episode, one thread per agent; same statement as move_body.
__global__ __launch_bounds__(1024) void rollout_team_move_kernel(const RolloutArgs p) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int N = p.N, b = blockIdx.x, t = threadIdx.x, nt = blockDim.x, nw = nt >> 6;
    const TeamMoveLds L = team_move_layout(gnnpp_smem, N);
    int* pos = p.pos + (size_t)b * N * 2;
    const unsigned char* grid = p.grid + (p.grid_batched ? (size_t)b * p.H * p.W : 0);
    const int* goal = p.goal + (size_t)b * N * 2;
    int* reached = p.reached + (size_t)b * N;
    int* start_step = p.start_step + (size_t)b * N;
    int* end_step = p.end_step + (size_t)b * N;
    const int step = p.currentstep, maxstep = p.maxstep[b];
    const bool live = t < N;
    int key = 4, curx = 0, cury = 0, rch = 1, sst = -1, est = -1;
    if (live) {
        if (p.logits) {                                  // argmax of the logits, first max wins
            const float* l = p.logits + ((size_t)t * p.B + b) * 5;
            float best = l[0];
            key = 0;
#pragma unroll
            for (int k = 1; k < 5; ++k)
                if (l[k] > best) { best = l[k]; key = k; }
        } else {
            key = p.actions[(size_t)b * N + t];
        }
        curx = pos[2 * t]; cury = pos[2 * t + 1];
        rch = reached[t]; sst = start_step[t]; est = end_step[t];
    }
    const bool all_reached = !team_any(live && !rch, L.words, t, nw);
    bool predict_collision = false, move_collision = false;
    int calls = 0;                                       // (counted by wave 0, which makes every choice)
    const bool frozen = (p.done && p.done[b] != 0) || step > maxstep;   // the case's loop has ended
    if (!frozen && (!all_reached || step < maxstep)) {
        bool bumped = false;
        int nx = curx, ny = cury;
        if (live) {
            if (key != 4 && sst < 0) sst = step - 1;
            const int tx = curx + (key == 0 ? -1 : key == 2 ? 1 : 0);
            const int ty = cury + (key == 1 ? -1 : key == 3 ? 1 : 0);
            const bool edge = tx >= p.H || tx < 0 || ty >= p.W || ty < 0;
            bumped = edge || grid[tx * p.W + ty] == 1;
            if (!bumped) { nx = tx; ny = ty; }
        }
        {
            typedef unsigned v4u __attribute__((ext_vector_type(4)));
            const v4u none = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
            const int n16 = (int)(round16((size_t)2 * p.H * p.W) / 16);
            for (int i = t; i < n16; i += nt) reinterpret_cast<v4u*>(L.idx)[i] = none;
        }
        __syncthreads();
        if (live) {
            L.idx[curx * p.W + cury] = (unsigned short)t;   // agents stand on distinct cells
            L.ckey[t] = team_key(curx, cury);
            L.lkey[t] = team_key(nx, ny);
            L.last[t] = bumped ? 4 : key;
        }
        predict_collision = team_any(bumped, L.words, t, nw);   // (its barriers publish the writes above)
        bool detect = team_collision_pass(p, b, L, t, nw, calls);
        for (int it = 0; it < N; ++it) {
            if (!detect) break;
            detect = team_collision_pass(p, b, L, t, nw, calls);
            predict_collision = true;
        }
        move_collision = team_collision_pass(p, b, L, t, nw, calls);
        if (live) {
            const unsigned k2 = L.lkey[t];
            nx = (int)(k2 >> 16); ny = (int)(k2 & 0xffffu);
            pos[2 * t] = nx; pos[2 * t + 1] = ny;
            if (nx == goal[2 * t] && ny == goal[2 * t + 1] && !rch) {
                rch = 1;
                est = step;
            }
            if (step >= maxstep && !rch) {
                est = step;
                if (sst < 0) sst = 0;
            }
            reached[t] = rch; start_step[t] = sst; end_step[t] = est;
        }
    }
    if (!frozen && (all_reached || step >= maxstep)) {
        // makespan = max(end) - min(start), flowtime = sum(end - start); start None -> 0 (see move_body)
        int* e_l = reinterpret_cast<int*>(L.skey);      // (the collision scratch is free now)
        int* s_l = L.last;
        __syncthreads();
        if (live) { e_l[t] = est; s_l[t] = sst < 0 ? 0 : sst; }
        __syncthreads();
        if (t < 64) {
            int flow = 0, emax = -(1 << 30), smin = 1 << 30;
            for (int n = t; n < N; n += 64) {
                flow += e_l[n] - s_l[n];
                emax = max(emax, e_l[n]);
                smin = min(smin, s_l[n]);
            }
            __builtin_amdgcn_wave_barrier();
            e_l[t] = flow; s_l[t] = emax; L.ckey[t] = (unsigned)smin;
            __builtin_amdgcn_wave_barrier();
            if (t == 0) {
                for (int l = 1; l < 64; ++l) {
                    flow += e_l[l];
                    emax = max(emax, s_l[l]);
                    smin = min(smin, (int)L.ckey[l]);
                }
                p.stats[2 * b] = emax - smin;
                p.stats[2 * b + 1] = flow;
            }
        }
    }
    if (t == 0) {
        p.flags[3 * b] = all_reached;
        p.flags[3 * b + 1] = move_collision;
        p.flags[3 * b + 2] = predict_collision;
        if (p.choice_count) p.choice_count[b] = calls;
        if (p.done && !frozen && (all_reached || step >= maxstep)) p.done[b] = 1;   // the reference's loop breaks
    }
}

// ---- communication GSO ------------------------------------------------------------------------------------------
// The statement of comm_graph.hip (its dist2 / dist2_bound / inv_sqrt_degree) for one thread per agent: a node joins the
// level-synchronous search when one of the frontier's nodes is within reach (N-bit frontier sets in LDS, one barrier per
// level).  The adjacency is recomputed from the positions instead of being stored (N^2 bits).
__host__ __device__ inline size_t team_gso_smem(int N) {
    return round16((size_t)8 * N) + (size_t)8 * N + 3 * kTeamWords * 8 + 16;
}

__global__ __launch_bounds__(1024) void rollout_team_gso_kernel(const RolloutArgs p, int grow) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int N = p.N, b = blockIdx.x, t = threadIdx.x, nt = blockDim.x, nw = nt >> 6;
    int* px = reinterpret_cast<int*>(gnnpp_smem);                                   // [N]
    int* py = px + N;                                                               // [N]
    double* inv = reinterpret_cast<double*>(gnnpp_smem + round16((size_t)8 * N));   // [N]
    unsigned long long* fr[2] = {reinterpret_cast<unsigned long long*>(inv + N), nullptr};
    fr[1] = fr[0] + kTeamWords;
    unsigned long long* words = fr[1] + kTeamWords;                                 // [kTeamWords]
    const int* pos = p.pos + (size_t)b * N * 2;
    const bool live = t < N;
    int mx = 0, my = 0;
    if (live) { mx = pos[2 * t]; my = pos[2 * t + 1]; px[t] = mx; py[t] = my; }
    __syncthreads();
    double r = p.radius[b];
    if (grow) r = r / 1.1;
    unsigned Tu = 0u;
    bool connected = false;
    // Termination with grow: r grows by 1.1 per trip, so the bound reaches 65535^2 (the largest d2 of two cells, below
    // the clamp of dist2_bound) after finitely many trips; from then on every pair is an edge and the graph is connected.
    for (;;) {
        if (grow) r = r * 1.1;
        Tu = dist2_bound(r);                             // d2 < 2^32 - 1: a map of 65 536 cells can be 1 x 65 536
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
                for (int w = 0; w < nw && !join; ++w) {
                    for (unsigned long long f = fr[cur][w]; f; f &= f - 1) {
                        const int j = w * 64 + __ffsll((long long)f) - 1;
                        if (dist2(px[j], py[j], mx, my) <= Tu) { join = true; break; }
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
    if (live) {
        int deg = 0;
        for (int j = 0; j < N; ++j) deg += j != t && dist2(px[j], py[j], mx, my) <= Tu;
        inv[t] = inv_sqrt_degree(deg);
    }
    __syncthreads();
    // S: thread t owns columns t, t + nt, ...; rows go by (consecutive threads store consecutive floats)
    float* S = p.S + (size_t)b * N * N;
    for (int j = t; j < N; j += nt) {
        const int jx = px[j], jy = py[j];
        const double ij = inv[j];
        for (int i = 0; i < N; ++i)
            S[(size_t)i * N + j] = (i != j && dist2(px[i], py[i], jx, jy) <= Tu) ? (float)(inv[i] * ij) : 0.f;
    }
    if (t == 0) {
        p.radius[b] = r;
        if (p.connected) p.connected[b] = connected;
    }
}

// rollout_team_gso_kernel as a device body (as gso_body of rollout_kernels.hip is for small teams), for the streamed seat
// of rollout_team_stream_kernels.hip: the same statement, the same order of fp64 operations, the same stores.  Thread t of
// nt = team_threads(N), every thread of the workgroup calls it, `smem` = team_gso_smem(N) bytes of LDS.  Reads pos[b] and
// radius[b]; writes S[b], radius[b], connected[b].  The kernel above keeps its own text: called through this body it
// measured 3.7 % slower at 8 x 1024 agents, so only the new kernel calls it.  A change to one is a change
// to both; the streamed seat's tests (CPU and GPU) hold the body to the kernel bit for bit.
__device__ __forceinline__ void team_gso_body(const RolloutArgs& p, int b, int t, int nt, int grow, char* smem) {
    const int N = p.N, nw = nt >> 6;
    int* px = reinterpret_cast<int*>(smem);                                         // [N]
    int* py = px + N;                                                               // [N]
    double* inv = reinterpret_cast<double*>(smem + round16((size_t)8 * N));         // [N]
    unsigned long long* fr[2] = {reinterpret_cast<unsigned long long*>(inv + N), nullptr};
    fr[1] = fr[0] + kTeamWords;
    unsigned long long* words = fr[1] + kTeamWords;                                 // [kTeamWords]
    const int* pos = p.pos + (size_t)b * N * 2;
    const bool live = t < N;
    int mx = 0, my = 0;
    if (live) { mx = pos[2 * t]; my = pos[2 * t + 1]; px[t] = mx; py[t] = my; }
    __syncthreads();
    double r = p.radius[b];
    if (grow) r = r / 1.1;
    unsigned Tu = 0u;
    bool connected = false;
    // Termination with grow: r grows by 1.1 per trip, so the bound reaches 65535^2 (the largest d2 of two cells, below
    // the clamp of dist2_bound) after finitely many trips; from then on every pair is an edge and the graph is connected.
    for (;;) {
        if (grow) r = r * 1.1;
        Tu = dist2_bound(r);                             // d2 < 2^32 - 1: a map of 65 536 cells can be 1 x 65 536
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
                for (int w = 0; w < nw && !join; ++w) {
                    for (unsigned long long f = fr[cur][w]; f; f &= f - 1) {
                        const int j = w * 64 + __ffsll((long long)f) - 1;
                        if (dist2(px[j], py[j], mx, my) <= Tu) { join = true; break; }
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
    if (live) {
        int deg = 0;
        for (int j = 0; j < N; ++j) deg += j != t && dist2(px[j], py[j], mx, my) <= Tu;
        inv[t] = inv_sqrt_degree(deg);
    }
    __syncthreads();
    // S: thread t owns columns t, t + nt, ...; rows go by (consecutive threads store consecutive floats)
    float* S = p.S + (size_t)b * N * N;
    for (int j = t; j < N; j += nt) {
        const int jx = px[j], jy = py[j];
        const double ij = inv[j];
        for (int i = 0; i < N; ++i)
            S[(size_t)i * N + j] = (i != j && dist2(px[i], py[i], jx, jy) <= Tu) ? (float)(inv[i] * ij) : 0.f;
    }
    if (t == 0) {
        p.radius[b] = r;
        if (p.connected) p.connected[b] = connected;
    }
}

// ---- observation builder -----------------------------------------------------------------------------------------
// rollout_observe_kernel with room for the goals of N agents: grid (ceil(N / 16), B), 16 agents per workgroup.
__host__ __device__ inline size_t team_observe_smem(int N, int H, int W) {
    return round16((size_t)8 * N) + round16((size_t)H * W) + kObsStageBytes;
}

__global__ __launch_bounds__(256) void rollout_team_observe_kernel(const RolloutArgs p) {
    extern __shared__ __attribute__((aligned(16))) char gnnpp_smem[];
    const int b = blockIdx.y;
    const int n0 = blockIdx.x * kObsAgentsPerWg;
    int* goal_l = reinterpret_cast<int*>(gnnpp_smem);                        // [2N]
    unsigned char* cell = reinterpret_cast<unsigned char*>(gnnpp_smem + round16((size_t)8 * p.N));
    float* stage = reinterpret_cast<float*>(cell + round16((size_t)p.H * p.W));
    const int* pos = p.pos + (size_t)b * p.N * 2;
    observe_stage(p, b, cell, goal_l, threadIdx.x, 256);
    __syncthreads();
    observe_prep(p, pos, cell, goal_l, threadIdx.x, 256);
    __syncthreads();
    const int n1 = min(p.N, n0 + kObsAgentsPerWg);
    observe_rows(p, b, pos, n0, n1, cell, goal_l, threadIdx.x, 256, stage);
    __syncthreads();
    observe_flush(p, b, n0, n1, stage, threadIdx.x, 256);
}

// rollout_team_observe_kernel's four stages for agents [n0, n0 + 16) of episode b, for the streamed seat: 256 threads,
// `smem` = team_observe_smem(N, H, W) bytes of LDS
__device__ __forceinline__ void team_observe_body(const RolloutArgs& p, int b, int n0, int tid, char* smem) {
    int* goal_l = reinterpret_cast<int*>(smem);                              // [2N]
    unsigned char* cell = reinterpret_cast<unsigned char*>(smem + round16((size_t)8 * p.N));
    float* stage = reinterpret_cast<float*>(cell + round16((size_t)p.H * p.W));
    const int* pos = p.pos + (size_t)b * p.N * 2;
    observe_stage(p, b, cell, goal_l, tid, 256);
    __syncthreads();
    observe_prep(p, pos, cell, goal_l, tid, 256);
    __syncthreads();
    const int n1 = min(p.N, n0 + kObsAgentsPerWg);
    observe_rows(p, b, pos, n0, n1, cell, goal_l, tid, 256, stage);
    __syncthreads();
    observe_flush(p, b, n0, n1, stage, tid, 256);
}

// ---- launchers (N > GNNPP_ROLLOUT_MAX_AGENTS) ---------------------------------------------------------------------
// -2: the map does not fit the kernels' LDS (more than GNNPP_ROLLOUT_TEAM_MAX_CELLS cells); nothing is enqueued.
inline bool team_map_ok(const RolloutArgs& a) { return (long)a.H * a.W <= kTeamMaxCells; }

int rollout_team_observe_launch(const RolloutArgs& a, hipStream_t st) {
    if (!team_map_ok(a)) return -2;
    static LdsAttrOnce once;
    set_lds_attr_once(once, reinterpret_cast<const void*>(&rollout_team_observe_kernel), kTeamLdsBytes);
    hipLaunchKernelGGL(rollout_team_observe_kernel, dim3((a.N + kObsAgentsPerWg - 1) / kObsAgentsPerWg, a.B),
                       dim3(256), team_observe_smem(a.N, a.H, a.W), st, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int rollout_team_gso_launch(const RolloutArgs& a, int grow, hipStream_t st) {
    hipLaunchKernelGGL(rollout_team_gso_kernel, dim3(a.B), dim3(team_threads(a.N)), team_gso_smem(a.N), st, a, grow);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int rollout_team_move_launch(const RolloutArgs& a, hipStream_t st) {
    if (!team_map_ok(a)) return -2;
    static LdsAttrOnce once;
    set_lds_attr_once(once, reinterpret_cast<const void*>(&rollout_team_move_kernel), kTeamLdsBytes);
    hipLaunchKernelGGL(rollout_team_move_kernel, dim3(a.B), dim3(team_threads(a.N)), team_move_smem(a.N, a.H, a.W),
                       st, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// gnnpp_rollout_gso_observe: the graph, then the observations (two launches)
int rollout_team_gso_observe_launch(const RolloutArgs& a, hipStream_t st) {
    if (!team_map_ok(a)) return -2;
    const int rc = rollout_team_gso_launch(a, 0, st);
    return rc ? rc : rollout_team_observe_launch(a, st);
}

// gnnpp_rollout_step: move, then the graph and the observations of the new positions (three launches)
int rollout_team_step_launch(const RolloutArgs& a, hipStream_t st) {
    if (!team_map_ok(a)) return -2;
    int rc = rollout_team_move_launch(a, st);
    if (!rc) rc = rollout_team_gso_launch(a, 0, st);
    return rc ? rc : rollout_team_observe_launch(a, st);
}

static_assert(kTeamMaxCells == 64 * 1024 && 16 * kMaxTeam + 2 * kTeamWords * 8 + 16 + 2 * kTeamMaxCells <= kTeamLdsBytes,
              "team move kernel LDS");
static_assert(8 * kMaxTeam + kTeamMaxCells + (int)kObsStageBytes <= kTeamLdsBytes, "team observe kernel LDS");

}  // namespace gnnpp
