// extern "C" surface of libgnnpp.so -- see include/gnnpp.h for the contract of every entry point.
// Single translation unit: the kernels are included so hipcc builds one code object.
#include "../../include/gnnpp.h"
#include "../../include/gnnpp_train_b3.h"
#ifdef GNNPP_MEASURE
#include "gnnpp_measure.h"
#endif

#include "encoder_pack.hip"
#include "encoder_ring_f32.hip"
#include "encoder_kernel_f32.hip"
#include "comm_graph.hip"           // the communication graph, once per execution form: used by the rollout and expert files
#include "rollout_kernels.hip"       // before the fused policy kernel, which can run the simulator step too
#include "rollout_team_kernels.hip"  // teams of more than GNNPP_ROLLOUT_MAX_AGENTS agents
#include "expert_kernels.hip"        // training samples from expert schedules (uses the rollout's observation / graph code)
#include "expert_team_kernels.hip"   // ... for teams of up to GNNPP_ROLLOUT_MAX_TEAM agents (one thread per agent, row tiles of S)
#include "mapf_kernels.hip"          // prioritized-planning MAPF solver (the expert of the online loop)
#include "mapf_team_kernels.hip"     // ... for teams of up to 1024 agents on maps of up to 256 x 256 (one workgroup per case)
#include "mapf_distance_kernels.hip" // ... its planning orders: true goal distances and the orders ranked from them
#include "casegen_kernels.hip"       // ... its cases: connected random maps with start and goal pairs, from a seed
#include "casegen_maze_kernels.hip"  // ... their raw maps as the reference draws them: numpy's stream and the wall walk
#include "mapf_audit_kernels.hip"    // ... its checker: conflicts, arrivals and costs of any schedule
#include "encoder_kernel_h2.hip"
#include "encoder_kernel_b3.hip"
#include "lsigf_kernel.hip"
#include "policy_filter_kernel.hip"
#include "lsigf_small_kernel.hip"
#include "lsigf_team_kernel.hip"   // forward filter / head / policy step for graphs of up to 1024 nodes, spread over workgroups
#include "lsigf_team_train_kernel.hip"   // ... its training calls: lists of S^T, the forward that keeps the tap signals
#include "rollout_team_lists_kernel.hip"   // the rollout's communication graph as the team filter's neighbour lists
#include "expert_team_lists_kernel.hip"    // the expert schedules' graphs as capped neighbour lists, and the draw from them
#include "schedule_draw_kernels.hip"       // a training batch straight from stored schedules: only the picked steps are built
#include "train_encoder.hip"
#include "train_encoder_b3.hip"          // ... its convolutions on bf16x3 planes (opt-in training precision)
#include "train_ops.hip"
#include "rollout_trace_kernels.hip"       // the rollout's trace: a record launch behind each move, no simulator kernel touched
#include "rollout_stream_kernels.hip"      // streamed rollouts: finished episode slots refilled from a case queue
#include "rollout_stream_trace_kernels.hip"   // ... their trace: per-case tables, rows relative to the seat
#include "rollout_team_stream_kernels.hip"    // ... for teams of up to GNNPP_ROLLOUT_MAX_TEAM agents, dense graph or lists
#include "rollout_summary_kernels.hip"        // the reference's metrics of a rollout's per-case tables, one launch

using namespace gnnpp;

static_assert(GNNPP_OK == 0 && GNNPP_ERR_UNSUPPORTED == -2 && GNNPP_ERR_LAUNCH == -3, "codes");

extern "C" {

int gnnpp_version(void) { return 330; }

const char* gnnpp_error_string(int code) {
    switch (code) {
        case GNNPP_OK: return "ok";
        case GNNPP_ERR_ARG: return "invalid argument (null pointer, non-positive size or inconsistent flags)";
        case GNNPP_ERR_UNSUPPORTED: return "shape not supported by the gfx950 kernels (more than 112 nodes, or the graph's rows exceed the 160 KB LDS budget: N <= 100 is guaranteed at G, F <= 128)";
        case GNNPP_ERR_RANGE: return "an activation left the f16 range (|x| >= 65504) of GNNPP_PREC_SPLIT_F16; results of this call are not trustworthy -- run it with GNNPP_PREC_FP32 (the default), which has no input domain";
        case GNNPP_ERR_LAUNCH: return "HIP kernel launch failed";
        default: return "unknown gnnpp error code";
    }
}

size_t gnnpp_filter_packed_floats(int G, int F, int K, int E) {
    if (G <= 0 || F <= 0 || K <= 0 || E <= 0) return 0;
    return filter_packed_floats(G, F, K, E);
}

int gnnpp_filter_pack(const float* h, float* packed, int G, int F, int K, int E, void* stream) {
    if (!h || !packed || G <= 0 || F <= 0 || K <= 0 || E <= 0) return GNNPP_ERR_ARG;
    return filter_pack_launch(h, packed, G, F, K, E, static_cast<hipStream_t>(stream));
}

// One launch covers F <= 128 output features; wider filters run as several launches over
// output-feature chunks inside lsigf_launch (each chunk recomputes the cheap shifts).
// gnnpp_lsigf_fwd is this body without the tap signals (zs) and on S itself (s_transposed = 0).
static int lsigf_fwd_body(const float* x, const void* S, const float* packed, const float* bias, float* y, float* zs,
                          int B, int N, int Nin, int G, int F, int K, int E, int s_is_f64, int s_batched,
                          int s_transposed, int x_node_major, int y_node_major, int relu, int bias_per_node,
                          int precision, int* range_flag, void* stream) {
    if (!x || !packed || !y || B <= 0 || N <= 0 || Nin <= 0 || Nin > N || G <= 0 || F <= 0 ||
        K <= 0 || E <= 0 || precision < 0 || precision > 2)
        return GNNPP_ERR_ARG;
    if (K > 1 && !S) return GNNPP_ERR_ARG;
    if ((x_node_major || y_node_major) && Nin != N) return GNNPP_ERR_ARG;
    if (N > GNNPP_MAX_ROWS) return GNNPP_ERR_UNSUPPORTED;
    LsigfArgs a = {};
    a.x = x; a.S = S; a.wpk = packed; a.bias = bias; a.y = y; a.zs = zs;
    a.B = B; a.N = N; a.Nin = Nin; a.G = G; a.F = F; a.K = K; a.E = E;
    a.s_is_f64 = s_is_f64; a.s_batched = s_batched; a.s_transposed = s_transposed;
    a.x_node_major = x_node_major; a.y_node_major = y_node_major; a.relu = relu;
    a.bias_per_node = bias && bias_per_node; a.range_flag = range_flag; a.prec = precision;
    return lsigf_launch(a, static_cast<hipStream_t>(stream));
}

int gnnpp_lsigf_fwd(const float* x, const void* S, const float* packed, const float* bias,
                    float* y, int B, int N, int Nin, int G, int F, int K, int E, int s_is_f64,
                    int s_batched, int x_node_major, int y_node_major, int relu, int bias_per_node,
                    int precision, int* range_flag, void* stream) {
    return lsigf_fwd_body(x, S, packed, bias, y, nullptr, B, N, Nin, G, F, K, E, s_is_f64, s_batched, 0, x_node_major,
                          y_node_major, relu, bias_per_node, precision, range_flag, stream);
}

int gnnpp_lsigf_fwd_save(const float* x, const void* S, const float* packed, const float* bias,
                         float* y, float* zs, int B, int N, int Nin, int G, int F, int K, int E,
                         int s_is_f64, int s_batched, int s_transposed, int x_node_major,
                         int y_node_major, int relu, int bias_per_node, int precision, int* range_flag,
                         void* stream) {
    return lsigf_fwd_body(x, S, packed, bias, y, zs, B, N, Nin, G, F, K, E, s_is_f64, s_batched, s_transposed,
                          x_node_major, y_node_major, relu, bias_per_node, precision, range_flag, stream);
}

int gnnpp_lsigf_input_grad(const float* dy, const void* S, const float* packed_t, const float* mask, float* dx,
                           int B, int N, int G, int F, int K, int E, int s_is_f64, int s_batched, int node_major,
                           void* stream) {
    if (!dy || !packed_t || !dx || B <= 0 || N <= 0 || G <= 0 || F <= 0 || K <= 0 || E <= 0) return GNNPP_ERR_ARG;
    if (K > 1 && !S) return GNNPP_ERR_ARG;
    if (mask && !node_major) return GNNPP_ERR_ARG;     // (the mask is applied where the node-major rows are stored)
    if (N > GNNPP_MAX_ROWS) return GNNPP_ERR_UNSUPPORTED;
    LsigfArgs a = {};
    // the filter of h^T [G,E,K,F] on S^T: F input features (dy), G output features (dx); exact fp32 contraction
    a.x = dy; a.S = S; a.wpk = packed_t; a.bias = nullptr; a.y = dx; a.y_mask = mask;
    a.B = B; a.N = N; a.Nin = N; a.G = F; a.F = G; a.K = K; a.E = E;
    a.s_is_f64 = s_is_f64; a.s_batched = s_batched; a.s_transposed = 1;
    a.x_node_major = node_major; a.y_node_major = node_major; a.relu = 0;
    a.prec = GNNPP_PREC_FP32_MFMA;
    return lsigf_launch(a, static_cast<hipStream_t>(stream));
}

int gnnpp_lsigf_fits(int N, int G, int F, int K, int E) {
    if (N <= 0 || G <= 0 || F <= 0 || K <= 0 || E <= 0) return GNNPP_ERR_ARG;
    if (N > GNNPP_MAX_ROWS) return 0;
    if ((F + 127) / 128 > 64) return 0;                // lsigf_launch plans at most 64 chunks of 128 output features:
                                                       // F > 8192 takes the dense form too (the reference
                                                       // BatchLSIGF has no such limit)
    for (int f0 = 0; f0 < F; f0 += 128) {              // (lsigf_launch's chunks of <= 128 output features)
        LsigfArgs a = {};
        a.B = 1; a.N = N; a.Nin = N; a.G = G; a.K = K; a.E = E;
        a.F_all = F; a.f0 = f0; a.F = F - f0 < 128 ? F - f0 : 128;
        LsigfPlan plan;
        if (lsigf_plan(a, plan) != 0) return 0;
    }
    return 1;
}

size_t gnnpp_encoder_packed_floats(void) { return EncLayout::kTotal; }

int gnnpp_encoder_pack(const gnnpp_encoder_params* p, float* packed, void* stream) {
    if (!p || !packed || !p->fc_w || !p->fc_b) return GNNPP_ERR_ARG;
    EncRawParams rp;
    for (int i = 0; i < 5; ++i) {
        if (!p->conv_w[i] || !p->conv_b[i] || !p->bn_w[i] || !p->bn_b[i] || !p->bn_mean[i] ||
            !p->bn_var[i])
            return GNNPP_ERR_ARG;
        rp.conv_w[i] = p->conv_w[i]; rp.conv_b[i] = p->conv_b[i];
        rp.bn_w[i] = p->bn_w[i]; rp.bn_b[i] = p->bn_b[i];
        rp.bn_mean[i] = p->bn_mean[i]; rp.bn_var[i] = p->bn_var[i];
    }
    rp.fc_w = p->fc_w; rp.fc_b = p->fc_b; rp.bn_eps = p->bn_eps;
    return encoder_pack_launch(rp, packed, static_cast<hipStream_t>(stream));
}

int gnnpp_encoder_fwd(const float* obs, const float* packed, float* feat, int M, int precision,
                      int* range_flag, void* stream) {
    if (!obs || !packed || !feat || M <= 0 || precision < 0 || precision > 2) return GNNPP_ERR_ARG;
    return encoder_launch(obs, packed, feat, M, range_flag, precision, static_cast<hipStream_t>(stream));
}

std::atomic<int> g_fused_policy{1};   // GNNPP_TUNE_FUSED_POLICY

// Does the one-launch policy kernel apply?  (bf16x3 or split-f16 arithmetic -- the exact-fp32 MFMA schedule has no
// fused form --, N <= 16, K = 2..4, and a batch for which one workgroup per graph pays: measured -8 % at B = 512,
// -17 % at B <= 64 (N = 10), but +40 % at B = 2048 -- or N nearly fills the 16-lane tile.)
static bool fused_policy_applies(int B, int N, int K, int prec) {
#ifdef GNNPP_MEASURE
    if (g_filter_ablate.load(std::memory_order_relaxed) || g_encoder_stop.load(std::memory_order_relaxed))
        return false;
#endif
    const int knob = g_fused_policy.load(std::memory_order_relaxed);            // 2: whatever the batch size
    const bool fused_pays = B <= 2 * 256 || N >= 13 || knob == 2;
    return knob && fused_pays && prec != kPrecFp32Mfma &&
           N <= kTileAgents && K >= kPolicyTapsMin && K <= kPolicyTapsMax;
}

int gnnpp_policy_fwd(const float* obs, const void* S, const float* enc_packed,
                     const float* filt_packed, const float* gf_bias, const float* act_w,
                     const float* act_b, float* feat_ws, float* logits, int B, int N, int K, int E,
                     int s_is_f64, int precision, int* range_flag, void* stream) {
    if (!obs || !enc_packed || !filt_packed || !act_w || !act_b || !feat_ws || !logits || B <= 0 ||
        N <= 0 || K <= 0 || E <= 0 || precision < 0 || precision > 2)
        return GNNPP_ERR_ARG;
    if (K > 1 && !S) return GNNPP_ERR_ARG;
    if (N > GNNPP_MAX_ROWS) return GNNPP_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    LsigfArgs a = {};
    a.x = feat_ws; a.S = S; a.wpk = filt_packed; a.bias = gf_bias; a.y = nullptr;
    a.act_w = act_w; a.act_b = act_b; a.logits = logits;
    a.B = B; a.N = N; a.Nin = N; a.G = GNNPP_FEAT; a.F = GNNPP_FEAT; a.K = K; a.E = E;
    a.s_is_f64 = s_is_f64; a.s_batched = 1; a.x_node_major = 1; a.y_node_major = 1; a.relu = 1;
    a.range_flag = range_flag; a.prec = precision;
    LsigfPlan plan;
    int rc = lsigf_plan(a, plan);
    if (rc) return rc;
    // Fused path: a 16-lane tile per graph wastes (16 - N) / 16 of the encoder's lanes, which is free
    // while the graphs fit the chip in one round (2 workgroups per CU).
    if (E == 1 && fused_policy_applies(B, N, K, precision)) {
        // one launch: a workgroup encodes one graph's agents and runs its filter + action head
        PolicyTail pt;
        pt.S = S; pt.filt_h2 = precision == kPrecFp32 ? a.wpk_b : a.wpk_h;
        pt.gf_bias = gf_bias; pt.act_w = act_w; pt.act_b = act_b;
        pt.logits = logits; pt.B = B; pt.N = N; pt.s_is_f64 = s_is_f64;
        pt.range_flag = range_flag;
        pt.with_sim = 0;
        return precision == kPrecFp32 ? policy_launch_fused_b3(obs, enc_packed, pt, K, st)
                                      : policy_launch_fused(obs, enc_packed, pt, K, st);
    }
    rc = encoder_launch(obs, enc_packed, feat_ws, B * N, range_flag, precision, st);
    return rc ? rc : lsigf_dispatch(a, plan, st);
}

int gnnpp_filter_head_fwd(const float* x, const void* S, const float* packed, const float* bias,
                          const float* act_w, const float* act_b, float* logits, int B, int N, int G,
                          int F, int K, int E, int s_is_f64, int precision, int* range_flag, void* stream) {
    if (!x || !packed || !act_w || !act_b || !logits || B <= 0 || N <= 0 || G <= 0 || F <= 0 || K <= 0 ||
        E <= 0 || precision < 0 || precision > 2)
        return GNNPP_ERR_ARG;
    if (K > 1 && !S) return GNNPP_ERR_ARG;
    if (N > GNNPP_MAX_ROWS || F > 128) return GNNPP_ERR_UNSUPPORTED;   // the head needs all features at once
    LsigfArgs a = {};
    a.x = x; a.S = S; a.wpk = packed; a.bias = bias; a.y = nullptr;
    a.act_w = act_w; a.act_b = act_b; a.logits = logits;
    a.B = B; a.N = N; a.Nin = N; a.G = G; a.F = F; a.K = K; a.E = E;
    a.s_is_f64 = s_is_f64; a.s_batched = 1; a.x_node_major = 1; a.y_node_major = 1; a.relu = 1;
    a.range_flag = range_flag; a.prec = precision;
    return lsigf_launch(a, static_cast<hipStream_t>(stream));
}

size_t gnnpp_lsigf_team_workspace_bytes(int B, int N, int G, int K, int E, int s_batched) {
    if (B <= 0 || N <= 0 || N > GNNPP_ROLLOUT_MAX_TEAM || G <= 0 || G > 128 || K <= 0 || E <= 0) return 0;
    return team_layout(B, N, G, K, E, s_batched).total;
}

// Validation shared by the three team calls: GNNPP_OK when the launch sequence may be enqueued.
static int team_check(const void* x, const void* S, const void* packed, const void* workspace, size_t workspace_bytes,
                      int B, int N, int G, int F, int K, int E, int s_batched, int precision) {
    if (!x || !packed || !workspace || B <= 0 || N <= 0 || G <= 0 || F <= 0 || K <= 0 || E <= 0 || precision < 0 ||
        precision > 2 || N > GNNPP_ROLLOUT_MAX_TEAM)
        return GNNPP_ERR_ARG;
    if (K > 1 && !S) return GNNPP_ERR_ARG;
    if (G > 128 || F > 128 || precision == GNNPP_PREC_SPLIT_F16) return GNNPP_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < team_layout(B, N, G, K, E, s_batched).total)
        return GNNPP_ERR_ARG;
    return GNNPP_OK;
}

// The TeamArgs of a team call from its arguments.  S = nullptr: the caller's lists take its place (team_launch's last
// argument); the filter calls pass y, the head calls act_w / act_b / logits.
static TeamArgs team_args(const float* x, const void* S, int s_is_f64, const float* packed, const float* bias, float* y,
                          const float* act_w, const float* act_b, float* logits, int B, int N, int G, int F, int K,
                          int E, int s_batched, int relu, int bias_per_node) {
    TeamArgs a = {};
    a.x = x; a.S = S; a.wpk = packed; a.bias = bias; a.y = y; a.act_w = act_w; a.act_b = act_b; a.logits = logits;
    a.B = B; a.N = N; a.G = G; a.F = F; a.K = K; a.E = E;
    a.s_is_f64 = s_is_f64; a.s_batched = s_batched != 0; a.relu = relu; a.bias_per_node = bias && bias_per_node;
    return a;
}

int gnnpp_lsigf_team_fwd(const float* x, const void* S, const float* packed, const float* bias, float* y,
                         void* workspace, size_t workspace_bytes, int B, int N, int G, int F, int K, int E,
                         int s_is_f64, int s_batched, int relu, int bias_per_node, int precision, void* stream) {
    if (!y) return GNNPP_ERR_ARG;
    const int rc = team_check(x, S, packed, workspace, workspace_bytes, B, N, G, F, K, E, s_batched, precision);
    if (rc) return rc;
    return team_launch(team_args(x, S, s_is_f64, packed, bias, y, nullptr, nullptr, nullptr, B, N, G, F, K, E,
                                 s_batched, relu, bias_per_node),
                       workspace, precision, static_cast<hipStream_t>(stream));
}

int gnnpp_filter_head_team_fwd(const float* x, const void* S, const float* packed, const float* bias,
                               const float* act_w, const float* act_b, float* logits, void* workspace,
                               size_t workspace_bytes, int B, int N, int G, int F, int K, int E,
                               int s_is_f64, int precision, void* stream) {
    if (!act_w || !act_b || !logits) return GNNPP_ERR_ARG;
    const int rc = team_check(x, S, packed, workspace, workspace_bytes, B, N, G, F, K, E, 1, precision);
    if (rc) return rc;
    return team_launch(team_args(x, S, s_is_f64, packed, bias, nullptr, act_w, act_b, logits, B, N, G, F, K, E, 1, 1, 0),
                       workspace, precision, static_cast<hipStream_t>(stream));
}

size_t gnnpp_team_lists_bytes(int graphs, int N) {
    if (graphs <= 0 || N <= 0 || N > GNNPP_ROLLOUT_MAX_TEAM) return 0;
    return team_lists_bytes(graphs, N);
}

// a lists block handed in by the caller: present, 16-byte aligned and large enough for `graphs` graphs of N nodes
static bool team_lists_block_ok(const void* lists, size_t lists_bytes, int graphs, int N) {
    return lists && graphs > 0 && N > 0 && N <= GNNPP_ROLLOUT_MAX_TEAM && !(reinterpret_cast<uintptr_t>(lists) & 15) &&
           lists_bytes >= team_lists_bytes(graphs, N);
}

int gnnpp_team_lists_from_dense(const void* S, void* lists, size_t lists_bytes, int graphs, int N, int s_is_f64,
                                void* stream) {
    if (!S || !team_lists_block_ok(lists, lists_bytes, graphs, N)) return GNNPP_ERR_ARG;
    TeamArgs a = {};
    a.S = S; a.N = N; a.s_is_f64 = s_is_f64;
    return team_lists_launch(a, lists, graphs, static_cast<hipStream_t>(stream));
}

// The team calls on the caller's lists: team_check with the lists in the place of S (NULL allowed at K = 1), then
// the block's alignment.  Its size is the caller's contract (include/gnnpp.h).
static int team_lists_check(const void* x, const void* lists, const void* packed, const void* workspace,
                            size_t workspace_bytes, int B, int N, int G, int F, int K, int E, int s_batched,
                            int precision) {
    const int rc = team_check(x, lists, packed, workspace, workspace_bytes, B, N, G, F, K, E, s_batched, precision);
    if (rc) return rc;
    return (reinterpret_cast<uintptr_t>(lists) & 15) ? GNNPP_ERR_ARG : GNNPP_OK;
}

int gnnpp_lsigf_team_lists_fwd(const float* x, const void* lists, const float* packed, const float* bias, float* y,
                               void* workspace, size_t workspace_bytes, int B, int N, int G, int F, int K, int E,
                               int s_batched, int relu, int bias_per_node, int precision, void* stream) {
    if (!y) return GNNPP_ERR_ARG;
    const int rc = team_lists_check(x, lists, packed, workspace, workspace_bytes, B, N, G, F, K, E, s_batched, precision);
    if (rc) return rc;
    return team_launch(team_args(x, nullptr, 0, packed, bias, y, nullptr, nullptr, nullptr, B, N, G, F, K, E, s_batched,
                                 relu, bias_per_node),
                       workspace, precision, static_cast<hipStream_t>(stream), K > 1 ? lists : nullptr);
}

int gnnpp_filter_head_team_lists_fwd(const float* x, const void* lists, const float* packed, const float* bias,
                                     const float* act_w, const float* act_b, float* logits, void* workspace,
                                     size_t workspace_bytes, int B, int N, int G, int F, int K, int E, int precision,
                                     void* stream) {
    if (!act_w || !act_b || !logits) return GNNPP_ERR_ARG;
    const int rc = team_lists_check(x, lists, packed, workspace, workspace_bytes, B, N, G, F, K, E, 1, precision);
    if (rc) return rc;
    return team_launch(team_args(x, nullptr, 0, packed, bias, nullptr, act_w, act_b, logits, B, N, G, F, K, E, 1, 1, 0),
                       workspace, precision, static_cast<hipStream_t>(stream), K > 1 ? lists : nullptr);
}

// gnnpp_policy_team_fwd and _lists_fwd: the encoder into feat_ws, then the filter + head on it.  `graph` is the dense S,
// or with from_lists the caller's lists block.
static int policy_team(const float* obs, const void* graph, bool from_lists, int s_is_f64, const float* enc_packed,
                       const float* filt_packed, const float* gf_bias, const float* act_w, const float* act_b,
                       float* feat_ws, float* logits, int B, int N, int K, int E, int precision, int* range_flag,
                       void* stream, void* workspace, size_t workspace_bytes) {
    if (!obs || !enc_packed || !act_w || !act_b || !logits) return GNNPP_ERR_ARG;
    int rc = (from_lists ? team_lists_check : team_check)(feat_ws, graph, filt_packed, workspace, workspace_bytes, B, N,
                                                          GNNPP_FEAT, GNNPP_FEAT, K, E, 1, precision);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = encoder_launch(obs, enc_packed, feat_ws, B * N, range_flag, precision, st);
    if (rc) return rc;
    return team_launch(team_args(feat_ws, from_lists ? nullptr : graph, s_is_f64, filt_packed, gf_bias, nullptr, act_w,
                                 act_b, logits, B, N, GNNPP_FEAT, GNNPP_FEAT, K, E, 1, 1, 0),
                       workspace, precision, st, from_lists && K > 1 ? graph : nullptr);
}

int gnnpp_policy_team_fwd(const float* obs, const void* S, const float* enc_packed, const float* filt_packed,
                          const float* gf_bias, const float* act_w, const float* act_b, float* feat_ws,
                          float* logits, int B, int N, int K, int E, int s_is_f64, int precision,
                          int* range_flag, void* stream, void* workspace, size_t workspace_bytes) {
    return policy_team(obs, S, false, s_is_f64, enc_packed, filt_packed, gf_bias, act_w, act_b, feat_ws, logits, B, N, K,
                       E, precision, range_flag, stream, workspace, workspace_bytes);
}

int gnnpp_policy_team_lists_fwd(const float* obs, const void* lists, const float* enc_packed, const float* filt_packed,
                                const float* gf_bias, const float* act_w, const float* act_b, float* feat_ws,
                                float* logits, int B, int N, int K, int E, int precision, int* range_flag, void* stream,
                                void* workspace, size_t workspace_bytes) {
    return policy_team(obs, lists, true, 0, enc_packed, filt_packed, gf_bias, act_w, act_b, feat_ws, logits, B, N, K, E,
                       precision, range_flag, stream, workspace, workspace_bytes);
}

int gnnpp_team_lists_transpose(const void* lists, void* lists_t, size_t lists_bytes, int graphs, int N, void* stream) {
    if (lists == lists_t || !team_lists_block_ok(lists, lists_bytes, graphs, N) ||
        !team_lists_block_ok(lists_t, lists_bytes, graphs, N))
        return GNNPP_ERR_ARG;
    return team_transpose_launch(lists, lists_t, graphs, N, static_cast<hipStream_t>(stream));
}

int gnnpp_lsigf_team_lists_fwd_save(const float* x, const void* lists, const float* packed, const float* bias, float* y,
                                    float* zs, void* workspace, size_t workspace_bytes, int B, int N, int G, int F,
                                    int K, int E, int s_batched, int relu, int bias_per_node, int precision,
                                    void* stream) {
    if (!y || !zs) return GNNPP_ERR_ARG;
    const int rc = team_lists_check(x, lists, packed, workspace, workspace_bytes, B, N, G, F, K, E, s_batched, precision);
    if (rc) return rc;
    return team_save_launch(team_args(x, nullptr, 0, packed, bias, y, nullptr, nullptr, nullptr, B, N, G, F, K, E,
                                      s_batched, relu, bias_per_node),
                            K > 1 ? lists : nullptr, zs, precision, static_cast<hipStream_t>(stream));
}

// the team forward on (dy [B,N,F], lists of S^T, taps of h.permute(3,1,2,0)) -> dx [B,N,G], exact fp32 MFMA
int gnnpp_lsigf_team_lists_input_grad(const float* dy, const void* lists_t, const float* packed_t, float* dx,
                                      void* workspace, size_t workspace_bytes, int B, int N, int G, int F, int K,
                                      int E, int s_batched, void* stream) {
    return gnnpp_lsigf_team_lists_fwd(dy, lists_t, packed_t, nullptr, dx, workspace, workspace_bytes, B, N, F, G, K, E,
                                      s_batched, 0, 0, GNNPP_PREC_FP32_MFMA, stream);
}

int gnnpp_filter_head_mode(int B, int N, int K, int precision) {
    if (B <= 0 || N <= 0 || K <= 0 || precision < 0 || precision > 2) return -1;
    if (N > GNNPP_MAX_ROWS) return -1;
    alignas(16) static const float dummy[4] = {0.f, 0.f, 0.f, 0.f};   // (never dereferenced: the plan only tests pointers)
    LsigfArgs a = {};
    a.x = dummy; a.S = dummy; a.wpk = dummy; a.act_w = dummy; a.act_b = dummy;
    a.logits = const_cast<float*>(dummy);
    a.B = B; a.N = N; a.Nin = N; a.G = 128; a.F = 128; a.K = K; a.E = 1;
    a.s_batched = 1; a.x_node_major = 1; a.y_node_major = 1; a.relu = 1; a.prec = precision;
    a.F_all = 128;
    LsigfPlan plan;
    if (lsigf_plan(a, plan) != 0) return -1;
    PfLaunch L;
    return policy_filter_plan(a, L) ? L.mode : -1;
}

size_t gnnpp_encoder_train_workspace_floats(int N, int B) {
    if (N <= 0 || B <= 0) return 0;
    return train_ws_layout(N, B).total;
}

static int train_params_ok(const gnnpp_encoder_params* p, EncRawParams& rp) {
    if (!p) return 0;
    for (int i = 0; i < 5; ++i) {
        if (!p->conv_w[i] || !p->conv_b[i] || !p->bn_w[i] || !p->bn_b[i]) return 0;
        rp.conv_w[i] = p->conv_w[i]; rp.conv_b[i] = p->conv_b[i];
        rp.bn_w[i] = p->bn_w[i]; rp.bn_b[i] = p->bn_b[i];
        rp.bn_mean[i] = p->bn_mean[i]; rp.bn_var[i] = p->bn_var[i];
    }
    rp.fc_w = p->fc_w; rp.fc_b = p->fc_b; rp.bn_eps = p->bn_eps;
    return 1;
}

size_t gnnpp_train_pack_floats(void) { return train_pack_layout().total; }

int gnnpp_train_pack(const gnnpp_encoder_params* p, float* train_pack, const float* h, float* taps_fwd,
                     float* taps_t, int G, int F, int K, int E, void* stream) {
    if (!p && !h) return GNNPP_ERR_ARG;
    const float* cw[5] = {};
    if (p) {
        if (!train_pack || (reinterpret_cast<size_t>(train_pack) & 15)) return GNNPP_ERR_ARG;
        for (int i = 0; i < 5; ++i) {
            if (!p->conv_w[i]) return GNNPP_ERR_ARG;
            cw[i] = p->conv_w[i];
        }
    }
    TrainFilterPack fp = {};
    if (h) {
        if (!taps_fwd || !taps_t || G <= 0 || F <= 0 || K <= 0 || E <= 0) return GNNPP_ERR_ARG;
        fp.h = h; fp.fwd = taps_fwd; fp.tr = taps_t; fp.G = G; fp.F = F; fp.K = K; fp.E = E;
    }
    return train_pack_launch(p ? cw : nullptr, p ? train_pack : nullptr, fp, static_cast<hipStream_t>(stream));
}

// pack_b3 != NULL: the nine convolution launches run on bf16x3 planes (gnnpp_train_b3.h); NULL: exact fp32
static int encoder_train_fwd_call(const gnnpp_encoder_params* p, const float* obs, float* workspace, float* feat,
                                  int B, int N, float momentum, int update_running,
                                  long long* const* bn_num_batches, int feat_sample_major, const float* train_pack,
                                  void* stream, const void* pack_b3) {
    EncRawParams rp;
    if (train_pack && (reinterpret_cast<size_t>(train_pack) & 15)) return GNNPP_ERR_ARG;
    if (!train_params_ok(p, rp) || !obs || !workspace || !feat || B <= 0 || N <= 0) return GNNPP_ERR_ARG;
    float* rm[5];
    float* rv[5];
    for (int i = 0; i < 5; ++i) {
        if (update_running && (!p->bn_mean[i] || !p->bn_var[i])) return GNNPP_ERR_ARG;
        rm[i] = update_running ? const_cast<float*>(p->bn_mean[i]) : nullptr;
        rv[i] = update_running ? const_cast<float*>(p->bn_var[i]) : nullptr;
    }
    if (reinterpret_cast<size_t>(workspace) & 15) return GNNPP_ERR_ARG;      // (16-byte loads on its regions)
    return train_encoder_fwd(rp, rm, rv, update_running ? bn_num_batches : nullptr, momentum, obs, workspace, feat,
                             N, B, feat_sample_major, static_cast<hipStream_t>(stream), train_pack, pack_b3);
}

static int encoder_train_bwd_call(const gnnpp_encoder_params* p, const float* obs, float* workspace,
                                  const float* dfeat, const gnnpp_encoder_grads* g, int B, int N,
                                  int feat_sample_major, const float* train_pack, void* stream, const void* pack_b3) {
    EncRawParams rp;
    if (train_pack && (reinterpret_cast<size_t>(train_pack) & 15)) return GNNPP_ERR_ARG;
    if (!train_params_ok(p, rp) || !obs || !workspace || !dfeat || !g || B <= 0 || N <= 0) return GNNPP_ERR_ARG;
    for (int i = 0; i < 5; ++i)
        if (!g->conv_w[i] || !g->conv_b[i] || !g->bn_w[i] || !g->bn_b[i]) return GNNPP_ERR_ARG;
    return train_encoder_bwd(rp, obs, workspace, dfeat, g->conv_w, g->conv_b, g->bn_w, g->bn_b, N, B,
                             feat_sample_major, static_cast<hipStream_t>(stream), train_pack, pack_b3);
}

int gnnpp_encoder_train_fwd(const gnnpp_encoder_params* p, const float* obs, float* workspace, float* feat,
                            int B, int N, float momentum, int update_running,
                            long long* const* bn_num_batches, int feat_sample_major, const float* train_pack,
                            void* stream) {
    return encoder_train_fwd_call(p, obs, workspace, feat, B, N, momentum, update_running, bn_num_batches,
                                  feat_sample_major, train_pack, stream, nullptr);
}

int gnnpp_encoder_train_bwd(const gnnpp_encoder_params* p, const float* obs, float* workspace,
                            const float* dfeat, const gnnpp_encoder_grads* g, int B, int N,
                            int feat_sample_major, const float* train_pack, void* stream) {
    return encoder_train_bwd_call(p, obs, workspace, dfeat, g, B, N, feat_sample_major, train_pack, stream, nullptr);
}

// ---- include/gnnpp_train_b3.h: the opt-in training precision ------------------------------------------------------
size_t gnnpp_train_pack_b3_bytes(void) { return train_pack_b3_layout().total; }

int gnnpp_train_pack_b3(const gnnpp_encoder_params* p, void* pack_b3, void* stream) {
    if (!p || !pack_b3 || (reinterpret_cast<size_t>(pack_b3) & 15)) return GNNPP_ERR_ARG;
    const float* cw[5];
    for (int i = 0; i < 5; ++i) {
        if (!p->conv_w[i]) return GNNPP_ERR_ARG;
        cw[i] = p->conv_w[i];
    }
    return train_pack_b3_launch(cw, pack_b3, static_cast<hipStream_t>(stream));
}

// GNNPP_OK and the pack the launches read (NULL: exact fp32), or the refusal of (precision, pack_b3)
static int train_prec_ok(int precision, const void*& pack_b3) {
    if (precision == GNNPP_PREC_FP32_MFMA) { pack_b3 = nullptr; return GNNPP_OK; }
    if (precision != GNNPP_PREC_FP32) return GNNPP_ERR_UNSUPPORTED;
    if (!pack_b3 || (reinterpret_cast<size_t>(pack_b3) & 15)) return GNNPP_ERR_ARG;
    return GNNPP_OK;
}

int gnnpp_encoder_train_fwd_prec(const gnnpp_encoder_params* p, const float* obs, float* workspace, float* feat,
                                 int B, int N, float momentum, int update_running,
                                 long long* const* bn_num_batches, int feat_sample_major, const float* train_pack,
                                 void* stream, int precision, const void* pack_b3) {
    const int rc = train_prec_ok(precision, pack_b3);
    if (rc != GNNPP_OK) return rc;
    return encoder_train_fwd_call(p, obs, workspace, feat, B, N, momentum, update_running, bn_num_batches,
                                  feat_sample_major, train_pack, stream, pack_b3);
}

int gnnpp_encoder_train_bwd_prec(const gnnpp_encoder_params* p, const float* obs, float* workspace,
                                 const float* dfeat, const gnnpp_encoder_grads* g, int B, int N,
                                 int feat_sample_major, const float* train_pack, void* stream, int precision,
                                 const void* pack_b3) {
    const int rc = train_prec_ok(precision, pack_b3);
    if (rc != GNNPP_OK) return rc;
    return encoder_train_bwd_call(p, obs, workspace, dfeat, g, B, N, feat_sample_major, train_pack, stream, pack_b3);
}

size_t gnnpp_gemm_workspace_floats(int batch, int M, int N, int K) {
    if (batch <= 0 || M <= 0 || N <= 0 || K <= 0) return 0;
    return gemm_workspace_floats(batch, M, N, K);
}

int gnnpp_gemm_kmajor(const float* A, long long a_sb, long long a_sm, long long a_sk, const float* B,
                      long long b_sb, long long b_sk, float* C, long long c_sb, long long c_sm, int batch,
                      int M, int N, int K, float* workspace, void* stream) {
    if (!A || !B || !C || batch <= 0 || M <= 0 || N <= 0 || K <= 0) return GNNPP_ERR_ARG;
    const gnnpp_gemm_desc d = {A, a_sb, a_sm, a_sk, B, b_sb, b_sk, C, c_sb, c_sm, batch, M, N, K, nullptr};
    return gnnpp_gemm_kmajor_multi(&d, 1, workspace, stream);
}

size_t gnnpp_gemm_multi_workspace_floats(const gnnpp_gemm_desc* d, int count) {
    if (!d || count <= 0 || count > kGemmMax) return 0;
    size_t n = 0;
    for (int i = 0; i < count; ++i)
        if (d[i].batch > 0 && d[i].M > 0 && d[i].N > 0 && d[i].K > 0)
            n += gemm_workspace_floats(d[i].batch, d[i].M, d[i].N, d[i].K);
    return n;
}

int gnnpp_gemm_kmajor_multi(const gnnpp_gemm_desc* d, int count, float* workspace, void* stream) {
    if (!d || count <= 0 || count > kGemmMax) return GNNPP_ERR_ARG;
    GemmTable tb = {};
    for (int i = 0; i < count; ++i) {
        if (!d[i].A || !d[i].B || !d[i].C || d[i].batch <= 0 || d[i].M <= 0 || d[i].N <= 0 || d[i].K <= 0)
            return GNNPP_ERR_ARG;
        GemmOne& g = tb.g[i];
        g.A = d[i].A; g.a_sb = (long)d[i].a_sb; g.a_sm = (long)d[i].a_sm; g.a_sk = (long)d[i].a_sk;
        g.B = d[i].B; g.b_sb = (long)d[i].b_sb; g.b_sk = (long)d[i].b_sk;
        g.C = d[i].C; g.c_sb = (long)d[i].c_sb; g.c_sm = (long)d[i].c_sm;
        g.batch = d[i].batch; g.M = d[i].M; g.N = d[i].N; g.K = d[i].K; g.mask = d[i].mask;
    }
    tb.count = count;
    if (gnnpp_gemm_multi_workspace_floats(d, count) > 0 && !workspace) return GNNPP_ERR_ARG;
    return gemm_multi_launch(tb, workspace, static_cast<hipStream_t>(stream));
}

int gnnpp_linear_fwd(const float* x, const float* W, const float* bias, float* y, int R, int I, int O, int relu,
                     void* stream) {
    if (!x || !W || !y || R <= 0 || I <= 0 || O <= 0) return GNNPP_ERR_ARG;
    if (I % 64 != 0 || ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(W)) & 15)) return GNNPP_ERR_UNSUPPORTED;
    // (O % 4 == 0: every row of y is stored as 16-byte vectors)
    if ((O & 3) == 0 && (reinterpret_cast<size_t>(y) & 15)) return GNNPP_ERR_UNSUPPORTED;
    const int tiles = ((O + 15) / 16) * ((R + 15) / 16);
    hipLaunchKernelGGL(linear_fwd_kernel, dim3((tiles + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), x, W,
                       bias, y, R, I, O, relu);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

int gnnpp_policy_loss(const float* logits, const float* target, float* loss, float* dlogits, int B, int N,
                      int C, int logits_sample_major, void* stream) {
    if (!logits || !target || !loss || B <= 0 || N <= 0 || C <= 0 || C > 64) return GNNPP_ERR_ARG;
    hipLaunchKernelGGL(policy_loss_kernel, dim3(1), dim3(1024), 1024 * sizeof(double),
                       static_cast<hipStream_t>(stream), logits, target, loss, dlogits, B, N, C, logits_sample_major);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

int gnnpp_adam_step(const gnnpp_adam_tensors* t, float* state, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int tick, void* stream) {
    if (!t || !state || t->count <= 0 || t->count > kAdamTensors) return GNNPP_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    AdamTable tb = {};
    int blocks = 0;
    for (int i = 0; i < t->count; ++i) {
        if (!t->p[i] || !t->g[i] || !t->m[i] || !t->v[i] || t->numel[i] <= 0) return GNNPP_ERR_ARG;
        tb.p[i] = t->p[i]; tb.g[i] = t->g[i]; tb.m[i] = t->m[i]; tb.v[i] = t->v[i];
        tb.numel[i] = (long)t->numel[i];
        tb.first[i] = blocks;
        blocks += (int)((t->numel[i] + 1023) / 1024);
    }
    tb.first[t->count] = blocks;
    tb.count = t->count;
    hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 4 * sizeof(float), st, tb, state, lr, beta1, beta2, eps,
                       weight_decay, tick ? 1 : 0);
    return hipGetLastError() == hipSuccess ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}

#ifdef GNNPP_MEASURE
// libgnnpp_measure.so only: copy the kernels' phase time stamps ([1024 workgroups][16 wall + 16 cycle slots], 100 MHz
// ticks) to a HOST buffer of n entries (synchronises the device).
int gnnpp_measure_read_stamps(unsigned long long* host, int n) {
    if (!host || n <= 0 || n > 1024 * 32) return GNNPP_ERR_ARG;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), (size_t)n * sizeof(unsigned long long)) == hipSuccess
               ? GNNPP_OK : GNNPP_ERR_LAUNCH;
}
#endif

int gnnpp_get_tuning(int key) {
    switch (key) {
        case GNNPP_TUNE_FILTER_GPW: return g_filter_gpw.load();
        case GNNPP_TUNE_FILTER_WAVES: return g_filter_waves.load();
        case GNNPP_TUNE_FUSED_POLICY: return g_fused_policy.load();
        case GNNPP_TUNE_FILTER_SPLIT: return g_filter_split.load();
        case GNNPP_TUNE_POLICY_FILTER: return g_filter_policy_kernel.load();
        case GNNPP_TUNE_FILTER_SMALL: return g_filter_small_kernel.load();
        case GNNPP_TUNE_FILTER_SMALL_ROWS: return g_filter_small_rows.load();
        case GNNPP_TUNE_FILTER_PIPE_GRID: return g_filter_pipe_grid.load();
        case GNNPP_TUNE_POLICY_CP: return g_policy_column_packing.load();
        case GNNPP_TUNE_POLICY_CP_TEAM: return g_policy_cp_team.load();
        case GNNPP_TUNE_POLICY_CP_TEAM_L0: return g_policy_cp_team_l0.load();
        case GNNPP_TUNE_ENCODER_CP_TILE: return g_encoder_cp_tile.load();
        case GNNPP_TUNE_FILTER_PLANE_ALIAS: return g_filter_plane_alias.load();
        case GNNPP_TUNE_TRAIN_WGRAD_WGS: return g_train_wgrad_wgs.load();
        case GNNPP_TUNE_TRAIN_RUNNING_FUSED: return g_train_running_fused.load();
        case GNNPP_TUNE_ENCODER_ONE_PLANE: return g_encoder_one_plane.load();
#ifdef GNNPP_MEASURE
        case GNNPP_TUNE_FILTER_ABLATE: return g_filter_ablate.load();
        case GNNPP_TUNE_ENCODER_STOP: return g_encoder_stop.load();
#endif
        default: return GNNPP_ERR_ARG;
    }
}

int gnnpp_set_tuning(int key, int value) {
    switch (key) {
        case GNNPP_TUNE_FILTER_GPW:
            if (value < 0) return GNNPP_ERR_ARG;
            g_filter_gpw.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_FUSED_POLICY:
            if (value < 0 || value > 2) return GNNPP_ERR_ARG;
            g_fused_policy.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_FILTER_WAVES:
            if (value != 0 && value != 8 && value != 16) return GNNPP_ERR_ARG;
            g_filter_waves.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_FILTER_SPLIT:
            if (value < 0 || value > 7) return GNNPP_ERR_ARG;
            g_filter_split.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_POLICY_FILTER:
            if (value < 0 || value > 1) return GNNPP_ERR_ARG;
            g_filter_policy_kernel.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_FILTER_SMALL_ROWS:
            if (value != 0 && value != 32 && value != 48 && value != 64) return GNNPP_ERR_ARG;
            g_filter_small_rows.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_FILTER_PIPE_GRID:
            if (value < 0 || value > 4096) return GNNPP_ERR_ARG;
            g_filter_pipe_grid.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_POLICY_CP:
            if (value != 0 && value != 1) return GNNPP_ERR_ARG;
            g_policy_column_packing.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_POLICY_CP_TEAM:
            if (value != 0 && value != 1) return GNNPP_ERR_ARG;
            g_policy_cp_team.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_POLICY_CP_TEAM_L0:
            if (value != 0 && value != 1) return GNNPP_ERR_ARG;
            g_policy_cp_team_l0.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_ENCODER_CP_TILE:
            if (value != 0 && value != 16 && (value < 1 || value > 12)) return GNNPP_ERR_ARG;
            g_encoder_cp_tile.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_FILTER_PLANE_ALIAS:
            if (value < 0 || value > 1) return GNNPP_ERR_ARG;
            g_filter_plane_alias.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_TRAIN_RUNNING_FUSED:
            if (value < 0 || value > 1) return GNNPP_ERR_ARG;
            g_train_running_fused.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_ENCODER_ONE_PLANE:
            if (value < 0 || value > 1) return GNNPP_ERR_ARG;
            g_encoder_one_plane.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_TRAIN_WGRAD_WGS:
            if (value != 0 && (value < 16 || value > 2048)) return GNNPP_ERR_ARG;
            g_train_wgrad_wgs.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_FILTER_SMALL:
            if (value < 0 || value > 3) return GNNPP_ERR_ARG;
            g_filter_small_kernel.store(value);
            return GNNPP_OK;
#ifdef GNNPP_MEASURE
        case GNNPP_TUNE_ENCODER_STOP:
            if (value < 0 || value > 6) return GNNPP_ERR_ARG;
            g_encoder_stop.store(value);
            return GNNPP_OK;
        case GNNPP_TUNE_FILTER_ABLATE:
            g_filter_ablate.store(value);
            return GNNPP_OK;
#endif
        default:
            return GNNPP_ERR_ARG;
    }
}

int gnnpp_decode_actions(const float* logits, int* actions, int B, int N, void* stream) {
    if (!logits || !actions || B <= 0 || N <= 0) return GNNPP_ERR_ARG;
    return decode_actions_launch(logits, actions, B, N, static_cast<hipStream_t>(stream));
}

// pointers first, then the sizes: a struct with NULL pointers is GNNPP_ERR_ARG whatever its N
static int rollout_common_ok(const gnnpp_rollout* r, int max_agents = GNNPP_ROLLOUT_MAX_TEAM) {
    return r && r->pos && r->B > 0 && r->N > 0 && r->N <= max_agents;
}

static bool rollout_team(const gnnpp_rollout* r) { return r->N > GNNPP_ROLLOUT_MAX_AGENTS; }

int gnnpp_rollout_observe(const gnnpp_rollout* r, void* stream) {
    if (!rollout_common_ok(r) || !r->grid || !r->goal || !r->obs || r->H <= 0 || r->W <= 0)
        return GNNPP_ERR_ARG;
    if (rollout_team(r)) return rollout_team_observe_launch(*r, static_cast<hipStream_t>(stream));
    return rollout_observe_launch(*r, static_cast<hipStream_t>(stream));
}

int gnnpp_rollout_gso(const gnnpp_rollout* r, void* stream) {
    if (!rollout_common_ok(r) || !r->radius || !r->S) return GNNPP_ERR_ARG;
    if (rollout_team(r)) return rollout_team_gso_launch(*r, r->grow != 0, static_cast<hipStream_t>(stream));
    return rollout_gso_launch(*r, static_cast<hipStream_t>(stream));
}

int gnnpp_rollout_lists(const gnnpp_rollout* r, void* lists, size_t lists_bytes, void* stream) {
    if (!rollout_common_ok(r) || !r->radius || !team_lists_block_ok(lists, lists_bytes, r->B, r->N)) return GNNPP_ERR_ARG;
    return rollout_team_lists_launch(*r, r->grow != 0, lists, static_cast<hipStream_t>(stream));
}

int gnnpp_rollout_gso_observe(const gnnpp_rollout* r, void* stream) {
    if (!rollout_common_ok(r) || !r->radius || !r->S || !r->grid || !r->goal || !r->obs || r->H <= 0 || r->W <= 0)
        return GNNPP_ERR_ARG;
    if (rollout_team(r)) return rollout_team_gso_observe_launch(*r, static_cast<hipStream_t>(stream));
    return rollout_gso_observe_launch(*r, static_cast<hipStream_t>(stream));
}

// what gnnpp_rollout_move, _step and _policy_step share: the map, the actions' source, the episode's bookkeeping and a
// tie mode with the inputs it reads
static bool rollout_move_ok(const gnnpp_rollout* r, int max_agents = GNNPP_ROLLOUT_MAX_TEAM) {
    if (!rollout_common_ok(r, max_agents) || !r->grid || !r->goal || (!r->logits && !r->actions) ||
        !r->reached || !r->start_step || !r->end_step || !r->maxstep || !r->flags || !r->stats ||
        r->H <= 0 || r->W <= 0)
        return false;
    if (r->tie_mode == GNNPP_TIE_REPLAY && (!r->choices || r->max_choices <= 0)) return false;
    if (r->tie_mode < 0 || r->tie_mode > 3) return false;
    return !(r->tie_mode == GNNPP_TIE_MT19937 && (!r->rng_words || !r->rng_cursor || r->rng_max <= 0));
}

int gnnpp_rollout_move(const gnnpp_rollout* r, void* stream) {
    if (!rollout_move_ok(r)) return GNNPP_ERR_ARG;
    if (rollout_team(r)) return rollout_team_move_launch(*r, static_cast<hipStream_t>(stream));
    return rollout_move_launch(*r, static_cast<hipStream_t>(stream));
}

int gnnpp_rollout_step(const gnnpp_rollout* r, void* stream) {
    if (!rollout_move_ok(r) || !r->obs || !r->radius || !r->S) return GNNPP_ERR_ARG;
    if (rollout_team(r)) return rollout_team_step_launch(*r, static_cast<hipStream_t>(stream));
    return rollout_step_launch(*r, static_cast<hipStream_t>(stream));
}

int gnnpp_rollout_policy_step(const gnnpp_rollout* r, const float* enc_packed, const float* filt_packed,
                              const float* gf_bias, const float* act_w, const float* act_b, int K,
                              int precision, void* stream) {
    if (!rollout_move_ok(r, GNNPP_ROLLOUT_MAX_AGENTS) || !r->obs || !r->radius || !r->S || !r->logits ||
        !enc_packed || !filt_packed || !act_w || !act_b || precision < 0 || precision > 2)
        return GNNPP_ERR_ARG;
    // same conditions as the fused policy kernel of gnnpp_policy_fwd, plus room for the occupancy grid
    const size_t occ_room = precision == kPrecFp32 ? policy_sim_occ_bytes_b3() : policy_sim_occ_bytes(K);
    if (!(fused_policy_applies(r->B, r->N, K, precision) && (size_t)r->H * r->W <= occ_room))
        return GNNPP_ERR_UNSUPPORTED;
    PolicyTail pt;
    pt.S = r->S;
    pt.filt_h2 = filt_packed + (precision == kPrecFp32 ? filter_packed_b3_offset(GNNPP_FEAT, GNNPP_FEAT, K, 1)
                                                       : filter_packed_f32_floats(GNNPP_FEAT, GNNPP_FEAT, K, 1));
    pt.gf_bias = gf_bias; pt.act_w = act_w; pt.act_b = act_b; pt.logits = const_cast<float*>(r->logits);
    pt.B = r->B; pt.N = r->N; pt.s_is_f64 = 0;
    pt.range_flag = r->range_flag;
    pt.with_sim = 1;
    pt.sim = *r;
    pt.sim.grow = 0;
    pt.sim.actions = nullptr;
    return precision == kPrecFp32 ? policy_launch_fused_b3(r->obs, enc_packed, pt, K, static_cast<hipStream_t>(stream))
                                  : policy_launch_fused(r->obs, enc_packed, pt, K, static_cast<hipStream_t>(stream));
}

int gnnpp_rollout_policy_steps(const gnnpp_rollout* r, const float* enc_packed, const float* filt_packed,
                               const float* gf_bias, const float* act_w, const float* act_b, int K,
                               int nsteps, int precision, void* stream) {
    if (!r || nsteps <= 0 || r->tie_mode == GNNPP_TIE_REPLAY) return GNNPP_ERR_ARG;
    gnnpp_rollout rs = *r;
    for (int s = 0; s < nsteps; ++s) {
        rs.currentstep = r->currentstep + s;
        const int rc = gnnpp_rollout_policy_step(&rs, enc_packed, filt_packed, gf_bias, act_w, act_b, K, precision,
                                                 stream);
        if (rc != GNNPP_OK) return rc;                   // (argument / shape errors surface at s = 0)
    }
    return GNNPP_OK;
}

// pointers and sizes first (GNNPP_ERR_ARG; the team call's workspace among them), then the supported range: nothing is
// enqueued on an error
static bool schedules_ok(const gnnpp_schedules* s, int max_agents, bool need_obs = true, bool need_S = true) {
    return s && s->grid && s->goal && s->pos && s->case_start && (s->obs || !need_obs) && (s->S || !need_S) && s->target &&
           s->radius &&
           s->growth && s->status && s->step_info && s->C > 0 && s->T_total > 0 && s->C <= s->T_total && s->N > 0 &&
           s->N <= max_agents && s->H > 0 && s->W > 0 && s->radius0 > 0.0 && s->radius0 < 1e300;
}

int gnnpp_schedule_samples(const gnnpp_schedules* s, void* stream) {
    if (!schedules_ok(s, GNNPP_ROLLOUT_MAX_AGENTS)) return GNNPP_ERR_ARG;
    if (s->N < 2) return GNNPP_ERR_UNSUPPORTED;          // a graph of one node: deg = 0, the reference divides by it
    return schedule_samples_launch(*s, static_cast<hipStream_t>(stream));
}

size_t gnnpp_schedule_team_workspace_bytes(int N, int T_total) {
    if (N <= 0 || N > GNNPP_ROLLOUT_MAX_TEAM || T_total <= 0) return 0;
    return schedule_team_workspace_bytes(N, T_total);
}

int gnnpp_schedule_team_samples(const gnnpp_schedules* s, void* workspace, size_t workspace_bytes, void* stream) {
    if (!schedules_ok(s, GNNPP_ROLLOUT_MAX_TEAM) || !workspace || (reinterpret_cast<size_t>(workspace) & 7) != 0 ||
        workspace_bytes < schedule_team_workspace_bytes(s->N, s->T_total))
        return GNNPP_ERR_ARG;
    if (s->N < 2) return GNNPP_ERR_UNSUPPORTED;
    return schedule_team_samples_launch(*s, static_cast<double*>(workspace), static_cast<hipStream_t>(stream));
}

// the workspace of the team calls: present, 8-byte aligned, large enough
static bool schedule_team_workspace_ok(const gnnpp_schedules* s, const void* workspace, size_t workspace_bytes) {
    return workspace && (reinterpret_cast<size_t>(workspace) & 7) == 0 &&
           workspace_bytes >= schedule_team_workspace_bytes(s->N, s->T_total);
}

int gnnpp_schedule_team_plan(const gnnpp_schedules* s, void* workspace, size_t workspace_bytes, int* step_deg,
                             void* stream) {
    if (!schedules_ok(s, GNNPP_ROLLOUT_MAX_TEAM, false, false) || !schedule_team_workspace_ok(s, workspace, workspace_bytes) ||
        !step_deg)
        return GNNPP_ERR_ARG;
    if (s->N < 2) return GNNPP_ERR_UNSUPPORTED;
    return schedule_team_plan_launch(*s, static_cast<double*>(workspace), step_deg, static_cast<hipStream_t>(stream));
}

// a capped lists set: cap a multiple of 4 in 4 .. roundup4(N), the three arrays present and 16-byte aligned
static bool capped_lists_ok(const void* cnt, const void* idx, const void* val, int cap, int N) {
    const uintptr_t align = reinterpret_cast<uintptr_t>(cnt) | reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(val);
    return cnt && idx && val && !(align & 15) && cap >= 4 && !(cap & 3) && cap <= ((N + 3) & ~3);
}

int gnnpp_schedule_team_fill_lists(const gnnpp_schedules* s, const void* workspace, size_t workspace_bytes, int* cnt,
                                   unsigned short* idx, float* val, int cap, void* stream) {
    if (!schedules_ok(s, GNNPP_ROLLOUT_MAX_TEAM, true, false) || !schedule_team_workspace_ok(s, workspace, workspace_bytes) ||
        !capped_lists_ok(cnt, idx, val, cap, s->N))
        return GNNPP_ERR_ARG;
    if (s->N < 2) return GNNPP_ERR_UNSUPPORTED;
    return schedule_team_fill_lists_launch(*s, static_cast<const double*>(workspace), cnt, idx, val, cap,
                                           static_cast<hipStream_t>(stream));
}

int gnnpp_team_lists_gather(const int* cnt, const unsigned short* idx, const float* val, int graphs_src, int cap,
                            const int* index, int B, void* lists, size_t lists_bytes, int N, void* stream) {
    if (graphs_src <= 0 || !index || !team_lists_block_ok(lists, lists_bytes, B, N) || !capped_lists_ok(cnt, idx, val, cap, N))
        return GNNPP_ERR_ARG;
    return team_lists_gather_launch(cnt, idx, val, graphs_src, cap, index, B, lists, N, static_cast<hipStream_t>(stream));
}

size_t gnnpp_schedule_draw_workspace_bytes(int N, int B) {
    if (N <= 0 || N > GNNPP_ROLLOUT_MAX_TEAM || B <= 0) return 0;
    return schedule_draw_workspace_bytes(N, B);
}

// pointers, alignments and sizes first (GNNPP_ERR_ARG), then the supported range: nothing is enqueued on an error
int gnnpp_schedule_draw(const gnnpp_schedules* s, const int* index, int B, float* obs, float* target, float* S, void* lists,
                        size_t lists_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (!s || !s->grid || !s->goal || !s->pos || !s->case_start || !s->radius || !s->status || !index || !obs || !target ||
        !workspace || (S != nullptr) == (lists != nullptr))
        return GNNPP_ERR_ARG;
    if (s->C <= 0 || s->T_total <= 0 || s->C > s->T_total || s->N <= 0 || s->N > GNNPP_ROLLOUT_MAX_TEAM || s->H <= 0 ||
        s->W <= 0 || B <= 0)
        return GNNPP_ERR_ARG;
    const uintptr_t words = reinterpret_cast<uintptr_t>(index) | reinterpret_cast<uintptr_t>(obs) |
                            reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(S) |
                            reinterpret_cast<uintptr_t>(s->goal) | reinterpret_cast<uintptr_t>(s->pos) |
                            reinterpret_cast<uintptr_t>(s->case_start) | reinterpret_cast<uintptr_t>(s->status);
    const uintptr_t doubles = reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(s->radius);
    if ((words & 3) || (doubles & 7) || workspace_bytes < schedule_draw_workspace_bytes(s->N, B) ||
        (lists && !team_lists_block_ok(lists, lists_bytes, B, s->N)))
        return GNNPP_ERR_ARG;
    if (s->N < 2 || !schedule_draw_fits(s->N, s->H, s->W, B)) return GNNPP_ERR_UNSUPPORTED;
    gnnpp_schedules a = *s;                              // the batch's tensors in the place of the set's
    a.obs = obs; a.target = target; a.S = S; a.S64 = nullptr;
    return schedule_draw_launch(a, index, B, lists, static_cast<double*>(workspace), static_cast<hipStream_t>(stream));
}

size_t gnnpp_mapf_workspace_bytes(int C, int R, int H, int T_max) {
    if (C <= 0 || R <= 0 || H <= 0 || H > GNNPP_MAPF_MAX_SIDE || T_max < 0 || T_max > GNNPP_MAPF_MAX_STEPS ||
        (long long)C * R > 0x7fffffffLL)
        return 0;
    return mapf_workspace_bytes(C, R, H, T_max);
}

// pointers and sizes first (GNNPP_ERR_ARG), then the supported map size, then the workspace: nothing is enqueued on
// an error
static bool mapf_ok(const gnnpp_mapf* m, int max_agents, int max_steps) {
    return m && m->grid && m->start && m->goal && m->schedule && m->arrival && m->makespan && m->flowtime &&
           m->status && m->failing && m->restart && m->workspace && m->C > 0 && m->N > 0 && m->N <= max_agents &&
           m->H > 0 && m->W > 0 && m->R > 0 && (m->order || m->R == 1) && m->T_max >= 0 && m->T_max <= max_steps &&
           (long long)m->C * m->R <= 0x7fffffffLL;
}

int gnnpp_mapf_solve(const gnnpp_mapf* m, void* stream) {
    if (!mapf_ok(m, GNNPP_ROLLOUT_MAX_AGENTS, GNNPP_MAPF_MAX_STEPS)) return GNNPP_ERR_ARG;
    if (m->H > GNNPP_MAPF_MAX_SIDE || m->W > GNNPP_MAPF_MAX_SIDE) return GNNPP_ERR_UNSUPPORTED;
    if (m->workspace_bytes < mapf_workspace_bytes(m->C, m->R, m->H, m->T_max)) return GNNPP_ERR_ARG;
    return mapf_launch(*m, static_cast<hipStream_t>(stream));
}

size_t gnnpp_mapf_team_workspace_bytes(int C, int R, int H, int W, int T_max) {
    if (C <= 0 || R <= 0 || H <= 0 || H > GNNPP_MAPF_TEAM_MAX_SIDE || W <= 0 || W > GNNPP_MAPF_TEAM_MAX_SIDE || T_max < 0 ||
        T_max > GNNPP_MAPF_TEAM_MAX_STEPS || (long long)C * R > 0x7fffffffLL)
        return 0;
    return mapf_team_workspace_bytes(C, R, H, W, T_max);
}

// the workspace must hold the summary and at least one slot
int gnnpp_mapf_team_solve(const gnnpp_mapf* m, void* stream) {
    if (!mapf_ok(m, GNNPP_ROLLOUT_MAX_TEAM, GNNPP_MAPF_TEAM_MAX_STEPS)) return GNNPP_ERR_ARG;
    if (m->H > GNNPP_MAPF_TEAM_MAX_SIDE || m->W > GNNPP_MAPF_TEAM_MAX_SIDE) return GNNPP_ERR_UNSUPPORTED;
    const int slots = mapf_team_slots((long long)m->C * m->R, m->R, m->C, m->H, m->W, m->T_max, m->workspace_bytes);
    if (slots < 1) return GNNPP_ERR_ARG;
    return mapf_team_launch(*m, slots, static_cast<hipStream_t>(stream));
}

// include/gnnpp_mapf_distance.h: checked in gnnpp_mapf_team_solve's order, nothing is enqueued on an error
int gnnpp_mapf_distances(const unsigned char* grid, int grid_batched, const int* start, const int* goal, int C, int N,
                         int H, int W, int* dist, int* lower_makespan, int* lower_flowtime, void* stream) {
    if (!grid || !start || !goal || !dist || !lower_makespan || !lower_flowtime || C <= 0 || N <= 0 ||
        N > GNNPP_ROLLOUT_MAX_TEAM || H <= 0 || W <= 0 || (long long)C * N > 0x7fffffffLL)
        return GNNPP_ERR_ARG;
    if (H > GNNPP_MAPF_TEAM_MAX_SIDE || W > GNNPP_MAPF_TEAM_MAX_SIDE) return GNNPP_ERR_UNSUPPORTED;
    MapfDistArgs a;
    a.grid = grid;
    a.grid_batched = grid_batched;
    a.start = start;
    a.goal = goal;
    a.C = C;
    a.N = N;
    a.H = H;
    a.W = W;
    a.dist = dist;
    a.lower_makespan = lower_makespan;
    a.lower_flowtime = lower_flowtime;
    return mapf_distance_launch(a, static_cast<hipStream_t>(stream));
}

int gnnpp_mapf_orders(const int* dist, int C, int N, int R, const int* rules, unsigned seed, int* order, void* stream) {
    if (!rules || !order || C <= 0 || R <= 0 || N <= 0 || N > GNNPP_ROLLOUT_MAX_TEAM || (long long)C * R > 0x7fffffffLL)
        return GNNPP_ERR_ARG;
    for (int r = 0; r < R; ++r) {
        if (rules[r] < GNNPP_MAPF_ORDER_INDEX || rules[r] > GNNPP_MAPF_ORDER_HASHED) return GNNPP_ERR_ARG;
        if (!dist && (rules[r] == GNNPP_MAPF_ORDER_LONGEST_FIRST || rules[r] == GNNPP_MAPF_ORDER_SHORTEST_FIRST))
            return GNNPP_ERR_ARG;
    }
    return mapf_order_launch(dist, C, N, R, rules, seed, order, static_cast<hipStream_t>(stream));
}

// include/gnnpp_casegen.h: checked in gnnpp_mapf_distances' order, nothing is enqueued on an error
int gnnpp_casegen(const unsigned char* grid_in, int grid_in_batched, unsigned obstacle_threshold, unsigned seed, int C,
                  int N, int H, int W, unsigned char* grid, int* start, int* goal, int* cells, int* status, void* stream) {
    if (!grid || !start || !goal || !cells || !status || C <= 0 || N <= 0 || N > GNNPP_ROLLOUT_MAX_TEAM || H <= 0 ||
        W <= 0 || (long long)C * N > 0x7fffffffLL)
        return GNNPP_ERR_ARG;
    if (H > GNNPP_MAPF_TEAM_MAX_SIDE || W > GNNPP_MAPF_TEAM_MAX_SIDE) return GNNPP_ERR_UNSUPPORTED;
    CasegenArgs a;
    a.grid_in = grid_in;
    a.grid_in_batched = grid_in_batched;
    a.threshold = obstacle_threshold;
    a.seed = seed;
    a.C = C;
    a.N = N;
    a.H = H;
    a.W = W;
    a.grid = grid;
    a.start = start;
    a.goal = goal;
    a.cells = cells;
    a.status = status;
    return casegen_launch(a, static_cast<hipStream_t>(stream));
}

// include/gnnpp_casegen_maze.h: the pointer, the sizes, the supported map size; nothing is enqueued on an error
int gnnpp_casegen_maze(const unsigned* seeds, unsigned seed0, int C, int H, int W, int walls, int steps,
                       unsigned char* grid, int* words, void* stream) {
    if (!grid || C <= 0 || H < 3 || W < 3 || walls < 0 || steps < 0 || (long long)walls * steps > 0x7fffffffLL)
        return GNNPP_ERR_ARG;
    if (H > GNNPP_MAPF_TEAM_MAX_SIDE || W > GNNPP_MAPF_TEAM_MAX_SIDE) return GNNPP_ERR_UNSUPPORTED;
    CasegenMazeArgs a;
    a.seeds = seeds;
    a.seed0 = seed0;
    a.C = C;
    a.H = H;
    a.W = W;
    a.walls = walls;
    a.steps = steps;
    a.grid = grid;
    a.words = words;
    return casegen_maze_launch(a, static_cast<hipStream_t>(stream));
}

// include/gnnpp_mapf_audit.h: sizes (GNNPP_ERR_ARG), the supported map size, the horizon, pointers, the workspace; nothing
// is enqueued on an error
static int mapf_audit_sizes(int C, int N, int H, int W, int T_max) {
    if (C <= 0 || N <= 0 || N > GNNPP_ROLLOUT_MAX_TEAM || H <= 0 || W <= 0) return GNNPP_ERR_ARG;
    if (H > GNNPP_MAPF_TEAM_MAX_SIDE || W > GNNPP_MAPF_TEAM_MAX_SIDE) return GNNPP_ERR_UNSUPPORTED;
    if (T_max < 0 || T_max > GNNPP_MAPF_TEAM_MAX_STEPS || (long long)C * mapf_audit_chunks(T_max) > 0x7fffffffLL)
        return GNNPP_ERR_ARG;
    return GNNPP_OK;
}

size_t gnnpp_mapf_audit_workspace_bytes(int C, int N, int T_max) {
    if (mapf_audit_sizes(C, N, 1, 1, T_max) != GNNPP_OK) return 0;
    return mapf_audit_ws_bytes(C, N, T_max);
}

int gnnpp_mapf_audit(const unsigned char* grid, int grid_batched, const int* start, const int* goal, const int* schedule,
                     const int* steps, int C, int N, int H, int W, int T_max, int* status, int* arrival, int* makespan,
                     int* flowtime, int* counts, int* first, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = mapf_audit_sizes(C, N, H, W, T_max);
    if (rc != GNNPP_OK) return rc;
    if (!grid || !goal || !schedule || !status || !arrival || !makespan || !flowtime || !counts || !first || !workspace)
        return GNNPP_ERR_ARG;
    if (workspace_bytes < mapf_audit_ws_bytes(C, N, T_max)) return GNNPP_ERR_ARG;
    MapfAuditArgs a;
    a.grid = grid;
    a.grid_batched = grid_batched;
    a.start = start;
    a.goal = goal;
    a.schedule = schedule;
    a.steps = steps;
    a.C = C;
    a.N = N;
    a.H = H;
    a.W = W;
    a.T_max = T_max;
    a.status = status;
    a.arrival = arrival;
    a.makespan = makespan;
    a.flowtime = flowtime;
    a.counts = counts;
    a.first = first;
    a.ws = static_cast<int*>(workspace);
    return mapf_audit_launch(a, static_cast<hipStream_t>(stream));
}

// include/gnnpp_rollout_trace.h: the struct's sizes and pointers, the trace's, then the `count` steps from `first` that are to
// be recorded; nothing is enqueued on an error
static bool rollout_trace_ok(const gnnpp_rollout* r, const gnnpp_rollout_trace* tr) {
    return r && tr && r->pos && r->B > 0 && r->N > 0 && r->N <= GNNPP_ROLLOUT_MAX_TEAM &&
           (long long)r->B * r->N <= 0x7fffffffLL && tr->path && tr->steps && tr->seen_done && tr->T_cap >= 1;
}

static bool rollout_trace_steps_ok(const gnnpp_rollout* r, const gnnpp_rollout_trace* tr, int first, int count) {
    if (first < 1 || first > tr->T_cap || count < 1 || count > tr->T_cap - first + 1) return false;
    return r->logits || r->actions || !(tr->action || tr->shielded);
}

int gnnpp_rollout_trace_begin(const gnnpp_rollout* r, const gnnpp_rollout_trace* tr, void* stream) {
    if (!rollout_trace_ok(r, tr)) return GNNPP_ERR_ARG;
    return rollout_trace_begin_launch(*r, *tr, static_cast<hipStream_t>(stream));
}

int gnnpp_rollout_trace_record(const gnnpp_rollout* r, const gnnpp_rollout_trace* tr, void* stream) {
    if (!rollout_trace_ok(r, tr) || !rollout_trace_steps_ok(r, tr, r->currentstep, 1)) return GNNPP_ERR_ARG;
    return rollout_trace_record_launch(*r, *tr, static_cast<hipStream_t>(stream));
}

int gnnpp_rollout_policy_steps_traced(const gnnpp_rollout* r, const float* enc_packed, const float* filt_packed,
                                      const float* gf_bias, const float* act_w, const float* act_b, int K, int nsteps,
                                      int precision, const gnnpp_rollout_trace* tr, void* stream) {
    if (!r || nsteps <= 0 || r->tie_mode == GNNPP_TIE_REPLAY) return GNNPP_ERR_ARG;
    if (!rollout_trace_ok(r, tr) || !rollout_trace_steps_ok(r, tr, r->currentstep, nsteps)) return GNNPP_ERR_ARG;
    gnnpp_rollout rs = *r;
    for (int s = 0; s < nsteps; ++s) {
        rs.currentstep = r->currentstep + s;
        int rc = gnnpp_rollout_policy_step(&rs, enc_packed, filt_packed, gf_bias, act_w, act_b, K, precision, stream);
        if (rc != GNNPP_OK) return rc;                   // (argument / shape errors surface at s = 0)
        rc = rollout_trace_record_launch(rs, *tr, static_cast<hipStream_t>(stream));
        if (rc != GNNPP_OK) return rc;
    }
    return GNNPP_OK;
}

// include/gnnpp_rollout_stream.h: pointers and sizes first (GNNPP_ERR_ARG), then what the streamed path does not cover
// (GNNPP_ERR_UNSUPPORTED); nothing is enqueued and no HIP call is made on an error
// the GNNPP_ERR_ARG half, shared with gnnpp_rollout_team_stream.h (whose lists form needs no r->S)
static int rollout_stream_args_check(const gnnpp_rollout* r, const gnnpp_rollout_stream* s, bool reseat, int now,
                                     bool need_S = true) {
    if (!r || !s || !r->pos || !r->done || r->B <= 0 || r->N < 1 || r->H <= 0 || r->W <= 0 || s->C <= 0)
        return GNNPP_ERR_ARG;
    if (!s->case_grid || !s->case_start || !s->case_goal || !s->case_maxstep || !s->cursor || !s->slot_case ||
        !s->slot_t0 || !s->assign || !s->goal || !s->maxstep || !s->reached || !s->start_step || !s->end_step || !s->pos ||
        !s->radius || !s->stats || !s->lived || !s->slot || !s->t0)
        return GNNPP_ERR_ARG;
    if (reseat && (!r->grid || !r->goal || !r->obs || !r->radius || (need_S && !r->S) || !r->reached || !r->start_step ||
                   !r->end_step || !r->maxstep || !r->flags || !r->stats))
        return GNNPP_ERR_ARG;
    if ((r->grid_batched != 0) != (s->case_grid_batched != 0)) return GNNPP_ERR_ARG;
    if (reseat) {
        if (s->case_grid_batched ? (!s->slot_grid || s->slot_grid != r->grid) : s->case_grid != r->grid) return GNNPP_ERR_ARG;
        if (s->goal != r->goal || s->maxstep != r->maxstep) return GNNPP_ERR_ARG;
        if (!(s->commR > 0.0) || !(s->commR < 1.0e300) || now < 0 || now > (1 << 30)) return GNNPP_ERR_ARG;
    }
    if (r->tie_mode < 0 || r->tie_mode > 3) return GNNPP_ERR_ARG;
    return GNNPP_OK;
}

static int rollout_stream_check(const gnnpp_rollout* r, const gnnpp_rollout_stream* s, bool reseat, int now) {
    const int rc = rollout_stream_args_check(r, s, reseat, now);
    if (rc != GNNPP_OK) return rc;
    if (r->N > GNNPP_ROLLOUT_MAX_AGENTS || (size_t)r->H * (size_t)r->W > kOneWaveMaxCells) return GNNPP_ERR_UNSUPPORTED;
    if (r->tie_mode == GNNPP_TIE_REPLAY || r->tie_mode == GNNPP_TIE_MT19937) return GNNPP_ERR_UNSUPPORTED;
    return GNNPP_OK;
}

int gnnpp_rollout_stream_begin(const gnnpp_rollout* r, const gnnpp_rollout_stream* s, void* stream) {
    const int rc = rollout_stream_check(r, s, false, 0);
    if (rc != GNNPP_OK) return rc;
    return rollout_stream_begin_launch(*r, *s, static_cast<hipStream_t>(stream));
}

int gnnpp_rollout_stream_reseat(const gnnpp_rollout* r, const gnnpp_rollout_stream* s, int now, void* stream) {
    const int rc = rollout_stream_check(r, s, true, now);
    if (rc != GNNPP_OK) return rc;
    return rollout_stream_reseat_launch(*r, *s, now, static_cast<hipStream_t>(stream));
}

// include/gnnpp_rollout_team_stream.h: the same order -- pointers and sizes, the lists block among them, then the scope
static int rollout_team_stream_check(const gnnpp_rollout* r, const gnnpp_rollout_stream* s, bool reseat, int now,
                                     const void* lists, size_t lists_bytes) {
    const int rc = rollout_stream_args_check(r, s, reseat, now, lists == nullptr);
    if (rc != GNNPP_OK) return rc;
    if (lists && r->N <= GNNPP_ROLLOUT_MAX_TEAM && !team_lists_block_ok(lists, lists_bytes, r->B, r->N)) return GNNPP_ERR_ARG;
    if (r->N <= GNNPP_ROLLOUT_MAX_AGENTS || r->N > GNNPP_ROLLOUT_MAX_TEAM ||
        (size_t)r->H * (size_t)r->W > (size_t)GNNPP_ROLLOUT_TEAM_MAX_CELLS)
        return GNNPP_ERR_UNSUPPORTED;
    if (r->tie_mode == GNNPP_TIE_REPLAY || r->tie_mode == GNNPP_TIE_MT19937) return GNNPP_ERR_UNSUPPORTED;
    return GNNPP_OK;
}

int gnnpp_rollout_team_stream_begin(const gnnpp_rollout* r, const gnnpp_rollout_stream* s, void* stream) {
    const int rc = rollout_team_stream_check(r, s, false, 0, nullptr, 0);
    if (rc != GNNPP_OK) return rc;
    return rollout_stream_begin_launch(*r, *s, static_cast<hipStream_t>(stream));
}

int gnnpp_rollout_team_stream_reseat(const gnnpp_rollout* r, const gnnpp_rollout_stream* s, int now, void* lists,
                                     size_t lists_bytes, void* stream) {
    const int rc = rollout_team_stream_check(r, s, true, now, lists, lists_bytes);
    if (rc != GNNPP_OK) return rc;
    return rollout_team_stream_reseat_launch(*r, *s, now, lists, static_cast<hipStream_t>(stream));
}

// include/gnnpp_rollout_stream_trace.h: pointers and sizes first (GNNPP_ERR_ARG), then what a stream does not cover
// (GNNPP_ERR_UNSUPPORTED, where gnnpp_rollout_stream_reseat answers it); `count` steps from r->currentstep are to be recorded
// (count = 0: begin).  Nothing is enqueued and no HIP call is made on an error
static int rollout_stream_trace_check(const gnnpp_rollout* r, const gnnpp_rollout_stream* s,
                                      const gnnpp_rollout_stream_trace* tr, bool record, int count) {
    if (!r || !s || !tr) return GNNPP_ERR_ARG;
    if (!r->pos || !r->done || !r->maxstep || !s->slot_case || !s->slot_t0 || !s->case_start || !tr->path || !tr->steps ||
        !tr->seen_done)
        return GNNPP_ERR_ARG;
    if (r->B <= 0 || r->N < 1 || s->C <= 0 || (long long)r->B * r->N > 0x7fffffffLL ||
        (long long)s->C * r->N > 0x7fffffffLL || tr->T_cap < 1)
        return GNNPP_ERR_ARG;
    if (record) {
        if (r->currentstep < 1 || count < 1) return GNNPP_ERR_ARG;
        if (!r->logits && !r->actions && (tr->action || tr->shielded)) return GNNPP_ERR_ARG;
    }
    if (r->N > GNNPP_ROLLOUT_MAX_AGENTS) return GNNPP_ERR_UNSUPPORTED;
    if (r->tie_mode == GNNPP_TIE_REPLAY || r->tie_mode == GNNPP_TIE_MT19937) return GNNPP_ERR_UNSUPPORTED;
    return GNNPP_OK;
}

int gnnpp_rollout_stream_trace_begin(const gnnpp_rollout* r, const gnnpp_rollout_stream* s,
                                     const gnnpp_rollout_stream_trace* tr, void* stream) {
    const int rc = rollout_stream_trace_check(r, s, tr, false, 0);
    if (rc != GNNPP_OK) return rc;
    return rollout_stream_trace_begin_launch(*r, *s, *tr, static_cast<hipStream_t>(stream));
}

int gnnpp_rollout_stream_trace_record(const gnnpp_rollout* r, const gnnpp_rollout_stream* s,
                                      const gnnpp_rollout_stream_trace* tr, void* stream) {
    const int rc = rollout_stream_trace_check(r, s, tr, true, 1);
    if (rc != GNNPP_OK) return rc;
    return rollout_stream_trace_record_launch(*r, *s, *tr, static_cast<hipStream_t>(stream));
}

int gnnpp_rollout_stream_policy_steps_traced(const gnnpp_rollout* r, const float* enc_packed, const float* filt_packed,
                                             const float* gf_bias, const float* act_w, const float* act_b, int K,
                                             int nsteps, int precision, const gnnpp_rollout_stream* s,
                                             const gnnpp_rollout_stream_trace* tr, void* stream) {
    int rc = rollout_stream_trace_check(r, s, tr, true, nsteps);
    if (rc != GNNPP_OK) return rc;
    gnnpp_rollout rs = *r;
    for (int i = 0; i < nsteps; ++i) {
        rs.currentstep = r->currentstep + i;
        rc = gnnpp_rollout_policy_step(&rs, enc_packed, filt_packed, gf_bias, act_w, act_b, K, precision, stream);
        if (rc != GNNPP_OK) return rc;                   // (argument / shape errors surface at i = 0)
        rc = rollout_stream_trace_record_launch(rs, *s, *tr, static_cast<hipStream_t>(stream));
        if (rc != GNNPP_OK) return rc;
    }
    return GNNPP_OK;
}

// include/gnnpp_rollout_summary.h: every check before any HIP call, nothing enqueued on an error
size_t gnnpp_rollout_summary_out_bytes(int N, int G) {
    if (N < 1 || G < 1 || G > GNNPP_SUMMARY_MAX_GROUPS) return 0;
    return summary_out_bytes(N, G);
}

int gnnpp_rollout_summary(const gnnpp_rollout_summary_in* in, void* out, void* stream) {
    if (!in || !out || !in->reached || !in->stats || !in->target_makespan || !in->target_flowtime) return GNNPP_ERR_ARG;
    if (in->C <= 0 || in->N < 1 || in->G < 1 || in->G > GNNPP_SUMMARY_MAX_GROUPS || in->target_stride < 1)
        return GNNPP_ERR_ARG;
    if ((!in->group && in->G != 1) || (long long)in->C * in->N > 0x7fffffffLL) return GNNPP_ERR_ARG;
    if (reinterpret_cast<size_t>(out) & 7) return GNNPP_ERR_ARG;
    return rollout_summary_launch(*in, out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
