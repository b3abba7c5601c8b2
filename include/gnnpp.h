/*
 * gnnpp.h -- C ABI of libgnnpp.so: the MI355X (gfx950) implementation of the GNN policy forward
 * pass of proroklab/gnn_pathplanning (DecentralPlannerNet + GraphFilter / GraphFilterBatch).
 *
 * The reference has no FFI for this path (it is 100 % stock aten calls); the entry points below
 * are what a binding of the reference's Python call sites needs.  Every function cites the
 * reference interface it replaces (paths relative to the upstream repo root).
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless marked "host"; the caller owns every buffer;
 *     inputs are never written;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call only
 *     enqueues work on that stream and returns without synchronising;
 *   - return value 0 = success, negative = error (gnnpp_error_string()); a failed call has
 *     enqueued nothing;
 *   - fp32 everywhere; a GSO may be given as fp64 and is rounded to fp32 on load exactly like the
 *     reference's `S.float()` (utils/graphUtils/graphML.py:2350);
 *   - every forward entry point takes `precision` (GNNPP_PREC_*): the arithmetic of its matrix-pipe
 *     contractions, chosen PER CALL (no process-wide state: two streams / threads cannot change each other's
 *     schedule).  0 = GNNPP_PREC_FP32 is what an unchanged caller of the reference gets.
 */
#ifndef GNNPP_H_
#define GNNPP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNNPP_OK               0
#define GNNPP_ERR_ARG         (-1)   /* null pointer / non-positive size / inconsistent flags   */
#define GNNPP_ERR_UNSUPPORTED (-2)   /* shape outside what the kernels cover (see each call)     */
#define GNNPP_ERR_LAUNCH      (-3)   /* HIP launch error                                         */
#define GNNPP_ERR_RANGE       (-4)   /* GNNPP_PREC_SPLIT_F16 only: an activation left the f16 range  */

/* Arithmetic of the matrix-pipe contractions (encoder convolutions + compressMLP, the filter's tap
 * contraction).  Graph shifts, BatchNorm / bias / ReLU / pooling epilogues and the action head are exact fp32
 * in every mode; accumulation is fp32 in every mode.
 *   GNNPP_PREC_FP32 (default)  fp32-equivalent, NO input domain: every fp32 operand is represented exactly as
 *       three bf16 planes (x = h + m + l, fp32's exponent range) and a product keeps six of the nine plane
 *       products on v_mfma_f32_16x16x32_bf16 (dropped terms <= 2^-23 |w x|, below one fp32 rounding).  Where
 *       a kernel has no LDS room for the planes -- the general graph-filter kernel (lsigf_kernel) and the
 *       policy filter of teams whose rows + planes exceed the 160 KB LDS (N > ~64 agents, e.g. the 100-agent
 *       configuration) -- the contraction runs on the exact fp32 MFMA instead: exact as well, only slower.
 *   GNNPP_PREC_FP32_MFMA       v_mfma_f32_16x16x4_f32 everywhere: bitwise an fmaf chain, 2.7x more pipe time.
 *   GNNPP_PREC_SPLIT_F16       fast, NARROWER than fp32: operands as f16 hi + lo halves (22 significand bits)
 *       on v_mfma_f32_16x16x32_f16, valid for |activation| < 65504 only -- see "Range guard"; opt-in.  The graph
 *       filter's operand rows are scaled by a power of two before the split (largest |z| of a row in [2^13, 2^14),
 *       undone exactly on the accumulators), so its error is fp32-level at any scale from 65504 down to ~2^-50.
 *       The encoder's activations are split unscaled: there the lo half of a value far below 1 is an f16
 *       subnormal, an absolute error of ~2^-25 |w| per product that does not shrink with the activations. */
#define GNNPP_PREC_FP32        0
#define GNNPP_PREC_FP32_MFMA   1
#define GNNPP_PREC_SPLIT_F16   2

#define GNNPP_OBS_C        3         /* observation channels      (decentralplanner.py:89)       */
#define GNNPP_OBS_HW       11        /* observation height=width  (decentralplanner.py:22-23)    */
#define GNNPP_FEAT         128       /* numFeatures2Share         (decentralplanner.py:93,197)   */
#define GNNPP_ACTIONS      5         /* numAction                 (decentralplanner.py:27)       */
#define GNNPP_MAX_NODES    100       /* N <= 100 nodes per graph always fits (G, F <= 128)       */
#define GNNPP_MAX_ROWS     112       /* hard limit: a workgroup keeps <= 112 node rows in LDS; N in
                                        101..112 works when the 160 KB LDS budget allows (narrower
                                        G / F), else GNNPP_ERR_UNSUPPORTED.  Larger graphs: the same
                                        filter as dense GEMMs, one gnnpp_gemm_kmajor call per shift
                                        (A = S with strides (1, N), B = z_{k-1}) and one for the tap
                                        contraction -- what graphML._lsigf_large does --, or, forward
                                        only and up to GNNPP_ROLLOUT_MAX_TEAM nodes, the gnnpp_*_team_fwd
                                        calls below, which spread a graph over many workgroups        */

int         gnnpp_version(void);
const char* gnnpp_error_string(int code);

/* Process-wide tuning knobs (atomic; a concurrent call sees the old or the new value).  They choose between
 * SCHEDULES of the same arithmetic (launch geometry, kernel fusion): every setting computes the same function
 * to the last bit or two.  The arithmetic itself is the per-call `precision` argument, never a knob.  Knobs
 * that skip kernel phases for profiling are not part of this ABI (csrc/gnnpp_measure.h, -DGNNPP_MEASURE
 * builds only). */
#define GNNPP_TUNE_FILTER_GPW      1  /* graphs per workgroup of the filter kernel; 0 = heuristic */
#define GNNPP_TUNE_FILTER_WAVES    2  /* waves per workgroup of the filter kernel: 8, 16; 0 = auto */
#define GNNPP_TUNE_FILTER_SPLIT    7  /* 0 = heuristic (when one-graph workgroups fill at most half of the
                                         256 CUs: 2 .. 7 workgroups per graph, as many as keep one workgroup
                                         per CU, at most one per 16-row tile -- v320; v310: two at most);
                                         1 = never; n = 2 .. 7: n parts (clamped to the row tiles) whenever
                                         a workgroup holds one graph with >= 2 row tiles            */
#define GNNPP_TUNE_FUSED_POLICY     6  /* 1 (default): for teams of N <= 16 agents and K = 2, 3 or 4 taps
                                         (GNNPP_PREC_FP32 or GNNPP_PREC_SPLIT_F16), when B <= 512 graphs
                                         or N >= 13, gnnpp_policy_fwd is ONE kernel -- a workgroup
                                         encodes one graph's agents, then runs that graph's filter and
                                         action head on chip (identical logits); 0: always the encoder
                                         kernel followed by the filter kernel; 2: the one kernel for
                                         every batch size (measurement: tools/cp_ab.py)              */
#define GNNPP_TUNE_POLICY_FILTER    9  /* 1 (default): the filter + action head of gnnpp_policy_fwd / the rollout step
                                         for teams of 17 .. 100 agents (one graph per workgroup,
                                         FILTER_WAVES != 8) runs on the latency-scheduled policy_filter_kernel;
                                         0: on the general filter kernel (same logits to the last bit or two).
                                         (v310's value 2 -- bf16x3 planes beside compact neighbour lists for 65 ..
                                         100 agents, measured no faster -- was removed in v320: GNNPP_ERR_ARG)   */
#define GNNPP_TUNE_FILTER_SMALL     10  /* 1 (default): graph filters over many small graphs (GNNPP_PREC_FP32, N <= 16,
                                         G = F = 128, node-major rows, >= 64 workgroups) run on the
                                         throughput kernel lsigf_small_b3_kernel (bf16x3 planes, two workgroups per
                                         CU); 0: on the general filter kernel; 2: whenever the shape fits,
                                         however few graphs (tests); 3: the pipeline kernel whenever it fits */
#define GNNPP_TUNE_FILTER_SMALL_ROWS 11 /* rows per workgroup of that kernel: 0 = heuristic, 32 or 48 (fewer tap bytes per
                                         agent-step); 64 = the producer / consumer pipeline kernel
                                         (lsigf_pipe_b3_kernel: one persistent 8-wave workgroup per CU -- the heuristic
                                         takes it from 4096 groups of 64 rows on; FILTER_SMALL = 3 forces it too)  */
#define GNNPP_TUNE_FILTER_PIPE_GRID 12  /* persistent workgroups of the pipeline kernel: 0 (default) = one per CU */
#define GNNPP_TUNE_POLICY_CP        13  /* 1 (default): the one-launch policy kernel of teams of <= 12 agents puts (agent,
                                         position) pairs on the MFMA columns in its 5x5 layers (a 10-agent graph then
                                         fills 15/16 of those tiles instead of 10/16); 0 = agents on the columns for
                                         every team size.  Same logits to the bit either way (v310)                     */
#define GNNPP_TUNE_ENCODER_CP_TILE   14  /* agents per tile of the (unfused) encoder kernel's column-packed form: 0 (default)
                                         = heuristic -- M <= 2048 agents: tiles of ceil(M / 256) agents, one per CU
                                         (latency regime), else 16-agent tiles --, 1 .. 12 = that tile size for every
                                         M, 16 = always 16-agent tiles.  Same features to the bit (v310)                */
/* (keys 15 and 18 -- v320's GNNPP_TUNE_TRAIN_FORK, the weight-gradient kernels of gnnpp_encoder_train_bwd on a second
 * stream, and v330's GNNPP_TUNE_TRAIN_WGRAD_MERGED = 0, one weight-gradient launch per layer; both measured slower than
 * the one launch for all five layers behind the backward chain -- were removed: that launch is the only schedule, the
 * numbers are not reused, and gnnpp_set_tuning / gnnpp_get_tuning answer GNNPP_ERR_ARG)                             */
#define GNNPP_TUNE_FILTER_PLANE_ALIAS 16 /* 1 (default): the filter + head launch of teams whose bf16x3 operand planes do
                                         not fit the LDS beside the graph (65 .. 100 agents) keeps the planes in the z buffer
                                         that is dead while a tap is contracted -- possible whenever the graph is split
                                         over >= 2 workgroups -- instead of contracting on the exact fp32 MFMA (2.7x the
                                         matrix-pipe time); 0 = r05's behaviour.  Same accuracy class (v330)              */
#define GNNPP_TUNE_TRAIN_WGRAD_WGS   17  /* workgroups per layer of the training step's weight-gradient kernel (ONE launch for all
                                         five layers behind the backward chain; image splits x output-channel tiles): 0 (default) = by the batch (128 up to 1 280 agent-samples, 256
                                         beyond), or 16 .. 2048: more splits = shorter workgroups, more partial sums to add.
                                         The workspace size AND its layout depend on it, and the size query, _train_fwd and
                                         _train_bwd each read it again (the launch geometry is computed on the host): a C
                                         caller must hold ONE value from gnnpp_encoder_train_workspace_floats until the
                                         _train_bwd call on that workspace has returned -- under another value _train_bwd
                                         writes partial sums outside the allocation, and no call checks this.  The Python
                                         side enforces it: the autograd function of the train-mode encoder records the value
                                         it sized the workspace under and raises before any launch if the forward or the
                                         backward finds another.  Same gradients to rounding (v330)                    */
#define GNNPP_TUNE_TRAIN_RUNNING_FUSED 19 /* 1 (default): gnnpp_encoder_train_fwd updates the BatchNorm running statistics inside
                                         its last BatchNorm launch (the workgroups of a channel tile publish their statistics
                                         with an agent-scope release / ticket / acquire hand-off and the last one to arrive
                                         runs the N updates); 0: a launch of its own (r05).  Same statistics to the bit (v330) */
#define GNNPP_TUNE_ENCODER_ONE_PLANE 20  /* 1 (default): a tile of the bf16x3 encoder / one-launch policy kernel whose pixels are
                                         all exactly one bf16 (the simulator's {0, 1} observations) stores them packed and
                                         skips the m and l plane products; 0 (debug): every tile takes the three-plane
                                         path.  Same results to the bit (the skipped products are exact zeros)         */
int         gnnpp_set_tuning(int key, int value);
int         gnnpp_get_tuning(int key);   /* current value of a knob; GNNPP_ERR_ARG for an unknown key */

/* ------------------------------------------------------------------------------------------
 * Graph filter (LSIGF):  y = bias + sum_e sum_k W[:,e,k,:] . (x S_e^k),   z_k = z_{k-1} S (right
 * multiplication: node n gathers from the non-zeros of COLUMN n of S).
 * Replaces LSIGF (utils/graphUtils/graphML.py:48-141) and BatchLSIGF (:2273-2367), and with them
 * GraphFilter.forward (:1200-1219) / GraphFilterBatch.forward (:2458-2477).
 * ------------------------------------------------------------------------------------------ */

/* Number of floats of the MFMA-fragment-ordered copy of the filter taps h[F,E,K,G]. */
size_t gnnpp_filter_packed_floats(int G, int F, int K, int E);

/* Re-order h[F,E,K,G] (the nn.Parameter `weight`, graphML.py:1175 / :2434) into `packed`.
 * Call again whenever the parameter changes (load_state_dict, optimizer step). */
int gnnpp_filter_pack(const float* h, float* packed, int G, int F, int K, int E, void* stream);

/*
 * x        [B,G,Nin] feature-major (the module API, graphML.py:2459) when x_node_major == 0,
 *          [B,N,G]   node-major when x_node_major == 1 (requires Nin == N);
 * S        [B,E,N,N] when s_batched == 1 (BatchLSIGF), [E,N,N] when 0 (LSIGF, shared by the batch);
 *          element type double when s_is_f64 != 0, else float;
 * packed   from gnnpp_filter_pack;  bias [F] (bias_per_node == 0), [F,N] one value per feature and
 *          node (bias_per_node != 0; the reference's `b` is F x N or F x 1, graphML.py:2300-2302,
 *          :2365-2366), or NULL;
 * y        [B,F,Nin] when y_node_major == 0, [B,N,F] when 1;
 * Nin <= N: nodes Nin..N-1 of x are zero and the corresponding outputs are dropped
 *          (zero padding + index_select of graphML.py:1206-1218 / :2464-2476);
 * relu     apply max(.,0) to y (GFL[1], decentralplanner.py:221).
 * Limits:  1 <= N <= GNNPP_MAX_NODES at G,F <= 128 (LDS footprint); K >= 1; any F
 *          (more than 128 output features run as ceil(F/128) launches inside the call).
 * precision   GNNPP_PREC_*; range_flag  optional DEVICE int (NULL = no check), see "Range guard" below.
 */
int gnnpp_lsigf_fwd(const float* x, const void* S, const float* packed, const float* bias,
                    float* y, int B, int N, int Nin, int G, int F, int K, int E,
                    int s_is_f64, int s_batched, int x_node_major, int y_node_major, int relu,
                    int bias_per_node, int precision, int* range_flag, void* stream);

/* Range guard (GNNPP_PREC_SPLIT_F16 only; the other modes have no input domain and never touch the flag).
 * The split-f16 schedules feed the f16 matrix pipe with fp32 operands split in hi + lo halves (22 significand
 * bits), which is exact to ~2^-22 as long as every activation satisfies |x| < 65504 (the filter's rows
 * are power-of-two scaled first, so small values keep their 22 bits; the encoder's are not, see above).  A call
 * that hands a larger value to that pipe stores 1 to *range_flag (never cleared by the library; plain store, no
 * synchronisation added): the results of that call are then NOT trustworthy -- re-run it with
 * GNNPP_PREC_FP32.  gnnpp_error_string(GNNPP_ERR_RANGE) is the message the Python layer raises. */

/*
 * Training variant of gnnpp_lsigf_fwd (loss.backward() at agents/decentralplannerlocal.py:314):
 *   zs            optional out [E*K, B*N, G] node-major: every tap signal z_{e,k} = x S_e^k, so that
 *                 dW[f,e,k,g] = sum_{b,n} dy[b,f,n] z_{e,k}[b,n,g] is one library GEMM per tap;
 *   s_transposed  use S^T.  The input gradient of the filter is itself a filter,
 *                 dx = sum_k W_k^T . dy . (S^T)^k, i.e. this call with x := dy, taps packed from
 *                 h.permute(3,1,2,0) and s_transposed = 1.  This form always contracts on the exact
 *                 fp32 MFMA, whatever `precision` says (cotangents are far below the f16 normal range).
 * LIMIT: this call keeps a graph's rows in one workgroup's LDS: N <= GNNPP_MAX_ROWS (112; 100 guaranteed at
 * G = F = 128), else GNNPP_ERR_UNSUPPORTED.  Larger graphs train through the dense form described at GNNPP_MAX_ROWS,
 * forward AND backward as gnnpp_gemm_kmajor calls (shifts, tap contraction, dh = dy^T Z, dZ = dy h, the adjoint shift
 * chain dz_{k-1} += S dz_k): graphML._LSIGFFunction does exactly that (the reference trains on 10-agent teams,
 * configs/dcp_*.json, but BatchLSIGF itself has no size limit).
 */
int gnnpp_lsigf_fwd_save(const float* x, const void* S, const float* packed, const float* bias,
                         float* y, float* zs, int B, int N, int Nin, int G, int F, int K, int E,
                         int s_is_f64, int s_batched, int s_transposed, int x_node_major,
                         int y_node_major, int relu, int bias_per_node, int precision, int* range_flag,
                         void* stream);

/* 1 when a graph of N nodes with G input / F output features, K taps and E edge features fits the LDS-resident
 * filter kernels (gnnpp_lsigf_fwd / _save return GNNPP_OK for it), 0 when they answer GNNPP_ERR_UNSUPPORTED for
 * LACK OF LDS (N > GNNPP_MAX_ROWS, or fewer nodes with wide features), negative on invalid arguments.  The
 * reference's BatchLSIGF (utils/graphUtils/graphML.py:2273-2367) has no size limit: a caller uses this to tell
 * "take the dense-GEMM form" (what graphML._lsigf_large does) from any other GNNPP_ERR_UNSUPPORTED, which must
 * stay an error (v310). */
int gnnpp_lsigf_fits(int N, int G, int F, int K, int E);

/* ------------------------------------------------------------------------------------------
 * Per-agent encoder: 5 x (conv3x3 pad 1 -> BatchNorm(eval) -> ReLU [-> MaxPool 2]) -> flatten ->
 * Linear(128,128) -> ReLU.  Replaces ConvLayers + compressMLP as run by
 * DecentralPlannerNet.forward (graphs/models/decentralplanner.py:284-290; layers :155-195).
 * ------------------------------------------------------------------------------------------ */

/* Raw parameters in the reference's state_dict layout. */
typedef struct gnnpp_encoder_params {
    const float* conv_w[5];     /* ConvLayers.{0,4,7,11,14}.weight  [Cout,Cin,3,3]             */
    const float* conv_b[5];     /* ConvLayers.{0,4,7,11,14}.bias    [Cout]                     */
    const float* bn_w[5];       /* ConvLayers.{1,5,8,12,15}.weight  [Cout]                     */
    const float* bn_b[5];       /* ...bias                                                      */
    const float* bn_mean[5];    /* ...running_mean                                              */
    const float* bn_var[5];     /* ...running_var                                               */
    const float* fc_w;          /* compressMLP.0.weight [128,128]                               */
    const float* fc_b;          /* compressMLP.0.bias   [128]                                   */
    float        bn_eps;        /* 1e-5 (torch default, decentralplanner.py:163)                */
} gnnpp_encoder_params;

size_t gnnpp_encoder_packed_floats(void);

/* Fold eval-mode BatchNorm into a per-channel scale/shift and re-order all weights into MFMA
 * fragment order.  `params` is a HOST struct of DEVICE pointers. */
int gnnpp_encoder_pack(const gnnpp_encoder_params* params, float* packed, void* stream);

/* obs [M,3,11,11] (M = B*N agents, agent index b*N+n as in inputTensor[B,N,3,11,11]) ->
 * feat [M,128] node-major.  Any M >= 1. */
int gnnpp_encoder_fwd(const float* obs, const float* packed, float* feat, int M, int precision,
                      int* range_flag, void* stream);

/* ------------------------------------------------------------------------------------------
 * TRAIN-mode encoder, forward and backward (BASELINE config 4: loss.backward() at
 * agents/decentralplannerlocal.py:314 over the per-agent ConvLayers calls of
 * graphs/models/decentralplanner.py:284-287).  The reference runs the CNN once per agent, so BatchNorm
 * uses the statistics of (agent n, channel c) over that call's B samples, and updates its running
 * statistics N times per forward in agent order (momentum, unbiased variance): exactly that.
 *   obs        [B,N,3,11,11] (inputTensor); feat out [N,B,128] = flattened ConvLayers output per agent
 *              call (the input of compressMLP); dfeat [N,B,128] its gradient;
 *   workspace  gnnpp_encoder_train_workspace_floats(N, B) floats: holds the activations between
 *              forward and backward -- pass the SAME buffer, untouched, to the backward call;
 *   update_running != 0: p->bn_mean / p->bn_var are UPDATED in place (the one documented exception
 *              to "inputs are never written"; eval-mode packs must be rebuilt afterwards);
 *   feat_sample_major != 0: feat and dfeat are [B,N,128] instead (node-major rows: what gnnpp_lsigf_fwd takes
 *              with x_node_major, so that no transposing copy sits between encoder and graph filter);
 *   bn_num_batches  NULL, or the five BatchNorm2d.num_batches_tracked counters (int64, device): each is
 *              advanced by N, as the N forward calls of the reference do (with update_running only);
 *   g          where the gradients of the 20 parameter tensors go (overwritten, not accumulated).
 *   train_pack  NULL (the ten MFMA-fragment packs of the convolution weights are built inside the forward call, in
 *              the workspace), or the buffer gnnpp_train_pack filled from the CURRENT weights (v330: one pack launch
 *              per weight version -- shared with the graph filter's taps -- instead of one per forward call); the
 *              backward call must be given what the forward call was given.
 * fp32, deterministic (fixed-order reductions, no atomics).  compressMLP, the graph filter and the
 * action head are separate calls (gnnpp_linear_fwd / gnnpp_lsigf_fwd_save / gnnpp_lsigf_input_grad).
 * ------------------------------------------------------------------------------------------ */
typedef struct gnnpp_encoder_grads {
    float* conv_w[5];           /* d ConvLayers.{0,4,7,11,14}.weight  [Cout,Cin,3,3]             */
    float* conv_b[5];           /* d ...bias [Cout] (exactly zero in exact arithmetic: BatchNorm follows) */
    float* bn_w[5];             /* d ConvLayers.{1,5,8,12,15}.weight [Cout]                      */
    float* bn_b[5];             /* d ...bias                                                      */
} gnnpp_encoder_grads;

size_t gnnpp_encoder_train_workspace_floats(int N, int B);
int gnnpp_encoder_train_fwd(const gnnpp_encoder_params* p, const float* obs, float* workspace, float* feat,
                            int B, int N, float momentum, int update_running,
                            long long* const* bn_num_batches, int feat_sample_major, const float* train_pack,
                            void* stream);
int gnnpp_encoder_train_bwd(const gnnpp_encoder_params* p, const float* obs, float* workspace,
                            const float* dfeat, const gnnpp_encoder_grads* g, int B, int N,
                            int feat_sample_major, const float* train_pack, void* stream);

/* Every weight re-ordering the training step of config 4 needs, in ONE launch (v330; r05: five launches and a
 * transposing copy per step): the ten fragment packs of the convolution weights p->conv_w (-> train_pack,
 * gnnpp_train_pack_floats() floats, 16-byte aligned) and, for the graph filter's taps h [F,E,K,G]
 * (GraphFilterBatch.weight, graphML.py:2434), the fp32 fragments of the forward filter (-> taps_fwd, a buffer of
 * gnnpp_filter_packed_floats(G, F, K, E) floats) and of the input-gradient filter h^T [G,E,K,F] (-> taps_t,
 * gnnpp_filter_packed_floats(F, G, K, E) floats), read straight from h.  ONLY the fp32 region of the two tap buffers is
 * written: they serve gnnpp_lsigf_fwd_save with GNNPP_PREC_FP32 / _FP32_MFMA and gnnpp_lsigf_input_grad (the exact-fp32
 * contractions the training step runs), not the split-f16 or bf16x3 schedules.  p == NULL: taps only; h == NULL:
 * convolution weights only. */
size_t gnnpp_train_pack_floats(void);
int gnnpp_train_pack(const gnnpp_encoder_params* p, float* train_pack, const float* h, float* taps_fwd,
                     float* taps_t, int G, int F, int K, int E, void* stream);

/* Input gradient of the graph filter (graphML.py:2345-2366 run backwards): dx = sum_k (dy W_k) (S^T)^k, i.e. the
 * filter of the transposed taps h^T [G,E,K,F] on S^T applied to dy [.., F] -> dx [.., G]; packed_t = the taps_t of
 * gnnpp_train_pack (or gnnpp_filter_pack of h.permute(3,1,2,0)).  node_major != 0: dy [B,N,F], dx [B,N,G], and an
 * optional mask [B,N,G]: dx is stored as 0 where mask <= 0 -- the ReLU backward of the layer that produced the
 * filter's input (compressMLP's ReLU, decentralplanner.py:190), folded into this launch (v330).  Exact fp32. */
int gnnpp_lsigf_input_grad(const float* dy, const void* S, const float* packed_t, const float* mask, float* dx,
                           int B, int N, int G, int F, int K, int E, int s_is_f64, int s_batched, int node_major,
                           void* stream);

/* y = x W^T + bias (+ ReLU): forward of compressMLP (Linear 128 -> 128 + ReLU, decentralplanner.py:187-195, :289-290)
 * and of actionsMLP (Linear 128 -> 5, :232-243, :304-315) in the training step.  x [R,I], W [O,I] (nn.Linear's layout),
 * bias [O] or NULL, y [R,O].  Exact fp32 MFMA, fixed summation order.  I must be a multiple of 64 and x, W 16-byte
 * aligned; where O is a multiple of 4 the rows of y are stored as 16-byte vectors and y must be 16-byte aligned too
 * (GNNPP_ERR_UNSUPPORTED otherwise).  (v330; r05 ran these as library GEMMs + an aten ReLU.) */
int gnnpp_linear_fwd(const float* x, const float* W, const float* bias, float* y, int R, int I, int O, int relu,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * The rest of the optimisation step of config 4 (agents/decentralplannerlocal.py:287-317): the weight
 * gradients that are tall-contraction GEMMs, the loss, and the Adam update.  fp32, deterministic.
 * ------------------------------------------------------------------------------------------ */
/* C[b][m][n] = sum_k A_b(m,k) * B_b(k,n), b < batch, with element addresses
 *   A_b(m,k) = A + b*a_sb + m*a_sm + k*a_sk,   B_b(k,n) = B + b*b_sb + k*b_sk + n,   C_b(m,n) = C + b*c_sb + m*c_sm + n
 * (strides in floats).  The contraction is split over workgroups (fp32 MFMA) and the partial results are
 * summed in order: meant for small M x N (<= a few hundred) and long K, where a library GEMM runs on one
 * macro tile.  Serves the graph filter's tap gradient dh (graphML.py:2345-2352 backwards: A = dy [F,(b n)],
 * B = the saved shifted signals z_k [(b n),G], batch = E*K) and Linear weight gradients (A = dY^T, B = X).
 * workspace: gnnpp_gemm_workspace_floats(batch, M, N, K) floats (may be 0 -> NULL allowed). */
size_t gnnpp_gemm_workspace_floats(int batch, int M, int N, int K);
int gnnpp_gemm_kmajor(const float* A, long long a_sb, long long a_sm, long long a_sk, const float* B,
                      long long b_sb, long long b_sk, float* C, long long c_sb, long long c_sm, int batch,
                      int M, int N, int K, float* workspace, void* stream);
/* Up to 8 independent products of that kind in ONE launch (plus one for the ordered sums): the three
 * products of a Linear layer's backward pass (dx = dY W, dW = dY^T X, db = 1^T dY) cost two launches
 * instead of six.  workspace: gnnpp_gemm_multi_workspace_floats(d, count) floats. */
typedef struct gnnpp_gemm_desc {
    const float* A; long long a_sb, a_sm, a_sk;
    const float* B; long long b_sb, b_sk;
    float*       C; long long c_sb, c_sm;
    int batch, M, N, K;
    const float* mask;          /* NULL, or addressed like C: C(m,n) is stored as 0 where mask(m,n) <= 0 -- the ReLU
                                   backward of the layer whose output gradient this product is (v330) */
} gnnpp_gemm_desc;
size_t gnnpp_gemm_multi_workspace_floats(const gnnpp_gemm_desc* d, int count);
int gnnpp_gemm_kmajor_multi(const gnnpp_gemm_desc* d, int count, float* workspace, void* stream);

/* The training loop's loss (agents/decentralplannerlocal.py:296-312), forward and backward in one launch:
 *   logits [N,B,C] (agent-major: the list forward() returns, stacked), target [B,N,C] one-hot expert actions;
 *   loss[0] = (1/N) sum_n CrossEntropyLoss(logits[n], argmax_c target[:, n])   (first maximum, like torch.max);
 *   dlogits [N,B,C] = d loss / d logits, or NULL.  C <= 64.  The softmax in it is exp(x - max) / sum with the sum of
 *   those terms taken in double (not exp(x - logsumexp), which is rounded at the size of the largest logit): every
 *   gradient row sums to 0 within a few units in the last place of 1 / (N B), whatever the size of the logits.
 *   logits_sample_major != 0: logits and dlogits are [B,N,C] (the layout the train-mode forward computes). */
int gnnpp_policy_loss(const float* logits, const float* target, float* loss, float* dlogits, int B, int N,
                      int C, int logits_sample_major, void* stream);

/* torch.optim.Adam's update (amsgrad = False; L2 weight decay added to the gradient; bias correction) of up
 * to 32 tensors in one launch:  p, m (exp_avg), v (exp_avg_sq) are updated in place from g.
 *   state  8 floats on the device, zero before the first step: state[0] = number of steps taken so far, [1], [2] the
 *          bias-correction factors of the last tick, [3] scratch (a workgroup arrival counter, zero between calls),
 *          [4] .. [7] the betas and the factors of the NEXT step (precomputed by the tick's last workgroup);
 *   tick   != 0: this call is the first table of a step: it uses t = state[0] + 1 and its last workgroup stores t
 *          (v330: inside the same launch; pass 0 for further tables of the same step).  The counter lives on the
 *          device so that the call can be captured in a HIP graph. */
typedef struct gnnpp_adam_tensors {
    float* p[32];
    const float* g[32];
    float* m[32];
    float* v[32];
    long long numel[32];
    int count;
} gnnpp_adam_tensors;
int gnnpp_adam_step(const gnnpp_adam_tensors* t, float* state, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int tick, void* stream);

/* ------------------------------------------------------------------------------------------
 * Whole policy step: DecentralPlannerNet.addGSO + forward (decentralplanner.py:266-318):
 * encoder -> GraphFilterBatch(128,128,K,E=1) -> ReLU -> actionsMLP Linear(128,5).
 * ------------------------------------------------------------------------------------------ */
/*
 * obs      [B,N,3,11,11];  S [B,E,N,N] float or double (s_is_f64); E = 1 in the reference's
 *          configuration (decentralplanner.py:208; addGSO :266-276 handles E > 1);
 * enc_packed / filt_packed from the two pack calls (taps h[128,E,K,128]); gf_bias [128] (GFL.0.bias),
 * act_w [5,128], act_b [5] (actionsMLP.0.*);
 * feat_ws  workspace [B*N,128] (receives the encoder output, i.e. extractFeatureMap in
 *          node-major order);
 * logits   [N,B,5]: logits + n*B*5 is the contiguous [B,5] tensor of agent n, the n-th element
 *          of the list the reference returns (decentralplanner.py:303-318).
 */
int gnnpp_policy_fwd(const float* obs, const void* S, const float* enc_packed,
                     const float* filt_packed, const float* gf_bias, const float* act_w,
                     const float* act_b, float* feat_ws, float* logits, int B, int N, int K, int E,
                     int s_is_f64, int precision, int* range_flag, void* stream);

/* Last graph-filter layer + ReLU + action head of a planner with SEVERAL graph-filter layers
 * (decentralplanner.py:205-224 builds L layers, :293-315 runs them and the head): the earlier layers
 * are gnnpp_lsigf_fwd calls (node-major in/out, relu = 1); this call runs layer L on
 * x [B,N,G] node-major with taps h[F,E,K,G] (F <= 128), bias [F] or NULL, then Linear(F,5):
 * logits [N,B,5] as gnnpp_policy_fwd. */
int gnnpp_filter_head_fwd(const float* x, const void* S, const float* packed, const float* bias,
                          const float* act_w, const float* act_b, float* logits, int B, int N, int G,
                          int F, int K, int E, int s_is_f64, int precision, int* range_flag, void* stream);

/* Which schedule gnnpp_filter_head_fwd / the second launch of gnnpp_policy_fwd would run for this shape under the
 * current tuning: 0 split-f16 planes (v_mfma_f32_16x16x32_f16), 1 exact fp32 MFMA (v_mfma_f32_16x16x4_f32), 2 bf16x3 planes
 * (v_mfma_f32_16x16x32_bf16) in an LDS buffer of their own, 3 bf16x3 planes aliased onto the dead z buffer;
 * -1: the shape runs on the general filter kernels (lsigf_kernel / the small-graph kernels), GNNPP_ERR_ARG < -1 never.
 * The answer depends on B through the workgroups-per-graph heuristic (GNNPP_TUNE_FILTER_SPLIT): a measurement states
 * the instruction it priced from this call instead of guessing it.  (v330) */
int gnnpp_filter_head_mode(int B, int N, int K, int precision);

/* Action decode used by the rollout loop (utils/multirobotsim_dcenlocal.py:589-591: LogSoftmax
 * then argmax == argmax of the logits, first maximum wins like torch.max).
 * logits [N,B,5] -> actions [B,N] int32. */
int gnnpp_decode_actions(const float* logits, int* actions, int B, int N, void* stream);

/* The forward filter, the filter + ReLU + action head and the policy step for TEAM graphs: 1 <= N <=
 * GNNPP_ROLLOUT_MAX_TEAM (1024) nodes, the sizes gnnpp_rollout_*, gnnpp_expert_samples_team and gnnpp_mapf_team run
 * (csrc/lsigf_team_kernel.hip).  The function is that of gnnpp_lsigf_fwd / gnnpp_filter_head_fwd / gnnpp_policy_fwd
 * (z_k = z_{k-1} S: node n gathers from the non-zeros of COLUMN n), at any N in range -- not only beyond GNNPP_MAX_ROWS.
 * A graph is spread over many workgroups: one launch turns the dense S into per-column neighbour lists, one launch
 * per tap k = 1 .. K-2 shifts the signal through them (exact fp32, ascending row order), the last launch fuses the
 * last shift with the tap contraction, bias, ReLU and the store (or the action head).
 *   x [B,N,G] and y [B,N,F] node-major only (Nin == N: the caller zero-pads); logits [N,B,5];
 *   packed: what gnnpp_filter_pack wrote; bias [F], [F,N] (bias_per_node) or NULL;
 *   S fp32 or fp64 (s_is_f64), [B,E,N,N] (s_batched) or [E,N,N], any values, symmetric or not; NULL allowed at K = 1;
 *   1 <= G, F <= 128 (any value), K >= 1, E >= 1; gnnpp_policy_team_fwd: G = F = 128, S batched;
 *   precision: GNNPP_PREC_FP32 (bf16x3 planes, six products on v_mfma_f32_16x16x32_bf16) or GNNPP_PREC_FP32_MFMA;
 *     GNNPP_PREC_SPLIT_F16 returns GNNPP_ERR_UNSUPPORTED (gnnpp_policy_team_fwd keeps `range_flag` for the day it
 *     does not; it is never written);
 *   workspace: gnnpp_lsigf_team_workspace_bytes(B, N, G, K, E, s_batched) bytes (0 for arguments out of range),
 *     16-byte aligned, not NULL, not overlapping x / y / logits; its content is scratch.  Layout, every region 16-byte
 *     aligned, graphs = (s_batched ? B : 1) * E, Np = N rounded up to 4, Gz = G rounded up to 4:
 *       int32 cnt [graphs][N] | uint16 idx [graphs][N][Np] | fp32 val [graphs][N][Np]   (K > 1: the dense worst case,
 *       so the host never needs a degree) | fp32 z [E][K-2][B][N][Gz]   (K > 2).
 * Errors: N > GNNPP_ROLLOUT_MAX_TEAM, NULL pointers, non-positive sizes, a precision outside 0 .. 2, a workspace that
 * is too small or misaligned: GNNPP_ERR_ARG.  G or F > 128, split-f16: GNNPP_ERR_UNSUPPORTED.  On any error nothing is
 * enqueued and nothing is written.
 * No allocation, no host synchronisation, no atomics; every output and workspace element has one writer (two calls
 * give the same bytes); capturable in a HIP graph. */
size_t gnnpp_lsigf_team_workspace_bytes(int B, int N, int G, int K, int E, int s_batched);
int gnnpp_lsigf_team_fwd(const float* x, const void* S, const float* packed, const float* bias, float* y,
                         void* workspace, size_t workspace_bytes, int B, int N, int G, int F, int K, int E,
                         int s_is_f64, int s_batched, int relu, int bias_per_node, int precision, void* stream);
int gnnpp_filter_head_team_fwd(const float* x, const void* S, const float* packed, const float* bias,
                               const float* act_w, const float* act_b, float* logits, void* workspace,
                               size_t workspace_bytes, int B, int N, int G, int F, int K, int E,
                               int s_is_f64, int precision, void* stream);
/* gnnpp_policy_fwd's arguments, then the workspace (sized for G = 128, s_batched = 1): the encoder launch into
 * feat_ws [B*N,128], then the three steps above with the action head. */
int gnnpp_policy_team_fwd(const float* obs, const void* S, const float* enc_packed, const float* filt_packed,
                          const float* gf_bias, const float* act_w, const float* act_b, float* feat_ws,
                          float* logits, int B, int N, int K, int E, int s_is_f64, int precision,
                          int* range_flag, void* stream, void* workspace, size_t workspace_bytes);

/* Neighbour lists as an INPUT format of the team filter (the symbols below were added without a version change, like
 * the team calls above).  A lists block is the head of the team workspace: team_layout with graphs = (s_batched ? B : 1)
 * * E, every region 16-byte aligned, Np = N rounded up to 4:
 *     int32 cnt [graphs][N] | uint16 idx [graphs][N][Np] | fp32 val [graphs][N][Np]
 * Column n of graph g (g = b * E + e, or e for a shared graph) holds cnt entries (row index, weight) in ASCENDING row
 * order, padded with (0, 0.0f) up to the next multiple of four entries; entries behind the padding are unspecified and
 * never read.  Node n gathers z[n] = sum_j val[n][j] * z_prev[idx[n][j]] as an fmaf chain in list order.
 * Validity is the CALLER's contract -- the filter calls do not inspect a block: 0 <= cnt <= N, every index < N, the
 * padding present, the block at least gnnpp_team_lists_bytes(graphs, N) bytes.
 *   gnnpp_team_lists_bytes        size of the block; 0 for graphs <= 0 or N outside 1 .. GNNPP_ROLLOUT_MAX_TEAM.
 *   gnnpp_team_lists_from_dense   the lists of the non-zeros of S [graphs][N][N] (fp32, or fp64 rounded like
 *                                 `S.float()`): the launch the dense-S team calls make on every call, as a call of
 *                                 its own.  One launch.
 *   gnnpp_lsigf_team_lists_fwd / gnnpp_filter_head_team_lists_fwd / gnnpp_policy_team_lists_fwd
 *                                 the three team calls with `const void* S, int s_is_f64` replaced by `const void* lists`:
 *                                 no list launch, bit-identical outputs to the dense-S call on the S the lists were made
 *                                 from.  `workspace` keeps its size (gnnpp_lsigf_team_workspace_bytes) and holds the tap
 *                                 signals z; its lists region goes unused.  lists may be NULL at K = 1.
 * Errors (checked before any HIP call, nothing enqueued or written): a NULL pointer, a size out of range, a block or
 * workspace that is misaligned or too small: GNNPP_ERR_ARG; G or F > 128, split-f16: GNNPP_ERR_UNSUPPORTED.
 * No atomics, one writer per element (two calls give the same bytes), capturable in a HIP graph. */
size_t gnnpp_team_lists_bytes(int graphs, int N);
int gnnpp_team_lists_from_dense(const void* S, void* lists, size_t lists_bytes, int graphs, int N, int s_is_f64,
                                void* stream);
int gnnpp_lsigf_team_lists_fwd(const float* x, const void* lists, const float* packed, const float* bias, float* y,
                               void* workspace, size_t workspace_bytes, int B, int N, int G, int F, int K, int E,
                               int s_batched, int relu, int bias_per_node, int precision, void* stream);
int gnnpp_filter_head_team_lists_fwd(const float* x, const void* lists, const float* packed, const float* bias,
                                     const float* act_w, const float* act_b, float* logits, void* workspace,
                                     size_t workspace_bytes, int B, int N, int G, int F, int K, int E, int precision,
                                     void* stream);
int gnnpp_policy_team_lists_fwd(const float* obs, const void* lists, const float* enc_packed, const float* filt_packed,
                                const float* gf_bias, const float* act_w, const float* act_b, float* feat_ws,
                                float* logits, int B, int N, int K, int E, int precision, int* range_flag, void* stream,
                                void* workspace, size_t workspace_bytes);

/* TRAINING the team filter on neighbour lists (added without a version change, like the lists calls above;
 * csrc/lsigf_team_train_kernel.hip).  The input gradient of the filter is the filter on S^T with the taps of
 * h.permute(3,1,2,0): dx = sum_k W_k^T . dy . (S^T)^k.
 *   gnnpp_team_lists_transpose    lists_t := the block of S^T for the block `lists` of S (graphs graphs of N nodes, both
 *                                 of lists_bytes >= gnnpp_team_lists_bytes(graphs, N) bytes): column m of lists_t holds
 *                                 every n with m in column n of lists, in ascending n, with the same weight, then
 *                                 (0, 0.0f) up to a multiple of four entries.  No dense matrix, one launch.  The
 *                                 validity of `lists` is the caller's contract (ascending indices, 0 <= cnt <= N); an
 *                                 invalid block gives unspecified lists but never a write outside lists_t.
 *                                 lists == lists_t, NULL, a misaligned pointer or a block too small: GNNPP_ERR_ARG.
 *   gnnpp_lsigf_team_lists_fwd_save
 *                                 gnnpp_lsigf_team_lists_fwd that also writes every tap signal to zs [E*K][B*N][G]
 *                                 (node-major, row stride G: the layout of gnnpp_lsigf_fwd_save; tap (e, 0) is a copy of
 *                                 x).  One shift launch per k = 1 .. K-1 and the tail, which stages all K taps from zs.
 *                                 y is BYTE-IDENTICAL to gnnpp_lsigf_team_lists_fwd on the same arguments, in both
 *                                 precisions.  `workspace` is validated like that call's and not written.
 *   gnnpp_lsigf_team_lists_input_grad
 *                                 dx [B,N,G] for dy [B,N,F]: gnnpp_lsigf_team_lists_fwd(dy, lists_t, packed_t, no bias,
 *                                 dx, ..., G := F, F := G, no ReLU, GNNPP_PREC_FP32_MFMA), byte for byte.  packed_t:
 *                                 gnnpp_filter_pack of h.permute(3,1,2,0) [G,E,K,F]; workspace:
 *                                 gnnpp_lsigf_team_workspace_bytes(B, N, F, K, E, s_batched).
 * The tap and bias gradients are gnnpp_gemm_kmajor_multi products over zs.  Limits and errors as the lists calls: 1 <=
 * G, F <= 128 (any value), N <= GNNPP_ROLLOUT_MAX_TEAM, split-f16 GNNPP_ERR_UNSUPPORTED; nothing enqueued on failure;
 * no atomics, one writer per element, capturable. */
int gnnpp_team_lists_transpose(const void* lists, void* lists_t, size_t lists_bytes, int graphs, int N, void* stream);
int gnnpp_lsigf_team_lists_fwd_save(const float* x, const void* lists, const float* packed, const float* bias, float* y,
                                    float* zs, void* workspace, size_t workspace_bytes, int B, int N, int G, int F,
                                    int K, int E, int s_batched, int relu, int bias_per_node, int precision,
                                    void* stream);
int gnnpp_lsigf_team_lists_input_grad(const float* dy, const void* lists_t, const float* packed_t, float* dx,
                                      void* workspace, size_t workspace_bytes, int B, int N, int G, int F, int K,
                                      int E, int s_batched, void* stream);

/* ------------------------------------------------------------------------------------------
 * Batched rollout step around the forward (B independent episodes resident on the device):
 *   gnnpp_rollout_observe  AgentState.toInputTensor             dataloader/statetransformer.py:82-130
 *   gnnpp_rollout_gso      multiRobotSim.computeAdjacencyMatrix utils/multirobotsim_dcenlocal.py:320-365
 *                          (+ getGSO :367-394: radius bookkeeping)
 *   gnnpp_rollout_move     multiRobotSim.move :562-723 with interRobotCollision :462-555
 * One struct (HOST struct of DEVICE pointers) carries the episode state; each call reads the
 * fields of its section.  Integer / boolean / fp64 work: bit-exact against the simulator.
 * ------------------------------------------------------------------------------------------ */
/* Team sizes.  Teams of up to GNNPP_ROLLOUT_MAX_AGENTS agents run the one-wave kernels (one wavefront per episode
 * moves; gnnpp_rollout_step is one launch); gnnpp_rollout_policy_step(s) needs N <= 16 and refuses
 * N > GNNPP_ROLLOUT_MAX_AGENTS with GNNPP_ERR_ARG.  observe / gso / move / gso_observe / step accept up to
 * GNNPP_ROLLOUT_MAX_TEAM agents: beyond GNNPP_ROLLOUT_MAX_AGENTS they run the large-team kernels (one workgroup of
 * one thread per agent per episode for move and gso; step and gso_observe enqueue the separate launches), with the
 * same results.  Those need H * W <= GNNPP_ROLLOUT_TEAM_MAX_CELLS (the occupancy maps live in LDS); a larger map
 * returns GNNPP_ERR_UNSUPPORTED with nothing enqueued.  N > GNNPP_ROLLOUT_MAX_TEAM: GNNPP_ERR_ARG.  (v330: the
 * large-team range widens what the existing entry points accept and adds no symbol.)
 * Map sizes.  The one-wave calls keep the occupancy grid in LDS too, one byte per cell: observe / gso_observe / step
 * serve every map with H * W rounded up to 16 <= 65 536 cells (the same count as GNNPP_ROLLOUT_TEAM_MAX_CELLS; 256 x 256
 * is the largest square) at every team size, and answer GNNPP_ERR_UNSUPPORTED with nothing enqueued beyond it.  Up to
 * that limit no accepted call answers GNNPP_ERR_LAUNCH for its LDS: the launchers raise their kernels' dynamic LDS
 * limit above the default 64 KB (66 560 bytes for observe / gso_observe, 72 736 for step).  gnnpp_rollout_move and
 * gnnpp_rollout_gso have no map limit of their own (move reads the map from memory), and gnnpp_rollout_policy_step(s)
 * has a smaller one, stated below.
 * Coordinates.  At every team size rows and columns lie in [0, 65 535]: a map of GNNPP_ROLLOUT_TEAM_MAX_CELLS cells may
 * be 1 x 65 536 or 65 536 x 1.  Squared distances are compared as unsigned 32-bit words (65 535^2 + 0^2 < 2^32 - 1) and
 * cells as row * 65 536 + column modulo 2^32, both exact on that range; H, W > 65 536 is outside the contract
 * (gnnpp_rollout_move on a map of more than GNNPP_ROLLOUT_TEAM_MAX_CELLS cells, which it alone accepts: H, W <= 32 767). */
#define GNNPP_ROLLOUT_MAX_AGENTS 128
#define GNNPP_ROLLOUT_MAX_TEAM 1024
#define GNNPP_ROLLOUT_TEAM_MAX_CELLS 65536
#define GNNPP_TIE_LOWEST  0   /* colliding agent with the lowest index keeps its move          */
#define GNNPP_TIE_HASHED  1   /* counter-based hash of (seed, episode, step, call)             */
#define GNNPP_TIE_REPLAY  2   /* replay recorded random.choice outcomes (parity tests)         */
#define GNNPP_TIE_MT19937 3   /* CPython's random.choice itself on a per-episode Mersenne-Twister stream
                                 (rng_words): what the reference does at :489 after random.seed(s)  */

typedef struct gnnpp_rollout {
    /* episode state shared by the three calls */
    const unsigned char* grid;  /* [B,H,W] when grid_batched else [H,W]; 1 = obstacle           */
    int          grid_batched;
    const int*   goal;          /* [B,N,2] (row, col)                                           */
    int*         pos;           /* [B,N,2] current positions; updated by move                   */
    int          B, N, H, W;
    /* observe */
    float*       obs;           /* out [B,N,3,11,11]: obstacle FOV, goal / projected goal, agents */
    /* gso */
    double*      radius;        /* [B] communication radius, in/out (commR at step 0)           */
    float*       S;             /* out [B,N,N] = float(D^-1/2 A D^-1/2)                          */
    int*         connected;     /* out [B] or NULL                                              */
    int          grow;          /* 1 at step 0: radius /= 1.1, then *= 1.1 until connected      */
    /* move */
    const float* logits;        /* [N,B,5] from gnnpp_policy_fwd (argmax decoded here), or NULL */
    const int*   actions;       /* [B,N] action ids when logits == NULL                         */
    int*         reached;       /* [B,N] 0/1                 (count_reachgoal)                   */
    int*         start_step;    /* [B,N], -1 = None          (startStep_action_predict)          */
    int*         end_step;      /* [B,N], -1 = None          (endStep_action_predict)            */
    const int*   maxstep;       /* [B] per-episode step limit (rate_maxstep * makespanTarget)    */
    int*         done;          /* [B] in/out, or NULL.  The reference's loop stops calling move() for
                                   a case after the call that saw allReachGoal at entry, or ran with
                                   currentstep >= maxstep (agents/decentralplannerlocal.py:560-605).
                                   That call sets done[b] = 1; an episode with done[b] != 0 -- or, with
                                   or without this array, one called with currentstep > maxstep[b] -- is
                                   FROZEN: nothing of its state (pos, reached, steps, stats) changes  */
    int*         flags;         /* out [B,3]: allReachGoal at entry, moveCollision, predictCollision */
    int*         stats;         /* out [B,2]: makespan, flowtime (written when the episode ends) */
    int          currentstep;   /* 1-based step index, as the agent passes it (:588)            */
    int          tie_mode;      /* GNNPP_TIE_*: stands in for random.choice (:489)              */
    unsigned     seed;
    const short* choices;       /* [B,max_choices] recorded outcomes for GNNPP_TIE_REPLAY       */
    int*         choice_count;  /* out [B] tie-breaks consumed in this call, or NULL            */
    int          max_choices;
    int*         range_flag;    /* gnnpp_rollout_policy_step only: range guard of the policy, or NULL */
    const unsigned* rng_words;  /* GNNPP_TIE_MT19937: [B,rng_max] successive genrand_uint32() outputs of
                                   each episode's generator (random.Random(seed).getrandbits(32))   */
    int*         rng_cursor;    /* [B] in/out: words consumed so far                              */
    int          rng_max;
} gnnpp_rollout;

int gnnpp_rollout_observe(const gnnpp_rollout* r, void* stream);
int gnnpp_rollout_gso(const gnnpp_rollout* r, void* stream);
int gnnpp_rollout_move(const gnnpp_rollout* r, void* stream);
/* gnnpp_rollout_gso (grow = 0) and gnnpp_rollout_observe of the current positions in ONE launch: the two depend only
 * on the positions, so their workgroups run side by side (large teams, where one workgroup per episode is too
 * little for gnnpp_rollout_step).  Same results as the two calls. */
int gnnpp_rollout_gso_observe(const gnnpp_rollout* r, void* stream);
/* gnnpp_rollout_gso with the graph delivered as the team filter's neighbour lists (see "Neighbour lists as an INPUT
 * format" above; graphs = B) instead of a dense S: the block equals, over cnt and the first roundup4(cnt) entries of
 * every column, what gnnpp_team_lists_from_dense makes of gnnpp_rollout_gso's S on the same state (every weight is at
 * least 1 / 1023, so no edge is lost as a zero); radius and connected are the same to the bit.  r->S is ignored and may
 * be NULL; radius, connected and grow as for gnnpp_rollout_gso; the map is not used.  Any 1 <= N <=
 * GNNPP_ROLLOUT_MAX_TEAM (one workgroup per episode, one thread per agent: csrc/rollout_team_lists_kernel.hip).
 * lists: gnnpp_team_lists_bytes(B, N) bytes, 16-byte aligned; NULL, misaligned or too small: GNNPP_ERR_ARG, nothing
 * enqueued.  One launch, no atomics, two calls give the same bytes, capturable. */
int gnnpp_rollout_lists(const gnnpp_rollout* r, void* lists, size_t lists_bytes, void* stream);
/* move -> gso (grow = 0) -> observe of the new positions in ONE launch: the simulator work between
 * two policy forwards of a rollout (the loop agents/decentralplannerlocal.py:560-599 runs move,
 * then getCurrentState + getGSO of the next iteration).  Same results as the three calls in
 * sequence; fields as for those calls. */
int gnnpp_rollout_step(const gnnpp_rollout* r, void* stream);
/* A WHOLE rollout step in one launch for teams of N <= 16 agents (K = 2, 3 or 4): policy forward on r->obs /
 * r->S (fp32) with the packed encoder / filter weights, logits to r->logits [N,B,5], then move ->
 * gso -> observe as gnnpp_rollout_step; r->obs and r->S are overwritten with the next step's.
 * GNNPP_ERR_UNSUPPORTED (nothing enqueued) when the shape does not qualify (see GNNPP_TUNE_FUSED_POLICY;
 * precision GNNPP_PREC_FP32 or GNNPP_PREC_SPLIT_F16; H*W must fit the kernel's spare LDS: 10 208 cells under
 * GNNPP_PREC_FP32): use gnnpp_policy_fwd + gnnpp_rollout_step then. */
int gnnpp_rollout_policy_step(const gnnpp_rollout* r, const float* enc_packed, const float* filt_packed,
                              const float* gf_bias, const float* act_w, const float* act_b, int K,
                              int precision, void* stream);
/* nsteps consecutive calls of gnnpp_rollout_policy_step with currentstep = r->currentstep, +1, ...: the
 * inner loop of a rollout (agents/decentralplannerlocal.py:560-599) enqueued back to back, so the host
 * returns to its interpreter once per nsteps launches.  Episodes that end on the way freeze (see `done`);
 * GNNPP_TIE_REPLAY is per-call state and is refused (GNNPP_ERR_ARG). */
int gnnpp_rollout_policy_steps(const gnnpp_rollout* r, const float* enc_packed, const float* filt_packed,
                               const float* gf_bias, const float* act_w, const float* act_b, int K,
                               int nsteps, int precision, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training samples from expert schedules (the reference's offlineExpert/DataGen_Transformer.py:295-371, 466-515 and
 * onlineExpert/DataTransformer_local_onlineExpert.py): C solved cases, each a schedule of T_c states of N agents,
 * T_total = sum T_c steps in all, become per step the observation tensor, the normalised communication graph and
 * the one-hot expert action.  HOST struct of DEVICE pointers, like gnnpp_rollout.  Bit-exact with the reference:
 *   target[t,n]  one-hot of pos[t+1,n] - pos[t,n] in the order [-1,0] [0,-1] [1,0] [0,1] [0,0]; after a case's last
 *                state the next state is the goal (obtainSchedule)
 *   obs[t]       AgentState.toSeqInputTensor (== gnnpp_rollout_observe of the step's positions)
 *   graph        computeAdjacencyMatrix: the radius starts at radius0, is multiplied by 1.1 until the graph of a step
 *                is connected, is carried from step to step, and the FINAL radius rebuilds every step of the case.
 *                radius[c] = radius0 * 1.1 * ... (growth[c] fp64 multiplications);  S64 = (s_i * A_ij) * s_j with
 *                s = sqrt(1.0 / deg) in fp64, S = (float)S64.
 * status[c] != 0: the schedule is not one the reference would transform; obs / S / S64 / target of THAT case are
 * left unwritten, every other case is unaffected.
 * 2 <= N <= GNNPP_ROLLOUT_MAX_AGENTS (N = 1: GNNPP_ERR_UNSUPPORTED, N > GNNPP_ROLLOUT_MAX_AGENTS: GNNPP_ERR_ARG); the
 * map must fit the LDS occupancy grid (H * W <= 61 000, H, W <= 16384), else GNNPP_ERR_UNSUPPORTED; nothing is
 * enqueued on an error.  Three launches on `stream`, no host synchronisation, capturable in a HIP graph.
 * ------------------------------------------------------------------------------------------ */
#define GNNPP_SCHEDULE_BAD_MOVE  1   /* a move that is not one of the five deltas (the reference: ValueError)   */
#define GNNPP_SCHEDULE_BAD_STATE 2   /* a state off the map or on an obstacle                                    */
#define GNNPP_SCHEDULE_NO_RADIUS 4   /* no connected graph within 65535 radius growths (radius0 far too small)    */

typedef struct gnnpp_schedules {
    const unsigned char* grid;  /* [C,H,W] when grid_batched else [H,W]; 1 = obstacle                   */
    int          grid_batched;
    const int*   goal;          /* [C,N,2] (row, col)                                                   */
    const int*   pos;           /* [T_total,N,2] the cases' states, concatenated                        */
    const int*   case_start;    /* [C+1] first step of each case in pos; [0] = 0, [C] = T_total         */
    int          C, N, H, W, T_total;
    double       radius0;       /* 5.0 in both reference transformers                                   */
    float*       obs;           /* out [T_total,N,3,11,11]                                              */
    float*       S;             /* out [T_total,N,N]                                                    */
    double*      S64;           /* out [T_total,N,N], or NULL                                           */
    float*       target;        /* out [T_total,N,5] (what gnnpp_policy_loss reads)                     */
    double*      radius;        /* out [C] the radius every step of the case was built with             */
    int*         growth;        /* out [C] times the radius was multiplied by 1.1                       */
    int*         status;        /* out [C] 0, or GNNPP_SCHEDULE_* bits                                  */
    int*         step_info;     /* out [T_total]: growths step t needs on its own | its status bits << 16 (also
                                   the hand-over between the call's launches)                           */
} gnnpp_schedules;

int gnnpp_schedule_samples(const gnnpp_schedules* s, void* stream);

/* The same samples for teams of up to GNNPP_ROLLOUT_MAX_TEAM agents: the same struct, the same contract and the same
 * outputs, computed with one thread per agent and row tiles of S instead of one wave per step (expert_team_kernels.hip).
 * For every call BOTH entry points accept, every output of the two is identical, step_info included.
 * Limits: 2 <= N <= GNNPP_ROLLOUT_MAX_TEAM (N = 1: GNNPP_ERR_UNSUPPORTED, N > GNNPP_ROLLOUT_MAX_TEAM: GNNPP_ERR_ARG);
 * H * W <= GNNPP_ROLLOUT_TEAM_MAX_CELLS (the occupancy grid lives in LDS), else GNNPP_ERR_UNSUPPORTED; NULL pointers,
 * C > T_total, radius0 outside (0, 1e300), a workspace that is NULL, not 8-byte aligned or smaller than
 * gnnpp_schedule_team_workspace_bytes(N, T_total): GNNPP_ERR_ARG.  The checks come before any HIP call and nothing is
 * enqueued on an error.
 * workspace: device memory, no initial contents: s = sqrt(1 / deg) of every agent of every step in fp64
 * ([T_total, N]), the hand-over from the degree launch to the launches that store S by row tiles.
 * Outputs are indexed in size_t (T_total * N * N may pass 2^31).  When N % 4 == 0 and S / S64 are 16-byte aligned the
 * graphs are stored 16 bytes per lane; any other alignment is accepted and gives the same bytes.
 * Five launches on `stream`, no atomics, no host synchronisation, capturable in a HIP graph. */
size_t gnnpp_schedule_team_workspace_bytes(int N, int T_total);   /* 0 on invalid arguments */
int gnnpp_schedule_team_samples(const gnnpp_schedules* s, void* workspace, size_t workspace_bytes, void* stream);

/* The same samples with the graphs kept as CAPPED NEIGHBOUR LISTS up to training: no dense S is written anywhere (the
 * symbols below were added without a version change, like the lists calls; csrc/expert_team_lists_kernel.hip).
 * A capped lists set is three device arrays for `graphs` graphs of N nodes and a capacity `cap`, a multiple of 4 with
 * 4 <= cap <= roundup4(N), each array 16-byte aligned:
 *     int32 cnt [graphs][N]      uint16 idx [graphs][N][cap]      fp32 val [graphs][N][cap]
 * A column holds its cnt entries (row index, weight) in ASCENDING row order, then (0, 0.0f) up to the next multiple of
 * four entries; entries behind the padding are unspecified.  With cap == roundup4(N) the three arrays are the regions of
 * a standard lists block ("Neighbour lists as an INPUT format" above).  A standard block reserves roundup4(N) entries
 * per column, more bytes than the dense S; the schedules' graphs have a few dozen neighbours per agent, so a set sized
 * by the largest degree is what a sample pool can afford to keep (N = 1024, cap = 24: 152 KB per step, S: 4 MB).
 * The schedule's graph is symmetric bit for bit (the weight is (float)(s_i * s_j) in fp64): the lists of S are those of
 * S^T, gnnpp_lsigf_team_lists_input_grad takes them as they are.
 *   gnnpp_schedule_team_plan        the first three launches of gnnpp_schedule_team_samples -- target, radius, growth,
 *                                   status, step_info and the workspace, byte for byte what that call writes -- and one
 *                                   more for step_deg [T_total] (device): the largest degree of step t under its
 *                                   case's final radius, 0 for the steps of a flagged case.  s->obs, s->S and s->S64 may
 *                                   be NULL and are not written.  Arguments, limits and errors as
 *                                   gnnpp_schedule_team_samples; step_deg NULL: GNNPP_ERR_ARG.  Four launches.
 *   gnnpp_schedule_team_fill_lists  reads radius, status and the workspace as gnnpp_schedule_team_plan left them (same
 *                                   struct, same stream order) and writes s->obs and the capped lists of all T_total
 *                                   steps (graphs = T_total); s->S and s->S64 are ignored.  The lists of step t are, per
 *                                   column, the non-zeros of S[t] of gnnpp_schedule_team_samples.  The steps of a
 *                                   flagged case are left unwritten.  cnt always holds the TRUE degree: where it exceeds
 *                                   cap only the first cap entries are stored and nothing is written outside the
 *                                   column -- a consumer must treat cnt > cap as invalid (the caller sizes cap from
 *                                   step_deg: roundup4 of its maximum).  Errors as the plan call (s->obs required),
 *                                   plus a cap that is no multiple of 4 in 4 .. roundup4(N), a NULL or not 16-byte
 *                                   aligned cnt / idx / val: GNNPP_ERR_ARG.  Two launches.
 *   gnnpp_team_lists_gather         graph b of the standard block `lists` (gnnpp_team_lists_bytes(B, N) bytes, 16-byte
 *                                   aligned) := graph index[b] of the capped set of graphs_src graphs: cnt and the first
 *                                   roundup4(cnt) entries of every column -- what the team kernels read; where cnt > cap
 *                                   (an invalid set) cnt is copied as it is and cap entries.  index [B]: int32, device;
 *                                   indices may repeat; an index outside [0, graphs_src) is CLAMPED into that range
 *                                   (never an out-of-range read).  NULL / misaligned pointers, graphs_src or B <= 0, N
 *                                   outside 1 .. GNNPP_ROLLOUT_MAX_TEAM, a bad cap, a block too small: GNNPP_ERR_ARG.
 *                                   One launch.
 * The checks come before any HIP call and nothing is enqueued on an error.  No atomics, one writer per element (two
 * calls give the same bytes), no host synchronisation, capturable in a HIP graph. */
int gnnpp_schedule_team_plan(const gnnpp_schedules* s, void* workspace, size_t workspace_bytes, int* step_deg,
                             void* stream);
int gnnpp_schedule_team_fill_lists(const gnnpp_schedules* s, const void* workspace, size_t workspace_bytes, int* cnt,
                                   unsigned short* idx, float* val, int cap, void* stream);
int gnnpp_team_lists_gather(const int* cnt, const unsigned short* idx, const float* val, int graphs_src, int cap,
                            const int* index, int B, void* lists, size_t lists_bytes, int N, void* stream);

/* ------------------------------------------------------------------------------------------
 * MAPF solver: prioritized planning of C cases (the reference's SIPP expert option, offlineExpert/CasesSolver.py:517-539
 * `mapf_prioritized_sipp`, a binary without source).  Per case: a grid (1 = obstacle), starts / goals [N,2] (row, col),
 * R planning orders (permutations of the agents) and a horizon T_max.  Agents are planned one after another in the
 * order, each against the finished plans of the agents before it; agents after it are ignored.
 *   moves      up, left, down, right, stop; a move may not leave the map or enter an obstacle;
 *   parking    an agent stays on its goal from its arrival a_j on;
 *   conflicts  vertex: no cell an earlier agent (parked ones included) holds at the same t >= 1; swap: no move b -> a
 *              from t to t+1 while an earlier agent moves a -> b (following into a cell vacated in the same step is
 *              allowed, as in the reference simulator);
 *   layers     R_0 = {start}; R_{t+1} = free cells no earlier agent holds at t+1, reached from R_t by a stop or a move
 *              that is not a swap;
 *   arrival    a_i = the smallest t >= t_min with goal in R_t, t_min = 1 + the last t <= T_max an earlier agent holds the
 *              goal.  a_i > T_max (or the goal an earlier agent's parking cell): GNNPP_MAPF_NO_PATH, this agent is the
 *              failing one and no later agent is planned;
 *   path       walked back from (goal, a_i): the first predecessor in R_{t-1} in the order stop, then the cell that
 *              entered by up, left, down, right, whose move is not a swap;
 *   restarts   each order is planned on its own; the case keeps the best by: solved first, smallest flowtime sum a_i,
 *              smallest makespan max a_i, lowest restart index (an unsolved restart has flowtime = makespan = -1).
 * Outputs (every one written by the call):
 *   schedule [C,T_max+1,N,2]  positions; agents wait on their goal after arriving; agents left unplanned: -1
 *   arrival  [C,N]            a_i, -1 when unplanned;   makespan, flowtime [C]: -1 unless solved
 *   status   [C]              0 = solved, GNNPP_MAPF_* bits;   failing [C]: agent index or -1;   restart [C]: chosen or -1
 * A case with a start / goal off the map or on an obstacle, two equal starts or goals, or an order that is not a
 * permutation is GNNPP_MAPF_BAD_CASE (all its outputs -1, status 2); other cases are unaffected.
 * Limits: 1 <= N <= GNNPP_ROLLOUT_MAX_AGENTS, R >= 1, 0 <= T_max <= GNNPP_MAPF_MAX_STEPS (GNNPP_ERR_ARG);
 * H, W <= GNNPP_MAPF_MAX_SIDE, else GNNPP_ERR_UNSUPPORTED.  order == NULL: the index order, R must be 1.
 * workspace: gnnpp_mapf_workspace_bytes(C, R, H, T_max) bytes of device memory (no initial contents).  Deterministic,
 * no atomics; two or three launches on `stream`, no host synchronisation, capturable in a HIP graph; nothing is
 * enqueued on an error.
 * ------------------------------------------------------------------------------------------ */
#define GNNPP_MAPF_NO_PATH   1     /* an agent has no arrival within T_max                                     */
#define GNNPP_MAPF_BAD_CASE  2     /* invalid starts / goals / order                                           */
#define GNNPP_MAPF_MAX_SIDE  64    /* a map row is one 64-bit word, a map one wave of rows                       */
#define GNNPP_MAPF_MAX_STEPS 1024  /* T_max bound (the default horizon 4 (H + W) is at most 512)               */

typedef struct gnnpp_mapf {
    const unsigned char* grid;  /* [C,H,W] when grid_batched else [H,W]; 1 = obstacle                   */
    int          grid_batched;
    const int*   start;         /* [C,N,2] (row, col)                                                   */
    const int*   goal;          /* [C,N,2]                                                              */
    const int*   order;         /* [C,R,N] planning orders, or NULL (index order, R = 1)                */
    int          C, N, H, W, R, T_max;
    int*         schedule;      /* out [C,T_max+1,N,2]                                                  */
    int*         arrival;       /* out [C,N]                                                            */
    int*         makespan;      /* out [C]                                                              */
    int*         flowtime;      /* out [C] (ECBS's `cost`)                                              */
    int*         status;        /* out [C]                                                              */
    int*         failing;       /* out [C]                                                              */
    int*         restart;       /* out [C]                                                              */
    void*        workspace;     /* gnnpp_mapf_workspace_bytes(C, R, H, T_max) bytes                      */
    size_t       workspace_bytes;
} gnnpp_mapf;

size_t gnnpp_mapf_workspace_bytes(int C, int R, int H, int T_max);   /* 0 on invalid arguments */
int gnnpp_mapf_solve(const gnnpp_mapf* m, void* stream);

/* The same solver for large maps and teams: the same struct, the same contract and the same outputs, computed by one
 * workgroup per (case, restart) instead of one wave (a map row is ceil(W / 64) words, one thread per word).  For every
 * case BOTH calls accept, every output of the two calls is identical.
 * Limits: 1 <= N <= GNNPP_ROLLOUT_MAX_TEAM, R >= 1, 0 <= T_max <= GNNPP_MAPF_TEAM_MAX_STEPS (GNNPP_ERR_ARG);
 * H, W <= GNNPP_MAPF_TEAM_MAX_SIDE, else GNNPP_ERR_UNSUPPORTED (checked in this order, then the workspace).
 * workspace: a summary of C * R items followed by slots of (T_max + 1) * 6 * H * ceil(W / 64) 64-bit words, one per
 * concurrently planned item.  gnnpp_mapf_team_workspace_bytes returns the size for min(C * R, 256) slots (one workgroup
 * per compute unit at most).  The call accepts any buffer that holds the summary and at least ONE slot and runs
 * min(C * R, 256, slots that fit) workgroups (a full set for 256 x 256 maps at T_max = 2048 would be 25 GB); the outputs
 * do not depend on the number of slots.  Less than one slot: GNNPP_ERR_ARG.  Nothing is enqueued on an error. */
#define GNNPP_MAPF_TEAM_MAX_SIDE  256   /* a map row is up to four 64-bit words, a map up to 1024 threads           */
#define GNNPP_MAPF_TEAM_MAX_STEPS 2048  /* T_max bound (the default horizon 4 (H + W) of a 256 x 256 map)           */

size_t gnnpp_mapf_team_workspace_bytes(int C, int R, int H, int W, int T_max);   /* 0 on invalid arguments */
int gnnpp_mapf_team_solve(const gnnpp_mapf* m, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNPP_H_ */
