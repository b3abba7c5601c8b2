/* The train-mode encoder's convolutions on bf16x3 planes -- an OPT-IN training precision: four entry points of
 * libgnnpp.so, added without a version change (gnnpp_version() stays 330) and kept in a header of their own: gnnpp.h and
 * its companions are exactly what they were.  csrc/train_encoder_b3.hip; DESIGN.md 5.6.
 *
 * gnnpp_encoder_train_fwd / _bwd (gnnpp.h) run every convolution of the training step on v_mfma_f32_16x16x4_f32.  The
 * calls below are those two with a `precision` argument:
 *   GNNPP_PREC_FP32_MFMA  exact fp32: the call enqueues EXACTLY what gnnpp_encoder_train_fwd / _bwd enqueue for the same
 *                         arguments -- the same launches, the same bytes in every output and in the workspace.  pack_b3
 *                         is not read and may be NULL.
 *   GNNPP_PREC_FP32       bf16x3, the fp32-equivalent form every forward entry point uses under this value (gnnpp.h
 *                         "precision"): the nine convolution launches of a step (five forward convolutions, four input-
 *                         gradient convolutions; layer 0 has no input gradient) run conv_b3_kernel -- both operands as
 *                         three exact bf16 planes, six plane products, small terms first, on v_mfma_f32_16x16x32_bf16 with
 *                         fp32 accumulation.  No input domain, no range flag: any finite fp32 value is carried exactly.
 *                         Every other launch (BatchNorm forward / backward, the running statistics, the weight-gradient
 *                         launch and its reduction, which stay on the fp32 MFMA) is what the exact-fp32 call enqueues,
 *                         and reads the convolutions' results from the same layouts and workspace slots.
 *   any other value       GNNPP_ERR_UNSUPPORTED (GNNPP_PREC_SPLIT_F16 included: training has no 22-bit form).
 *
 * pack_b3 (GNNPP_PREC_FP32 only): the convolution weights as bf16x3 MFMA A fragments, gnnpp_train_pack_b3_bytes() bytes
 * of device memory, 16-byte aligned, filled by gnnpp_train_pack_b3 from the CURRENT p->conv_w -- ONE launch per weight
 * version, as gnnpp_train_pack: re-pack after every optimizer step or load of the weights; the calls cannot see a stale
 * pack.  It is a buffer of its own: gnnpp_train_pack and the layout of its buffer are untouched, and `train_pack` keeps
 * its meaning here (NULL: the fp32 fragment packs are built inside the forward call, in the workspace; under
 * GNNPP_PREC_FP32 the convolutions do not read them).  The backward call must be given the precision, the pack_b3 and the
 * train_pack the forward call on that workspace was given.
 *
 * Everything else -- arguments, layouts, the workspace of gnnpp_encoder_train_workspace_floats(N, B) floats (unchanged)
 * and the GNNPP_TUNE_TRAIN_* knobs -- is as documented for gnnpp_encoder_train_fwd / _bwd in gnnpp.h.
 *
 * Errors; every check comes before any HIP call and nothing is enqueued on one.
 *   GNNPP_ERR_UNSUPPORTED  precision is neither GNNPP_PREC_FP32 nor GNNPP_PREC_FP32_MFMA (checked first)
 *   GNNPP_ERR_ARG          GNNPP_PREC_FP32 with pack_b3 NULL or not 16-byte aligned; whatever gnnpp_encoder_train_fwd /
 *                          _bwd answer GNNPP_ERR_ARG for (a NULL pointer, a NULL parameter tensor, B or N <= 0, a
 *                          misaligned workspace or train_pack, update_running without running statistics);
 *                          gnnpp_train_pack_b3: p, a p->conv_w[i] or pack_b3 NULL, pack_b3 not 16-byte aligned
 *
 * Deterministic: fixed reduction orders, one writer per element, no atomics -- two identical calls give identical bytes.
 * No host synchronisation; capturable in a HIP graph like the calls of gnnpp.h. */
#ifndef GNNPP_TRAIN_B3_H_
#define GNNPP_TRAIN_B3_H_

#include "gnnpp.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t gnnpp_train_pack_b3_bytes(void);
int gnnpp_train_pack_b3(const gnnpp_encoder_params* p, void* pack_b3, void* stream);
int gnnpp_encoder_train_fwd_prec(const gnnpp_encoder_params* p, const float* obs, float* workspace, float* feat,
                                 int B, int N, float momentum, int update_running,
                                 long long* const* bn_num_batches, int feat_sample_major, const float* train_pack,
                                 void* stream, int precision, const void* pack_b3);
int gnnpp_encoder_train_bwd_prec(const gnnpp_encoder_params* p, const float* obs, float* workspace,
                                 const float* dfeat, const gnnpp_encoder_grads* g, int B, int N,
                                 int feat_sample_major, const float* train_pack, void* stream, int precision,
                                 const void* pack_b3);

#ifdef __cplusplus
}
#endif
#endif /* GNNPP_TRAIN_B3_H_ */
