/*
 * vitcnn.h — C ABI of the MI355X (gfx950) ViT-CNN training hot path.
 *
 * libvitcnn_hip.so exports one entry point per fused device op of the reference's
 * "ViT-CNN (ours)" model (Multimodality_Mamba, /root/reference/model/Multimodality_Mamba/
 * Mutimodality_Mamba7.py:1141-1181) and of its training iteration (model_utils.py:918-936).
 * The reference has no native layer of its own: each entry
 * point below replaces a PyTorch op sequence of the reference, cited per function, and is
 * what the reference's plugin (get_model -> nn.Module.forward / loss.backward /
 * optimizer.step) binds through the Python mirror in vit-cnn_amd/vitcnn_amd (ctypes).
 *
 * Conventions (all functions):
 *   - plain device pointers (fp32 unless stated; int32 index tables), sizes and leading
 *     dimensions in elements; activations are channels-last [rows, C] row-major;
 *   - the caller owns every buffer, including the fp32 workspace `ws` (ws_floats elements)
 *     that reductions use for fixed-order partial sums; nothing is allocated, nothing
 *     synchronises, so every call is capturable into a hipGraph;
 *   - work is enqueued on `stream`; return 0 on success, a hipError_t code on a launch
 *     failure, 1 (hipErrorInvalidValue) on an invalid shape — the Python mirror raises
 *     RuntimeError, like the reference's shape errors;
 *   - `beta_*` arguments select overwrite (0) or accumulate (1) for outputs that several
 *     backward branches feed.
 */
#ifndef VITCNN_H
#define VITCNN_H

#include <stddef.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
#define VC_API extern "C" __attribute__((visibility("default")))
#else
#define VC_API __attribute__((visibility("default")))
#endif

/* ---------------------------------------------------------------- dense contractions
 * C[b] = alpha * op(A[b]) op(B[b]) + beta*C[b] (+ bias[n]) (+ addend[(m % add_mod)*add_ld + n]) (ReLU if flags&1)
 * op(A)(m,k) = transA ? A[k*lda+m] : A[m*lda+k];  op(B)(k,n) = transB ? B[n*ldb+k] : B[k*ldb+n].
 * fp32 in / fp32 accumulate on v_mfma_f32_16x16x4_f32, or, with flags&2, bf16 operands (rounded
 * RNE as they are staged) with fp32 accumulation on v_mfma_f32_16x16x32_bf16 (the config-2 mode);
 * flags&4 / flags&8 force the k-major / K-contiguous fp32 kernel, flags&16 / flags&32 take / skip the
 * pipelined LDS-DMA fp32 kernel (default: chosen by shape).  flags&64 turns the addend into a mask:
 * the result (after alpha, beta, bias) is kept where addend[(m % add_mod)*add_ld + n] > 0 and zeroed
 * elsewhere -- a ReLU backward through that layer output, fused into the GEMM producing the gradient.
 * Split-K (fixed-order, deterministic) when the output grid is small and ws is given.  bias_grad (batch 1 only, may be null) additionally receives
 * alpha * sum_k op(A)(m,k) (+ beta * bias_grad[m]) through an implicit ones column of op(B): the
 * bias gradient of a layer rides along its weight-gradient GEMM.  Replaces nn.Conv2d 1x1 /
 * 3x3-after-im2col / nn.Linear / torch.matmul forward and backward (Mutimodality_Mamba7.py:258,
 * :1040, :1068, :1071, :101-134, :147, :152, :1098, :1124, :1160; transformers
 * modeling_mamba.py:372, :433, :438, :481). */
VC_API int vc_gemm(int transA, int transB, int M, int N, int K, float alpha,
                   const float* A, long lda, long strideA, const float* B, long ldb, long strideB,
                   float beta, float* C, long ldc, long strideC, int batch,
                   const float* bias, const float* addend, long add_ld, int add_mod, int flags,
                   float* bias_grad, float* ws, long ws_floats, hipStream_t stream);
/* vc_gemm with an in-launch split-K combine: tile_counters (n_counters >= the output tile count) is
 * a caller-owned unsigned array that is zero on entry and left zero; when split-K is chosen the
 * last-arriving slice of each tile sums the slices (same fixed order as vc_gemm's separate reduce
 * kernel: bit-identical results) instead of a second launch.  Counters must not be shared by
 * concurrently running calls (one array per stream).  NULL counters = vc_gemm. */
VC_API int vc_gemm_ex(int transA, int transB, int M, int N, int K, float alpha, const float* A, long lda,
                      long strideA, const float* B, long ldb, long strideB, float beta, float* C, long ldc,
                      long strideC, int batch, const float* bias, const float* addend, long add_ld, int add_mod,
                      int flags, float* bias_grad, float* ws, long ws_floats, unsigned int* tile_counters,
                      int n_counters, hipStream_t stream);

/* Measurement hook: force the tile (bm, bn in {64, 128}), split-K slice count, prefetch depth
 * (pf in {1, 2}) and combine path (combine: 1 in-launch, 0 separate reduce kernel) of the following
 * vc_gemm / vc_gemm_ex calls; 0 (-1 for combine) restores the automatic choice.  Only the probe
 * library (libvitcnn_probe.so, `make probe`; tools/gemm_sweep.py) keeps this state; the product
 * library keeps none and accepts only the automatic configuration (0, 0, 0, 0, -1). */
VC_API int vc_gemm_tune(int bm, int bn, int nsplit, int pf, int combine);

/* C [M, N] = A [M, K] W [N, K]^T + bias on the pipelined kernel (no split-K; flags & 2: bf16 operands) with the
 * BatchNorm statistics partials of C computed in the epilogue: colstats [ceil(M/64)][2][N] fp64 sums of (C - bias)
 * and (C - bias)^2 per 64-row tile -- the conv1x1 + BN forward's statistics pass folded into its GEMM
 * (vc_bn_apply_partials finishes the BatchNorm).  A, W 16-B aligned, K, lda, ldw multiples of 4. */
VC_API int vc_gemm_colstats(int M, int N, int K, const float* A, long lda, const float* W, long ldw, const float* bias,
                            float* C, long ldc, int flags, double* colstats, hipStream_t stream);
/* Grouped launches: a horizontal fusion of independent products (a layer's weight and data
 * gradients, parallel branches).  `group` is caller-owned host memory of VC_GEMM_GROUP_BYTES bytes
 * (8-byte aligned) holding the group's state -- the library keeps none, so distinct groups (one per
 * stream / thread) are independent and every entry point stays reentrant.  vc_gemm_group_begin
 * opens it for `stream`; vc_gemm_group_add takes vc_gemm_ex's arguments (minus the stream): fp32
 * problems of the k-major kernel and fp32 / bf16 problems of the pipelined 64x64 kernel are recorded;
 * anything else (bf16 problems on the legacy tiles, long K) launches at once on the group's stream;
 * vc_gemm_group_end launches the recorded problems as
 * one grid per kernel (up to 8 problems each) plus one grouped split-K reduce.  A problem's plan
 * depends on its shape and the workspace / counters passed to it only, so its result is bit-identical
 * grouped or alone.  The problems must not depend on each other; each takes its own
 * slice of the workspace and arrival counters passed to it.  Misuse (add / end on a group that is
 * not open) returns 1. */
#define VC_GEMM_GROUP_BYTES 16384
VC_API int vc_gemm_group_begin(void* group, hipStream_t stream);
VC_API int vc_gemm_group_add(void* group, int transA, int transB, int M, int N, int K, float alpha,
                             const float* A, long lda, long strideA, const float* B, long ldb, long strideB,
                             float beta, float* C, long ldc, long strideC, int batch, const float* bias,
                             const float* addend, long add_ld, int add_mod, int flags, float* bias_grad,
                             float* ws, long ws_floats, unsigned int* tile_counters, int n_counters);
VC_API int vc_gemm_group_end(void* group);

/* out[c] = beta*out[c] + sum_r X[r*ldx + c]  (bias gradients; fixed-order two-stage) */
VC_API int vc_colsum(int R, int C, const float* X, long ldx, float* out, float beta,
                     float* ws, long ws_floats, hipStream_t stream);
/* The same with >= ceil(C/64) zeroed arrival counters (left zero; per stream): the partials are
 * reduced in the last-arriving block of each column group, no second launch. */
VC_API int vc_colsum_ex(int R, int C, const float* X, long ldx, float* out, float beta,
                        float* ws, long ws_floats, unsigned int* counters, int n_counters, hipStream_t stream);

/* ---------------------------------------------------------------- normalisation
 * LayerNorm over the last dim (nn.LayerNorm eps=1e-6 via build_norm_layer,
 * mmpretrain/models/utils/norm.py:119-123; used at Mutimodality_Mamba7.py:656, :985,
 * :1083, :1085).  Saves per-row mean / rstd for the backward. */
VC_API int vc_layernorm_fwd(int R, int C, const float* x, long ldx, const float* w, const float* b, float eps,
                            float* y, long ldy, float* mean, float* rstd, hipStream_t stream);
VC_API int vc_layernorm_bwd(int R, int C, const float* dy, long lddy, const float* x, long ldx, const float* w,
                            const float* mean, const float* rstd, float* dx, long lddx, float beta_dx,
                            float* dw, float* db, float beta_w, float* ws, long ws_floats, hipStream_t stream);
/* The same with dx = res + LNgrad: the residual gradient is read from res (left untouched). */
VC_API int vc_layernorm_bwd_res(int R, int C, const float* dy, long lddy, const float* x, long ldx, const float* w,
                                const float* mean, const float* rstd, const float* res, long ldr, float* dx,
                                long lddx, float* dw, float* db, float beta_w, float* ws, long ws_floats,
                                hipStream_t stream);
/* Split form: dx now (res + LN grad, or beta_dx * dx + LN grad when res is null) with the dw / db
 * partials left in `part`; the parameter reduction later (same R, C, part_floats), e.g. on another
 * stream off the critical path.  Together bit-identical to vc_layernorm_bwd. */
VC_API int vc_layernorm_bwd_dx(int R, int C, const float* dy, long lddy, const float* x, long ldx, const float* w,
                               const float* mean, const float* rstd, const float* res, long ldr, float* dx,
                               long lddx, float beta_dx, float* part, long part_floats, hipStream_t stream);
VC_API int vc_layernorm_bwd_params(int R, int C, const float* part, long part_floats, float* dw, float* db,
                                   float beta_w, hipStream_t stream);

/* BatchNorm2d over channels-last rows (torch train/eval semantics, eps, momentum):
 * ms_conv_bn_relu.bn (Mutimodality_Mamba7.py:1039), FusionLayer BN (:1103, :1129),
 * NonLocal W[1] (:113).  train=1: batch stats (biased var) -> save_mean/save_invstd and the
 * running stats (unbiased var) are updated in place; train=0: save_* from running stats. */
VC_API int vc_bn_stats(int train, long M, int C, const float* x, long ldx, float eps, float momentum,
                       float* save_mean, float* save_invstd, float* run_mean, float* run_var,
                       float* ws, long ws_floats, hipStream_t stream);
/* stats + apply in one call (train: the partials kernel + a channel-tiled apply that reduces them itself,
 * two launches; eval: from the running statistics); bit-identical to vc_bn_stats + vc_bn_apply */
VC_API int vc_bn_forward(int train, long M, int C, const float* x, long ldx, float eps, float momentum,
                         float* save_mean, float* save_invstd, float* run_mean, float* run_var, const float* w,
                         const float* b, int relu, float* y, long ldy, float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_bn_apply(long M, int C, const float* x, long ldx, const float* mean, const float* invstd,
                       const float* w, const float* b, int relu, float* y, long ldy, hipStream_t stream);
VC_API int vc_bn_bwd(int train, long M, int C, const float* dy, long lddy, const float* x, long ldx,
                     const float* relu_out, long ldo, const float* mean, const float* invstd, const float* w,
                     float* dx, long lddx, float beta_dx, float* dw, float* db, float beta_w,
                     float* ws, long ws_floats, hipStream_t stream);
/* The same with zeroed arrival counters (left zero; per stream, as vc_gemm_ex's).  vc_bn_stats_ex and
 * vc_bn_bwd_ex without dx (>= ceil(C/64) counters) reduce per channel in the last-arriving partial block,
 * one launch fewer than without counters; vc_bn_forward_ex and vc_bn_bwd_ex with dx ignore them (the
 * channel-tiled apply reduces the partials itself: two launches).  Results are bit-identical with and
 * without counters. */
VC_API int vc_bn_forward_ex(int train, long M, int C, const float* x, long ldx, float eps, float momentum,
                            float* save_mean, float* save_invstd, float* run_mean, float* run_var, const float* w,
                            const float* b, int relu, float* y, long ldy, float* ws, long ws_floats,
                            unsigned int* counters, int n_counters, hipStream_t stream);
VC_API int vc_bn_stats_ex(int train, long M, int C, const float* x, long ldx, float eps, float momentum,
                          float* save_mean, float* save_invstd, float* run_mean, float* run_var,
                          float* ws, long ws_floats, unsigned int* counters, int n_counters, hipStream_t stream);
VC_API int vc_bn_bwd_ex(int train, long M, int C, const float* dy, long lddy, const float* x, long ldx,
                        const float* relu_out, long ldo, const float* mean, const float* invstd, const float* w,
                        float* dx, long lddx, float beta_dx, float* dw, float* db, float beta_w,
                        float* ws, long ws_floats, unsigned int* counters, int n_counters, hipStream_t stream);
/* train-mode BatchNorm forward from fp64 partials another kernel produced ([P][2][C]: per partial p, sum (x - shift[c])
 * and sum (x - shift[c])^2 over its rows; vc_gemm_colstats writes them with P = ceil(M / 64), shift = its bias):
 * save_* and the running statistics as vc_bn_forward, y = relu?(BN(x)); one launch */
VC_API int vc_bn_apply_partials(long M, int C, const float* x, long ldx, int P, const double* part, const float* shift,
                                float eps, float momentum, float* save_mean, float* save_invstd, float* run_mean,
                                float* run_var, const float* w, const float* b, int relu, float* y, long ldy,
                                hipStream_t stream);
/* vc_bn_bwd_ex through the ReLU that follows the BatchNorm, its decisions recomputed from x, the saved
 * statistics and the affine (w, b) with the forward's own arithmetic instead of read from the forward's
 * output: bit-identical to vc_bn_bwd_ex with relu_out = that output, one [M, C] read less per pass. */
VC_API int vc_bn_bwd_relu_ex(int train, long M, int C, const float* dy, long lddy, const float* x, long ldx,
                             const float* mean, const float* invstd, const float* w, const float* b, float* dx,
                             long lddx, float beta_dx, float* dw, float* db, float beta_w, float* ws, long ws_floats,
                             unsigned int* counters, int n_counters, hipStream_t stream);

/* ---------------------------------------------------------------- layout / spatial
 * NCHW input patches (the reference's batch layout, datasets.py:571-572) -> channels-last. */
VC_API int vc_nchw_to_nhwc(int B, int C, int HW, const float* x, float* y, hipStream_t stream);
/* the same into rows of ldy >= C floats with columns C .. ldy - 1 written 0 (FusAtNet's 1-band LiDAR input padded
 * to 4 channels: 16-B rows for the pipelined conv) */
VC_API int vc_nchw_to_nhwc_pad(int B, int C, int HW, const float* x, float* y, int ldy, hipStream_t stream);

/* 3x3 valid im2col of a channels-last [B,H,W,C] map with the preceding BatchNorm's affine
 * (bn_* may be null) fused in: col[(b,oh,ow), c*9+kh*3+kw] — ms_conv_bn_relu
 * (Mutimodality_Mamba7.py:1035-1048), column order matching the [Co, Ci, 3, 3] weight. */
VC_API int vc_im2col3x3(int B, int H, int W, int C, const float* x, const float* bn_mean, const float* bn_invstd,
                        const float* bn_w, const float* bn_b, float* col, hipStream_t stream);
/* Implicit-GEMM 3x3 convolution (no im2col matrix) over channels-last maps, k = c*9 + kh*3 + kw over
 * the torch weight [O][C][3][3] = [O][9C] (ms_conv_bn_relu, Mutimodality_Mamba7.py:1035-1048; FusAtNet
 * ConvUnit / ConvUnit_NP / Residual units, FusAtNet.py:9-60).  x [B,H,W,C] (row stride ldx); pad 0
 * (valid) or 1; output map [B,OH,OW,O], OH = H + 2 pad - 2.  bn_* (all or none): the preceding
 * BatchNorm's affine (x - mean) * invstd * w + b applied to in-range pixels as the operand is gathered.
 *   fwd:   y (ld ldy) = conv(x) + bias (ReLU if relu)
 *   wgrad: dweight [O][9C] = beta*dweight + dY^T im2col(x); dbias [O] (may be null) = beta*dbias + colsum(dY)
 *   dgrad: dx (ld lddx) = beta*dx + the conv's input gradient for dY [B,OH,OW,O] (ld lddy)
 * ws: split-K slabs (fixed-order sums); may be null (no split). */
VC_API int vc_conv3x3_fwd(int B, int H, int W, int C, int O, int pad, const float* x, long ldx, const float* bn_mean,
                          const float* bn_invstd, const float* bn_w, const float* bn_b, const float* weight,
                          const float* bias, int relu, float* y, long ldy, float* ws, long ws_floats,
                          hipStream_t stream);
VC_API int vc_conv3x3_wgrad(int B, int H, int W, int C, int O, int pad, const float* x, long ldx, const float* bn_mean,
                            const float* bn_invstd, const float* bn_w, const float* bn_b, const float* dy, long lddy,
                            float beta, float* dweight, float* dbias, float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_conv3x3_dgrad(int B, int H, int W, int C, int O, int pad, const float* dy, long lddy, const float* weight,
                            float beta, float* dx, long lddx, float* ws, long ws_floats, hipStream_t stream);
/* FusAtNet's 3x3 convs (FusAtNet.py:10-62, :168-186; stride 1, pad 0 or 1, channels-last rows) as
 * implicit GEMMs over a TAP-MAJOR contraction index k = tap * C + c (conv_tap.hip): operand tiles are
 * row gathers (one input row per output pixel and tap), no im2col matrix, no col2im.  Weights in
 * tap-major layouts made by vc_conv3x3_pack from the torch layout w [O][C][3][3]:
 *   mode 0: Wt [O][9][Cw] (fwd and dgrad), Cw = C rounded up to a multiple of 4, padding written 0
 *           (16-B aligned rows: float4 operand loads at any C)                mode 1: W2 [9][O][C]
 *   mode 2: w = beta w + dWt unpacked (wgrad's tap-major [O][9][C] gradient back to the torch layout)
 *   fwd:   y [B*OH*OW] (ld ldy) = conv(x) + bias (bias may be null); with C % 4 != 0 and ldx % 4 == 0 the
 *          row padding x[.][C .. C rounded to 4) is read (against zero weights) and must hold finite values
 *   wgrad: dWt [O][9][C] = sum over output pixels of dy x (overwritten; the bias gradient is colsum(dy))
 *   dgrad: dx (ld lddx) = beta dx + the conv's input gradient for dy
 * ws: split-K slabs when the tile grid is small (fixed-order sums; may be null: no split). */
VC_API int vc_conv3x3_pack(int O, int C, int mode, const float* src, float* dst, float beta, hipStream_t stream);
/* mode-0 packs of n convs in one launch per 48: shapes = host array {O0, C0, O1, C1, ...}, src / dst = host
 * arrays of n device pointers (torch-layout weights / Wt buffers); bit-identical to n vc_conv3x3_pack calls */
VC_API int vc_conv3x3_pack_many(int n, const int* shapes, const float* const* src, float* const* dst,
                                hipStream_t stream);
VC_API int vc_conv3x3_tap_fwd(int B, int H, int W, int C, int O, int pad, const float* x, long ldx, const float* wt,
                              const float* bias, float* y, long ldy, float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_conv3x3_tap_wgrad(int B, int H, int W, int C, int O, int pad, const float* x, long ldx, const float* dy,
                                long lddy, float* dwt, float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_conv3x3_tap_dgrad(int B, int H, int W, int C, int O, int pad, const float* dy, long lddy,
                                const float* wt, float beta, float* dx, long lddx, float* ws, long ws_floats,
                                hipStream_t stream);
/* wgrad written straight into the torch layout dw [O][C][3][3] (overwritten): vc_conv3x3_tap_wgrad +
 * vc_conv3x3_pack mode 2 with beta 0 in one call, bit-identical (the same sums, stored transposed); db
 * (nullable, overwritten) also receives the bias gradient sum over output pixels of dy (the blocks of the
 * first output tile column sum their staged dy tiles: no separate column-sum launches). */
VC_API int vc_conv3x3_tap_wgrad_oihw(int B, int H, int W, int C, int O, int pad, const float* x, long ldx,
                                     const float* dy, long lddy, float* dw, float* db, float* ws, long ws_floats,
                                     hipStream_t stream);
/* The four tap-major convs with `flags` (the plain entry points are these with flags 0, bit-identical).
 * VC_CONV_BF16 (bit value 2, as vc_gemm's flags & 2): both operands of the contraction are rounded RNE to bf16
 * as the MFMA fragments are formed -- x and Wt (fwd), dy and x (wgrad), dy and Wt (dgrad) -- and the products are
 * accumulated in fp32 (v_mfma_f32_16x16x32_bf16 over the same fp32 LDS stages on the pipelined route; rounded
 * operands on the fp32 MFMAs of the register-staged route: products of bf16 values are exact in fp32, so the two
 * routes compute the same sums).  The bias add, beta dx, the fused bias gradient db = colsum(dy) (unrounded dy),
 * the split-K slabs and their fixed-order combine stay fp32; zero padding stays zero; the split plans are those of
 * flags 0, so a result is run-to-run bit-identical.  Any other flag bit is refused. */
#define VC_CONV_BF16 2
VC_API int vc_conv3x3_tap_fwd_ex(int B, int H, int W, int C, int O, int pad, const float* x, long ldx,
                                 const float* wt, const float* bias, float* y, long ldy, float* ws, long ws_floats,
                                 int flags, hipStream_t stream);
VC_API int vc_conv3x3_tap_wgrad_ex(int B, int H, int W, int C, int O, int pad, const float* x, long ldx,
                                   const float* dy, long lddy, float* dwt, float* ws, long ws_floats, int flags,
                                   hipStream_t stream);
VC_API int vc_conv3x3_tap_wgrad_oihw_ex(int B, int H, int W, int C, int O, int pad, const float* x, long ldx,
                                        const float* dy, long lddy, float* dw, float* db, float* ws, long ws_floats,
                                        int flags, hipStream_t stream);
VC_API int vc_conv3x3_tap_dgrad_ex(int B, int H, int W, int C, int O, int pad, const float* dy, long lddy,
                                   const float* wt, float beta, float* dx, long lddx, float* ws, long ws_floats,
                                   int flags, hipStream_t stream);
/* bf16 operands stored in memory (FusAtNet precision "bf16_store").  The arithmetic contract
 * is VC_CONV_BF16's -- both operands of each contraction are the RNE bf16 roundings of fp32 values, products
 * accumulate in fp32; bias add, beta dx, split-K slabs and their fixed-order combine are fp32; zero padding stays
 * zero; results are run-to-run bit-identical -- but the rounding happens once, where the operand is written, and the
 * kernels move 2-byte elements through HBM, the DMA ring and LDS with no conversion in the loop (the k order inside an
 * MFMA differs from VC_CONV_BF16's, so the two are not bit-identical to each other).
 * A bf16 operand is a matrix of 2-byte elements with a leading dimension ld % 8 == 0 (elements) on a 16-B aligned
 * base whose columns [C, ld) are zero.
 *   vc_cast_bf16_2d: dst16 [M][ldd] = RNE bf16 of src [M][C] (ld lds), columns [C, ldd) written 0 (16-B stores).
 *   vc_conv3x3_pack_bf16_many: vc_conv3x3_pack_many writing Wt16 [O][9][Cw8], Cw8 = C rounded up to 8, padding 0;
 *     dst16 = host array of n device pointers, each 16-B aligned.
 *   vc_conv3x3_tap_fwd_h / _wgrad_oihw_h / _dgrad_h: the three implicit GEMMs of the tap-major conv over x16
 *     (ldx16), dy16 (lddy16) and Wt16, fp32 outputs with the epilogues of vc_conv3x3_tap_fwd / _wgrad_oihw / _dgrad.
 *     Any C and O; the weight gradient produces no bias gradient (db = vc_colsum_ex of the fp32 dy).
 * Anything else (ld % 8 != 0, a misaligned or null operand) is status 1 before any launch. */
VC_API int vc_cast_bf16_2d(long M, int C, const float* src, long lds, void* dst16, long ldd, hipStream_t stream);
VC_API int vc_conv3x3_pack_bf16_many(int n, const int* shapes, const float* const* src, void* const* dst16,
                                     hipStream_t stream);
VC_API int vc_conv3x3_tap_fwd_h(int B, int H, int W, int C, int O, int pad, const void* x16, long ldx16,
                                const void* wt16, const float* bias, float* y, long ldy, float* ws, long ws_floats,
                                hipStream_t stream);
VC_API int vc_conv3x3_tap_wgrad_oihw_h(int B, int H, int W, int C, int O, int pad, const void* x16, long ldx16,
                                       const void* dy16, long lddy16, float* dw, float* ws, long ws_floats,
                                       hipStream_t stream);
VC_API int vc_conv3x3_tap_dgrad_h(int B, int H, int W, int C, int O, int pad, const void* dy16, long lddy16,
                                  const void* wt16, float beta, float* dx, long lddx, float* ws, long ws_floats,
                                  hipStream_t stream);
/* vc_bn_forward_ex / vc_bn_bwd_relu_ex with an optional extra bf16 output (y16 / dx16, ld % 8 == 0 elements, 16-B
 * aligned; null: exactly the plain call): the RNE bf16 rounding of every value stored to y / dx, bit-equal to
 * vc_cast_bf16_2d of that fp32 output, columns [C, ld16) written 0.  The fp32 outputs and statistics are bit-equal
 * to the plain entry points'. */
VC_API int vc_bn_forward_ex_h(int train, long M, int C, const float* x, long ldx, float eps, float momentum,
                              float* save_mean, float* save_invstd, float* run_mean, float* run_var, const float* w,
                              const float* b, int relu, float* y, long ldy, void* y16, long ldy16, float* ws,
                              long ws_floats, unsigned int* counters, int n_counters, hipStream_t stream);
VC_API int vc_bn_bwd_relu_ex_h(int train, long M, int C, const float* dy, long lddy, const float* x, long ldx,
                               const float* mean, const float* invstd, const float* w, const float* b, float* dx,
                               long lddx, float beta_dx, void* dx16, long lddx16, float* dw, float* db, float beta_w,
                               float* ws, long ws_floats, unsigned int* counters, int n_counters, hipStream_t stream);
/* train-mode BatchNorm(x) (statistics as vc_bn_stats_ex: save_* and running stats written) followed by
 * vc_im2col3x3 of the normalised x, the statistics' final reduction done inside the im2col launch
 * (ms_conv_bn_relu's BN -> conv3x3, Mutimodality_Mamba7.py:1035-1048); bit-identical to the two calls. */
VC_API int vc_bn_im2col3x3(int B, int H, int W, int C, const float* x, float eps, float momentum, float* save_mean,
                           float* save_invstd, float* run_mean, float* run_var, const float* bn_w, const float* bn_b,
                           float* col, float* ws, long ws_floats, hipStream_t stream);
/* gradient of vc_im2col3x3 w.r.t. its (post-BN) input, gather form: dx [B,H,W,C] overwritten */
VC_API int vc_col2im3x3(int B, int H, int W, int C, const float* dcol, float* dx, hipStream_t stream);

/* vc_maxpool2_fwd of the phi | g map pg [B,Hs,Hs,2Ci] (row stride ldpg) followed by vc_nonlocal_attn_fwd, in
 * one launch where the wave-per-row forward runs (training batch sizes): pooled [B,P,2Ci] and arg are still
 * written for the backward. */
VC_API int vc_nonlocal_attn_pool_fwd(int B, int S, int P, int Ci, int Hs, const float* theta, const float* pg,
                                     long ldpg, float* pooled, unsigned char* arg, float* att, float* o,
                                     hipStream_t stream);
/* vc_nonlocal_attn_bwd followed by vc_maxpool2_bwd of the pooled phi | g map (Hs x Hs, P = (Hs/2)^2 keys), in
 * one launch where the MFMA backward applies: dpg [B,Hs,Hs,2Ci] overwritten (dpooled is then untouched;
 * it is the intermediate of the two-launch fallback). */
VC_API int vc_nonlocal_attn_pool_bwd(int B, int S, int P, int Ci, int Hs, const float* theta, const float* pooled,
                                     const float* att, const float* dout, const unsigned char* arg, float* dtheta,
                                     float* dpooled, float* dpg, hipStream_t stream);
/* nn.MaxPool2d(2) of the NonLocal phi/g branches (Mutimodality_Mamba7.py:94, :136-138):
 * x channels-last [B,H,W,C] with row stride ldx -> y [B,H/2,W/2,C] + winning tap (uint8). */
VC_API int vc_maxpool2_fwd(int B, int H, int W, int C, const float* x, long ldx, float* y, unsigned char* arg,
                           hipStream_t stream);
VC_API int vc_maxpool2_bwd(int B, int H, int W, int C, const float* dy, const unsigned char* arg, float* dx,
                           long lddx, hipStream_t stream);

/* ---------------------------------------------------------------- Mamba mixer (10 scan orders)
 * hsiMamba '81_2+8' / '49_2+8' (Mutimodality_Mamba7.py:608-701, :787-867) over transformers
 * MambaMixer (modeling_mamba.py:359-481).  order/inv_order: int32 [ndir, L] token order per
 * direction and its inverse; xz = in_proj(LN(tokens)) computed ONCE per token [B*L, 2D];
 * per-direction sequences are gathered through `order`, never materialised.
 * u [ndir*B*L, D] = SiLU(causal dwconv1d_k4(x-part) + bias). */
VC_API int vc_mamba_dirconv_fwd(int B, int L, int D, int ndir, const int* order, const float* xz,
                                const float* conv_w, const float* conv_b, float* u, hipStream_t stream);
/* selective scan of every direction's sequence (modeling_mamba.py:175-283), ungated:
 * yp[k,b,t,d] = sum_n C_t[n] h_t[d,n] + D_d u_t[d]; h_t = exp(dt A) h_{t-1} + dt B_t u_t,
 * dt = softplus(W_dt dtr_t + b_dt).  u/xdbl/yp are [ndir*B*L, D] / [.., R+32] / [.., D]. */
/* ckpt (nullable): [ndir*B][ceil(L/4)][16][D] fp32 states entering every 4-token segment, saved
 * for vc_mamba_scan_bwd; vc_mamba_scan_ckpt_floats gives its size (-1 on bad arguments) */
VC_API int vc_mamba_scan_ckpt_floats(int B, int L, int D, int ndir);
VC_API int vc_mamba_scan_fwd(int B, int L, int D, int R, int ndir, const float* u, const float* xdbl,
                             const int* order, const float* dt_w, const float* dt_b, const float* A_log,
                             const float* Dskip, float* yp, float* ckpt, hipStream_t stream);
/* ypsum[b,l,:] = sum_k softmax(gate_logits)_k yp[k, b, inv_k(l), :]  (un-permute + gate, :694-701);
 * ysum = ypsum * SiLU(z[b,l,:]) — the token-wise SiLU(z) gate of modeling_mamba.py:274 applied
 * once after the combine (it commutes with the permutation and the gated sum) */
VC_API int vc_mamba_combine_fwd(int B, int L, int D, int ndir, const int* inv_order, const float* gate_logits,
                                const float* yp, const float* xz, float* ypsum, float* ysum, hipStream_t stream);
/* backward of the SiLU(z) gate: dyp = dysum * SiLU(z); the z half of dxz (ld 2D) = dysum * ypsum * SiLU'(z) */
VC_API int vc_mamba_gate_bwd(int B, int L, int D, const float* xz, const float* ypsum, const float* dysum,
                             float* dyp, float* dxz, hipStream_t stream);
/* backward of scan + gated combine given dyp: du, ddt_lin (pre-softplus) per sequence position;
 * the B/C columns of dxdbl (ld R+32); dA_log [D,16], dDskip [D], dgate_logits [ndir] (all overwritten;
 * each may be NULL, its cross-sequence reduction is then skipped).
 * ckpt: the states vc_mamba_scan_fwd saved (nullable: recomputed into ws) */
VC_API int vc_mamba_scan_bwd(int B, int L, int D, int R, int ndir, const float* u, const float* xdbl,
                             const int* order, const float* dt_w, const float* dt_b, const float* A_log,
                             const float* Dskip, const float* gate_logits, const float* yp, const float* dyp,
                             const float* ckpt, float* du, float* ddt_lin, float* dxdbl, float* dA_log,
                             float* dDskip, float* dgate_logits, float* ws, long ws_floats, hipStream_t stream);
/* The parameter reductions of vc_mamba_scan_bwd (dA_log, D, gate logits) from the per-sequence partials a
 * call with null parameter outputs left at the head of its ws; run later / elsewhere, bit-identical. */
VC_API int vc_mamba_scan_bwd_params(int B, int D, int ndir, const float* gate_logits, const float* ws,
                                    float* dA_log, float* dDskip, float* dgate_logits, float* scratch,
                                    long scratch_floats, hipStream_t stream);
/* backward of gather + conv1d + SiLU: du is turned into dpre in place; the x half of dxz [B*L, 2D]
 * is overwritten (summed over the directions); conv weight [D,1,4] / bias [D] grads overwritten */
VC_API int vc_mamba_dirconv_bwd(int B, int L, int D, int ndir, const int* order, const int* inv_order,
                                const float* xz, const float* conv_w, const float* conv_b, float* du, float* dxz,
                                float* dconv_w, float* dconv_b, float* ws, long ws_floats, hipStream_t stream);
/* Fused forms (one launch each way per block on the critical chain; needs D % 4 == 0 and R <= 16 --
 * true for the model's (D, R) = (72, 9) and (128, 16)):
 * vc_mamba_scan_fwd_fused = vc_mamba_dirconv_fwd + xdbl = u x_proj_w^T (modeling_mamba.py:441-456) +
 * vc_mamba_scan_fwd in one kernel; u [ndir*B*L, D] (bit-identical to vc_mamba_dirconv_fwd) and xdbl
 * [.., R+32] are written for the backward. */
VC_API int vc_mamba_scan_fwd_fused(int B, int L, int D, int R, int ndir, const float* xz, const int* order,
                                   const float* conv_w, const float* conv_b, const float* x_proj_w,
                                   const float* dt_w, const float* dt_b, const float* A_log, const float* Dskip,
                                   float* u, float* xdbl, float* yp, float* ckpt, hipStream_t stream);
/* vc_mamba_scan_bwd followed, per sequence, by the dt_proj / x_proj data gradients and the conv1d + SiLU
 * backward (modeling_mamba.py:433-456 backward): dxdbl complete (all R+32 columns), dpre = d(conv
 * pre-activation) [ndir*B*L, D], ddt_lin and the scan parameter outputs as vc_mamba_scan_bwd, conv_part
 * [ndir*B][5D] the per-sequence conv weight / bias partials (reduce with vc_mamba_conv_params).  ckpt
 * required.  The x half of dxz then comes from vc_mamba_dirconv_bwd_gather. */
VC_API int vc_mamba_scan_bwd_fused(int B, int L, int D, int R, int ndir, const float* u, const float* xdbl,
                                   const int* order, const float* xz, const float* conv_w, const float* conv_b,
                                   const float* x_proj_w, const float* dt_w, const float* dt_b, const float* A_log,
                                   const float* Dskip, const float* gate_logits, const float* yp, const float* dyp,
                                   const float* ckpt, float* dpre, float* ddt_lin, float* dxdbl, float* conv_part,
                                   float* dA_log, float* dDskip, float* dgate_logits, float* ws, long ws_floats,
                                   hipStream_t stream);
VC_API int vc_mamba_dirconv_bwd_gather(int B, int L, int D, int ndir, const int* inv_order, const float* conv_w,
                                       const float* dpre, float* dxz, hipStream_t stream);
/* conv1d weight [D,1,4] / bias [D] gradients (overwritten) from vc_mamba_scan_bwd_fused's partials */
VC_API int vc_mamba_conv_params(int B, int D, int ndir, const float* conv_part, float* dconv_w, float* dconv_b,
                                hipStream_t stream);
/* vc_mamba_scan_bwd_params and vc_mamba_conv_params in ONE launch (round 6): dA_log, D, the gate logits and the
 * conv1d weight / bias gradients (all overwritten) from a deferred vc_mamba_scan_bwd_fused's partials (ws) and
 * conv_part; ndir <= 64 */
VC_API int vc_mamba_bwd_params(int B, int D, int ndir, const float* gate_logits, const float* ws, const float* conv_part,
                               float* dA_log, float* dDskip, float* dgate_logits, float* dconv_w, float* dconv_b,
                               hipStream_t stream);

/* ---------------------------------------------------------------- hsiMamba row chains
 * Two projections with a LayerNorm between them for 32-row blocks in one launch (rowchain.hip), fp32:
 * front (Mutimodality_Mamba7.py:651-656, modeling_mamba.py:433): t = x w_embed^T + pos[row % L],
 *   xn = LN(t) (ln_w, ln_b, eps; mean / rstd saved), out = xn w_proj^T   (K0, E, N2 <= 256, % 4 == 0);
 * back (:694-701, modeling_mamba.py:274, :481, Mutimodality_Mamba7.py:985, :1068): ypsum / ysum as
 *   vc_mamba_combine_fwd (bit-identical, ndir <= 10), t2 = ysum w_out^T + residual, g = LN(t2),
 *   out = g w_proj^T + b_proj.  Each replaces 3 / 4 launches of the separate path. */
VC_API int vc_rowchain_front(int rows, int K0, int E, int N2, const float* x, const float* w_embed, const float* pos,
                             int L, float* t, const float* ln_w, const float* ln_b, float eps, float* xn, float* mean,
                             float* rstd, const float* w_proj, float* out, hipStream_t stream);
VC_API int vc_rowchain_back(int B, int L, int D, int ndir, const int* inv_order, const float* gate_logits,
                            const float* yp, const float* xz, float* ypsum, float* ysum, int E, const float* w_out,
                            const float* residual, float* t2, const float* ln_w, const float* ln_b, float eps,
                            float* g, float* mean, float* rstd, int N2, const float* w_proj, const float* b_proj,
                            float* out, hipStream_t stream);

/* Backward chains (same blocking): back_bwd = change_dim's data gradient (dcd w_cd), the ln1 backward
 * (dt = LN grad; per-block dw / db partials into ln_part), out_proj's data gradient and the SiLU(z) gate
 * backward (dyp, the z half of dxz) -- the separate path's vc_gemm + vc_layernorm_bwd_dx + vc_gemm +
 * vc_mamba_gate_bwd; front_bwd = in_proj's data gradient (dxz w_in), the pre_norm backward with the
 * residual gradient (dtt = res + LN grad; partials) and dx = beta dx + dtt w_embed (+ dx_add) (dx and dx_add
 * nullable; dx_add: another branch's share of dx, e.g. computed concurrently on another stream).
 * vc_rowchain_ln_params reduces the partials (size: vc_rowchain_ln_part_floats).  Weight gradients of
 * the projections are separate vc_gemm calls. */
VC_API int vc_rowchain_back_bwd(int rows, int Cout, int E, int D, const float* dcd, const float* w_cd, const float* t2,
                                const float* mean, const float* rstd, const float* ln_w, float* dt, float* ln_part,
                                const float* w_out, const float* xz, const float* ypsum, float* dyp, float* dxz,
                                hipStream_t stream);
VC_API int vc_rowchain_front_bwd(int rows, int K0, int E, int Cin, const float* dxz, const float* w_in, const float* t,
                                 const float* mean, const float* rstd, const float* ln_w, const float* res, float* dtt,
                                 float* ln_part, const float* w_embed, float* dx, float beta, const float* dx_add,
                                 hipStream_t stream);
VC_API int vc_rowchain_ln_params(int rows, int E, const float* ln_part, float* dw, float* db, float beta,
                                 hipStream_t stream);
VC_API int vc_rowchain_ln_part_floats(int rows, int E);

/* ---------------------------------------------------------------- TokenLearner
 * TokenLearner(S) of SpatialAttention (Mutimodality_Mamba7.py:26-64) over x [B*HW, C] channels-last
 * (C % 4 == 0, ldx % 4 == 0, x / dZ 16-B aligned; HW, S within the LDS plans: vc_tl_check).  params: S x 5
 * floats [conv.0.weight(2),
 * conv.0.bias, conv.1.weight, conv.1.bias]; bn_buffers: S x 2 [running_mean, running_var]; stats: 2 S + 8
 * fp64 -- per token [mean, invstd] of its BN(1) input, then the shared moments of the pooled (max, mean)
 * pair [n, mbar, vbar, Cmm, Cmv, Cvv, Km, Kv] -- kept for the backward (statistics and gradient sums in
 * fp64, as torch's CPU BatchNorm accumulates); ws: vc_tl_ws_floats(B, HW, S) floats of per-call-site
 * scratch (8-B aligned).  vc_tl_pixel_stats leaves the moment partials in ws for vc_tl_fwd. */
VC_API int vc_tl_ws_floats(int B, int HW, int S);
/* 0 when vc_tl_pixel_stats / vc_tl_fwd / vc_tl_bwd support the shape (C <= 512; the tokens of the forward and the
 * pixels of the backward are chunked so their LDS fits: up to 20 x 20 pixel grids with S = 18 x 18 tokens),
 * 1 otherwise.  Host-only (no HIP call). */
VC_API int vc_tl_check(int HW, int C, int S);
/* per pixel row of x [M, C] (C <= 512): channel max, its first argmax, channel mean; + moment partials */
VC_API int vc_tl_pixel_stats(long M, int C, const float* x, long ldx, float* mx, int* amx, float* avg, double* ws,
                             hipStream_t stream);
/* stats (train: batch statistics from the moments, running statistics updated; eval: the running ones),
 * the attention maps a [B, S, HW] (may be null when no backward follows) and the pooled tokens Z [B, S, C] =
 * (1/HW) a x, in one launch */
VC_API int vc_tl_fwd(int train, int B, int HW, int C, int S, const float* x, long ldx, const float* mx,
                     const float* avg, const float* params, float* bn_buffers, float eps, float momentum,
                     const double* ws, double* stats, float* a, float* Z, hipStream_t stream);
/* backward from dZ [B, S, C]: dx [B*HW, C] (ld lddx, overwritten) = (1/HW) a^T dZ + the pooled-path gradient
 * (argmax channel and mean), dparams (S x 5, overwritten); a = the attention maps vc_tl_fwd wrote (round 6: the
 * backward reads them instead of recomputing them; the round-5 `da` scratch argument is gone).  Two launches.
 * Any C in 1..512 and any ldx / lddx >= C: the x and dZ rows are read by 16-B loads when C % 4 == 0, ldx % 4 == 0
 * and both bases are 16-B aligned (bit-identical to the earlier kernels there), by guarded loads otherwise. */
VC_API int vc_tl_bwd(int train, int B, int HW, int C, int S, const float* x, long ldx, const float* mx,
                     const float* avg, const int* amx, const float* params, const double* stats, const float* a,
                     const float* dZ, double* ws, float* dx, long lddx, float* dparams, hipStream_t stream);
/* mask [B, S, HW] uint8 = the ReLU decisions (BN(1) output > 0) vc_tl_fwd / vc_tl_bwd take, from the
 * same stats (test instrumentation: the float64 parity yardstick follows the HIP path's fp32 ties) */
VC_API int vc_tl_relu_mask(int B, int HW, int S, const float* mx, const float* avg, const float* params,
                           const double* stats, unsigned char* mask, hipStream_t stream);

/* ---------------------------------------------------------------- non-local cross attention
 * NONLocalBlock2D core (Mutimodality_Mamba7.py:143-152): softmax(theta phi^T) g, no scaling.
 * theta [B*S, Ci]; pooled [B*P, 2Ci] = maxpooled phi | g; att [B,S,P] saved; o [B*S, Ci]. */
VC_API int vc_nonlocal_attn_fwd(int B, int S, int P, int Ci, const float* theta, const float* pooled, float* att,
                                float* o, hipStream_t stream);
VC_API int vc_nonlocal_attn_bwd(int B, int S, int P, int Ci, const float* theta, const float* pooled,
                                const float* att, const float* dout, float* dtheta, float* dpooled,
                                hipStream_t stream);

/* ---------------------------------------------------------------- fusion glue, head, loss, optimiser */
/* torch.concat((x1, x2), 1) with ChannelExchange (even channels swapped) when exchange=1
 * (fusionBlock, Mutimodality_Mamba7.py:1133-1136; exchange semantics inferred) */
VC_API int vc_cat2_fwd(long M, int C1, int C2, const float* x1, long ld1, const float* x2, long ld2, int exchange,
                       float* out, hipStream_t stream);
VC_API int vc_cat2_bwd(long M, int C1, int C2, const float* dout, int exchange, float* dx1, long ld1, float beta1,
                       float* dx2, long ld2, float beta2, hipStream_t stream);
/* GLfusionBlock (:1112-1115 with NonLocal's W_y + z, :155-156): out [M, 2C] =
 * [ (BN(w_pre) + fc) + fl | fl + fc ] */
VC_API int vc_glf_combine_fwd(long M, int C, const float* w_pre, const float* bn_mean, const float* bn_invstd,
                              const float* bn_w, const float* bn_b, const float* fc, const float* fl, float* out,
                              hipStream_t stream);
/* train-mode BatchNorm statistics of w_pre (as vc_bn_stats_ex: save_* and running stats written) +
 * vc_glf_combine_fwd, the statistics' final reduction inside the combine launch */
VC_API int vc_bn_glf_combine(long M, int C, const float* w_pre, float eps, float momentum, float* save_mean,
                             float* save_invstd, float* run_mean, float* run_var, const float* bn_w, const float* bn_b,
                             const float* fc, const float* fl, float* out, float* ws, long ws_floats,
                             hipStream_t stream);
/* out = beta*out + a (+ b) over [M, C] strided rows */
VC_API int vc_add2_2d(long M, int C, const float* a, long lda, const float* b, long ldb, float* out, long ldo,
                      float beta, hipStream_t stream);
/* out = out2 = a + b, both overwritten (GLfusionBlock :1112-1115: the concat gradient summed into the
 * local- and channel-feature accumulators in one launch) */
VC_API int vc_add2_2d_dup(long M, int C, const float* a, long lda, const float* b, long ldb, float* out, long ldo,
                          float* out2, long ldo2, hipStream_t stream);
/* avgpool(f1) + avgpool(f2) -> feat [B,C]; logits = feat W^T + bias (Mutimodality_Mamba7.py:1174-1178) */
VC_API int vc_head_fwd(int B, int S1, int S2, int C, int ncls, const float* f1, const float* f2, const float* W,
                       const float* bias, float* feat, float* logits, hipStream_t stream);
VC_API int vc_head_bwd(int B, int S1, int S2, int C, int ncls, const float* dlogits, const float* W,
                       const float* feat, float* df1, float* df2, float* dW, float* db, hipStream_t stream);
/* nn.CrossEntropyLoss(weight) mean (model_utils.py:311): target int64, weight may be null */
VC_API int vc_ce_fwd(int B, int ncls, const float* logits, const long long* target, const float* weight,
                     long long ignore_index, float* loss, hipStream_t stream);
VC_API int vc_ce_bwd(int B, int ncls, const float* logits, const long long* target, const float* weight,
                     long long ignore_index, const float* grad_out, float* dlogits, hipStream_t stream);
/* vc_ce_fwd then vc_ce_bwd with grad_out = 1 in ONE launch (bit-identical to the two): the training step's
 * loss and dlogits */
VC_API int vc_ce_fwd_bwd(int B, int ncls, const float* logits, const long long* target, const float* weight,
                         long long ignore_index, float* loss, float* dlogits, hipStream_t stream);
/* torch.optim.AdamW step (model_utils.py:309-310) over a flat buffer; hyper = device
 * [lr, beta1, beta2, eps, weight_decay, grad_scale]; step = device float[3] state: step[0] = t is
 * incremented first, step[1..2] receive the bias corrections (1 - beta1^t, sqrt(1 - beta2^t)) */
VC_API int vc_adamw(long n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                    const float* hyper, float* step, hipStream_t stream);
/* ptr[idx[i]] += val  (BatchNorm num_batches_tracked counters) */
VC_API int vc_index_add_i64(int n, const int* idx, long long* ptr, long long val, hipStream_t stream);
/* dx = dy * (y > 0)  (nn.ReLU backward from the saved output) */
VC_API int vc_relu_bwd(long n, const float* dy, const float* y, float* dx, hipStream_t stream);
VC_API int vc_fill(long n, float* ptr, float value, hipStream_t stream);
/* ptr[m * ld + c] = value over [M, C] strided rows (e.g. the padding columns of a channel concat) */
VC_API int vc_fill_2d(long M, int C, float* ptr, long ld, float value, hipStream_t stream);
/* ptr[idx[i]] = value  (the alignment gaps of the flat gradient: parameters start 16-B aligned) */
VC_API int vc_fill_index(int n, const int* idx, float* ptr, float value, hipStream_t stream);

/* ---------------------------------------------------------------- patch windows (callers of the step)
 * The reference cuts patches on the host: MultiModalX.__getitem__ (datasets.py:550-593) for
 * training batches and sliding_window/grouper + np.copy for whole-image inference
 * (utils.py:357-415, :567-582; model_utils.py:1067-1132).  Here the image cube stays resident in
 * HBM in its source layout, img[x][y][c] ([W][H][C], band-contiguous, fp32), and windows are
 * gathered on the device straight into the model's [n][C][P][P] input layout.
 *
 * Window i's top-left corner: corners != NULL -> (corners[2i], corners[2i+1]);
 * corners == NULL -> the (k0+i)-th window of sliding_window(step, (P,P)), row-major over
 * (x outer, y inner) with the reference's clamping of the last window to W-P / H-P.
 * xform (optional, training augmentation of datasets.py:511-526): bit0 = np.fliplr, bit1 = np.flipud
 * (applied in that order), bits 2-3 = k of np.rot90(patch, k) (applied when no flip bit is set). */
VC_API int vc_window_count(int W, int H, int P, int step, long* count);
VC_API int vc_patch_gather(int W, int H, int C, int P, const float* cube, const int* corners, long k0, int step,
                           int n, const unsigned char* xform, float* out, hipStream_t stream);
/* probs[(x + P/2) * H + (y + P/2)][c] += (double)logits[i][c] for each window i (center_pixel
 * mode of model_utils.py:1126-1128; windows are distinct, so no two i share a centre) */
VC_API int vc_center_accumulate(int W, int H, int P, int ncls, const int* corners, long k0, int step, int n,
                                const float* logits, double* probs, hipStream_t stream);
/* MultiModalX radiation / mixture noise (datasets.py:529-545, applied at :565-568 to the HSI patch
 * after flip / rot90), in place on gathered patches x [n][C][P][P]:
 *   rad[i] != 0:  x = rad[i] * x + N/25                                   (radiation_noise)
 *   mix[2i] > 0:  x = (a1 * x + a2 * d2) / (a1 + a2) + N/25, (a1, a2) = mix[2i..2i+1]  (mixture_noise)
 * d2[c][p] = cube[pix[off[v] + r]][c], v = (int)lab[i][p] the (transformed) label window, r uniform in
 * [0, off[v+1] - off[v]) per (sample, pixel) -- the reference's np.random.choice over the samples of
 * class v; an empty class (ignored labels) leaves d2 = 0.  pix: x * H + y pixel indices of the cube.
 * N: standard normals and r from a counter-based hash of (seed, gid0 + i, stream, element) -- the
 * host draws the per-sample decisions and alphas in the reference's RNG order; the per-element fields
 * are drawn on the device. */
VC_API int vc_patch_noise(int n, int C, int P, int H, float* x, const float* lab, const float* rad,
                          const float* mix, const int* off, const int* pix, int nlab, const float* cube,
                          unsigned long long seed, long long gid0, hipStream_t stream);
/* vc_patch_gather over explicit corners whose windows may leave the scene by up to P / 2 on each side: the
 * reference's utils.padding_image (np.pad of P // 2, utils.py:320-344) folded into the gather's addresses, so no
 * padded copy of the cube exists.  border: 1 symmetric, 2 reflect, 3 constant zero, with np.pad's meaning -- for an
 * axis of length L and an index i outside [0, L): symmetric reads -i - 1 / 2L - 1 - i, reflect reads -i / 2L - 2 - i,
 * constant reads 0.0f.  corners (required) hold each window's top-left corner in scene coordinates, every component in
 * [-(P / 2), L - P + P / 2]; the result is defined for such corners only, but for ANY corner value the mapped index
 * is clamped into [0, L) last, so the kernel never reads outside the cube.  Output layout and xform codes are
 * vc_patch_gather's, and where no window leaves the scene the output equals vc_patch_gather's bit for bit.
 * Refused (status 1, before any launch): border outside 1..3 (0 = "no border" is vc_patch_gather: only its
 * caller can promise in-scene corners), W < P or H < P, reflect on an axis shorter than 2, null corners, and
 * vc_patch_gather's LDS bound. */
VC_API int vc_patch_gather_border(int W, int H, int C, int P, const float* cube, const int* corners, int n,
                                  const unsigned char* xform, int border, float* out, hipStream_t stream);
/* labels[(x + P/2) * H + (y + P/2)] = argmax_k logits[i][k] for each window i with corner (x, y) = corners[2i..2i+1]
 * (np.argmax of main.py:504 on the centre-pixel rows, without the probability map): the first maximum wins and a NaN
 * counts as the maximum, as in numpy.  A centre outside the scene (even P at the far edge) is skipped; the caller
 * supplies distinct centres.  labels: int64 [W][H]; 1 <= ncls <= 64 (the confusion matrix's bound). */
VC_API int vc_center_argmax(int W, int H, int P, int ncls, const int* corners, int n, const float* logits,
                            long long* labels, hipStream_t stream);

/* ---------------------------------------------------------------- the training feed's per-epoch randomness
 * (vitcnn_amd.window.epoch_order / device_decisions restate both entries in numpy)
 *
 * vc_epoch_shuffle: one epoch's sample order -- DataLoader(shuffle=True), main.py:433-440 -- and the rank's shard of
 * it, gathered from the full centre list on the device.
 *   base  = mix64((seed ^ VC_SHUFFLE_DOMAIN) + epoch)        wrapping 64-bit; mix64 is the splitmix64 finaliser of
 *   key_j = mix64(base + j) >> (64 - key_bits), j in [0, N)  vc_patch_noise
 *   perm  = the stable argsort of key: perm[r] = j for the j with exactly r pairs (key_j', j') < (key_j, j),
 *           compared key first and index second, so equal keys keep the smaller index first
 *   per   = ceil(N / world);  for t in [0, per):  src = perm[(rank + t * world) % N]
 *           corners_out[t] = corners[src], labels_out[t] = labels[src], order_out[t] = src (order_out may be NULL)
 * which is np.resize(perm, per * world)[rank::world]; world 1 is the whole permutation.  Independent uniform keys
 * sorted give a uniform permutation; at key_bits 64 ties do not occur in practice, smaller widths exist so that the
 * tie-break can be exercised.  corners [N][2] int32, labels [N] int64; the outputs hold per rows and nothing is
 * written past them.  One launch; the rank of an element is counted against all N keys (O(N^2) compares over LDS
 * tiles of recomputed keys), once per epoch.
 * Refused (status 1, before any launch): a null corners, labels, corners_out or labels_out; N outside
 * 1..VC_SHUFFLE_MAX; world < 1 or rank outside [0, world); key_bits outside 1..64. */
#define VC_SHUFFLE_MAX (1 << 17)
#define VC_SHUFFLE_DOMAIN 0xD1B54A32D192ED03ull
VC_API int vc_epoch_shuffle(int N, unsigned long long seed, unsigned long long epoch, int rank, int world,
                            int key_bits, const int* corners, const long long* labels, int* corners_out,
                            long long* labels_out, int* order_out, hipStream_t stream);
/* vc_aug_draw: the per-sample augmentation decisions of MultiModalX.__getitem__ (datasets.py:559-568, :511-535) for
 * samples gid0 .. gid0 + n - 1, one thread each, into the arrays vc_patch_gather* (xform) and vc_patch_noise (rad,
 * mix) read.  dkey = mix64(seed ^ mix64(gid << 2 | 3)) -- stream 3 of the noise hash, whose streams 0..2 are
 * vc_patch_noise's fields --; u_e = (mix64(dkey + e) >> 40) * 2^-24 for e = 0..9.
 *   VC_AUG_FLIP:      u0 > 0.5: xform = (u1 > 0.5) | (u2 > 0.5) << 1 (both clear is an outcome)
 *                     else u3 > 0.5: xform = (1 + min(2, (int)(3.0f * u4))) << 2; else 0
 *   VC_AUG_RADIATION: u5 < 0.1f: rad = fmaf(0.2f, u6, 0.9f); else 0
 *   VC_AUG_MIXTURE:   u7 < 0.2f: mix = (fmaf(0.99f, u8, 0.01f), fmaf(0.99f, u9, 0.01f)); else (0, 0)
 * An augmentation whose flag is clear writes zeros.  Each value is one fused multiply-add of float32 operands, i.e.
 * the exact result rounded once.  xform [n] uint8, rad [n] float, mix [n][2] float, all written in full.
 * Refused (status 1, before any launch): n < 0, flag bits outside the three, a null output with n > 0. */
#define VC_AUG_FLIP 1
#define VC_AUG_RADIATION 2
#define VC_AUG_MIXTURE 4
VC_API int vc_aug_draw(int n, int flags, unsigned long long seed, long long gid0, unsigned char* xform, float* rad,
                       float* mix, hipStream_t stream);

/* ---------------------------------------------------------------- classification metrics
 * Confusion matrix of a prediction map (utils.py:585-663 metrics(), counting step :596-611):
 * cm[t * n_classes + p] += number of pixels with target t, prediction p, both in
 * [0, n_classes), target not flagged in ignored[n_classes] (uint8).  cm (uint64) is
 * accumulated into: zero it first.  n_classes <= 64. */
VC_API int vc_confusion_matrix(long n, const long long* target, const long long* pred, int n_classes,
                               const unsigned char* ignored, unsigned long long* cm, hipStream_t stream);

/* ---------------------------------------------------------------- S2EFT (config 5)
 * model/compare_method/S2EFT.py.  Token rows are [B, T, D] row-major, T = N + 1 (cls first).
 * vc_s2eft_gate_fwd: spectral gate :134-143 (x [B,N,C]; w = conv1d weight [1,2,7] (mean, max),
 *   bias [1]): mask[b,t] = sigmoid(conv1d_k7_pad3([mean_c x, max_c x]))[t] >= beta; xg = x * mask
 *   (the reference thresholds `.data`: no gradient reaches the gate).
 * vc_s2eft_patch_gate_fwd: the same gate straight from the two NCHW patches x1 [B,C1,P,P], x2 [B,C2,P,P]
 *   (x2 may be null when C2 = 0), over the circular neighbour-band token rows, which are never stored:
 *   with r = cat(x1, x2) over channels viewed [B, N = C1 + C2, P*P] and near in {1, 3},
 *   tokens[b, j, s*P*P + p] = r[b, (j + s - near/2) mod N, p]  (row j = previous, this, next band; the LiDAR
 *   band neighbours the last HSI band and HSI band 0); xg [B, N, near*P*P] = tokens * mask, mask [B, N] as
 *   vc_s2eft_gate_fwd's on tokens.  A token's mean is its slots' band sums added in slot order over
 *   (float)(near*P*P), its max the fmaxf chain of the band maxima: a mask can differ from vc_s2eft_gate_fwd's on
 *   materialised tokens only where the sigmoid is within fp32 rounding of beta.  w null: no gate (xg = tokens,
 *   mask = 1 where mask is given; bias and mask may be null).  N <= 4096, N*near*P*P < 2^31.
 * vc_s2eft_cls_rows: X[b,0,:] = cls + pos[0] (:150-152); vc_s2eft_strip_cls: dE = dX[:,1:,:].
 * vc_s2eft_attn_fwd/bwd: Attention :45-74 core, dim_head 16, softmax(q k^T * scale) v over
 *   qkv [B*T, 3*H*16] (to_qkv output, q|k|v blocks); out [B*T, H*16]; lse [B,H,T] saved; T <= 256.
 * vc_gelu_fwd/bwd: nn.GELU (erf form, FeedForward :25).
 * vc_s2eft_skip_pack/unpack/bias_grad: CAF skipcat Conv2d(T, T, [1,2]) (:88-106) as a GEMM with the
 *   weight viewed [T, 2T] over Z[b] = interleave(x, last) [2T, D]; biasmat [T, D] = bias broadcast. */
VC_API int vc_s2eft_gate_fwd(int B, int N, int C, const float* x, const float* w, const float* bias, float beta,
                             float* xg, float* mask, hipStream_t stream);
VC_API int vc_s2eft_patch_gate_fwd(int B, int C1, int C2, int P, int near, const float* x1, const float* x2,
                                   const float* w, const float* bias, float beta, float* xg, float* mask,
                                   hipStream_t stream);
VC_API int vc_s2eft_cls_rows(int B, int T, int D, const float* cls, const float* pos, float* X, hipStream_t stream);
VC_API int vc_s2eft_strip_cls(int B, int N, int D, const float* dX, float* dE, hipStream_t stream);
VC_API int vc_s2eft_attn_fwd(int B, int T, int H, const float* qkv, float scale, float* out, float* lse,
                             hipStream_t stream);
VC_API int vc_s2eft_attn_bwd(int B, int T, int H, const float* qkv, const float* out, const float* dout,
                             const float* lse, float scale, float* dqkv, hipStream_t stream);
VC_API int vc_gelu_fwd(long n, const float* x, float* y, hipStream_t stream);
VC_API int vc_gelu_bwd(long n, const float* dy, const float* x, float* dx, hipStream_t stream);
VC_API int vc_s2eft_skip_pack(int B, int T, int D, const float* x, const float* last, const float* bias, float* Z,
                              float* biasmat, hipStream_t stream);
/* the skipcat backward's split of dZ [B, T, 2, D]: dx = (acc_x ? dx : 0) + dZ[:, :, 0] (+ addx, may be null: a
 * residual gradient folded in), dlast = dZ[:, :, 1] (overwritten, round 6: each layer's is written once) */
VC_API int vc_s2eft_skip_unpack(int B, int T, int D, const float* dZ, float* dx, int acc_x, const float* addx,
                                float* dlast, hipStream_t stream);
VC_API int vc_s2eft_skip_bias_grad(int B, int T, int D, const float* dY, float* db, hipStream_t stream);
/* nn.Dropout(p) in training (S2EFT emb_dropout :120, to_out :43, FeedForward :26, :28):
 * keep = hash(seed, i) >= p (counter-based), y = add + keep * x / (1 - p) (add may be null, y may
 * alias x), mask[i] = keep; backward dx = mask * dy / (1 - p) (dx may alias dy). */
VC_API int vc_dropout_fwd(long n, const float* x, const float* add, float* y, unsigned char* mask, float p,
                          unsigned long long seed, hipStream_t stream);
VC_API int vc_dropout_bwd(long n, const float* dy, const unsigned char* mask, float p, float* dx, hipStream_t stream);
/* The step seed in device memory, so that a replayed hipGraph of a training step draws fresh
 * keep masks.  state: 4 x unsigned long long {base, step, cur, 0} (8-byte aligned).  vc_seed_next is one launch of
 * one thread: step += 1, cur = splitmix64(base + step * 0x9E3779B97F4A7C15) >> 2 (wrapping 64-bit arithmetic;
 * cur < 2^62, the range of the host seeds); vitcnn_amd/seeds.py step_seed(base, step) restates it.
 * Every seed-taking forward has a _ds twin that reads its seed there: seed_dev points at `cur`, and the effective
 * seed is *seed_dev + site_offset (no wrap for site offsets < 2^62).  With *seed_dev == v a _ds call writes the
 * outputs and mask bytes of its host-seed entry called with seed v + site_offset, bit for bit (one kernel body: the
 * host-seed entry passes a null seed_dev).  The backward kernels read the saved mask bytes and have no twin. */
VC_API int vc_seed_next(unsigned long long* state, hipStream_t stream);
VC_API int vc_dropout_fwd_ds(long n, const float* x, const float* add, float* y, unsigned char* mask, float p,
                             const unsigned long long* seed_dev, unsigned long long site_offset, hipStream_t stream);

/* ---------------------------------------------------------------- FusAtNet forward (config 5)
 * model/compare_method/FusAtNet.py over channels-last [B,H,W,C] rows.
 * vc_im2col3x3_pad: col[(b,oh,ow), c*9+kh*3+kw] of a 3x3 conv with padding pad (0: ConvUnit_NP :19-27,
 *   1: ConvUnit / Residual units :9-17, :29-62); OH = H + 2 pad - 2; GEMM against weight [O, C*9].
 * vc_mul2_2d: out = a * b elementwise (Mt = spatial_am(x2) * Fhs, Fss = Fm * Am, :178-183).
 * vc_pool_scale: out[b,hw,c] = mean_p pooled[b,p,c] * F[b,hw,c] (AdaptiveAvgPool2d(1) of the spectral
 *   attention map times Fhs, :100-101, :178). */
VC_API int vc_im2col3x3_pad(int B, int H, int W, int C, int pad, const float* x, long ldx, float* col,
                            hipStream_t stream);
VC_API int vc_mul2_2d(long M, int C, const float* a, long lda, const float* b, long ldb, float* out, long ldo,
                      hipStream_t stream);
VC_API int vc_pool_scale(int B, int HW, int HWp, int C, const float* pooled, const float* F, long ldf, float* out,
                         long ldo, hipStream_t stream);
/* backward (out-of-place residual semantics): gradient of vc_im2col3x3_pad
 * (gather form; dx rows of ld lddx, overwritten or accumulated), and of vc_pool_scale
 * (dF += mean_p(pooled) * dout; dpooled[b,p,c] = sum_hw dout*F / HWp). */
VC_API int vc_col2im3x3_pad(int B, int H, int W, int C, int pad, const float* dcol, float* dx, long lddx,
                            int accumulate, hipStream_t stream);
VC_API int vc_pool_scale_bwd(int B, int HW, int HWp, int C, const float* pooled, const float* F, long ldf,
                             const float* dout, long lddo, float* dF, long lddf, float* dpooled, hipStream_t stream);

/* ---------------------------------------------------------------- MFT (comparison model)
 * model/compare_method/MFT.py.  All fp32 with fp32 accumulation; the feature width is 64 (FM * 4, FM = 16).
 *
 * vc_mft_conv3d_fwd / _wgrad: conv5's Conv3d(1, 8, (9,3,3), padding (0,1,1)) (MFT.py:137) over x [B, NC, P, P]
 *   (the batch layout; the band axis is the depth), D = NC - 8 output depths, 5 <= P <= 28:
 *     y[(b*P*P + h*P + w) * ldy + d*8 + c] = bias[c] + sum_{kd<9,kh<3,kw<3} w[c][kd][kh][kw] x[b][d+kd][h+kh-1][w+kw-1]
 *   i.e. channels-last rows of 8 D channels ordered d*8 + c (ldy >= 8 D, ldy % 4 == 0, y 16-B aligned): the rows
 *   viewed as [B*P*P*D, 8] are a plain 8-channel BatchNorm (BatchNorm3d(8)) and the 3x3 conv that follows reads
 *   them as they are.  wgrad: dw [8][81] (= [8,1,9,3,3]) = sum_{b,d,h,w} dy[..., d*8+c] x[b][d+kd][h+kh-1][w+kw-1],
 *   db[c] = sum dy[..., d*8+c], both overwritten; per-block partials in ws (vc_mft_conv3d_ws_floats), summed
 *   in a fixed order.  x is data: there is no input gradient.
 * vc_mft_hetconv_pack / _unpack: conv6's HetConv (MFT.py:15-25) gwc(x) + pwc(x), gwc = Conv2d(C, O, 3, groups g,
 *   padding 1), pwc = Conv2d(C, O, 1), as ONE dense 3x3 conv in vc_conv3x3_tap_*'s tap-major layout over the
 *   d*8 + c channel order above (C = 8 D; torch channel ch = c*D + d <-> column k = d*8 + c):
 *     wt[o][tap][k] = (ch / (C/g) == o / (O/g) ? gwc_w[o][ch % (C/g)][tap] : 0) + (tap == 4 ? pwc_w[o][ch] : 0),
 *     bias[o] = gwc_b[o] + pwc_b[o];
 *   unpack: dgwc_w[o][cl][tap] = dwt[o][tap][k(ch = (o/(O/g)) * (C/g) + cl)], dpwc_w[o][ch] = dwt[o][4][k(ch)]
 *   (entries off the group diagonal are ignored).  C % g == 0, O % g == 0.
 * vc_mft_tokpool_fwd / _bwd: the tokenisers (MFT.py:187-207) for X [B*HW, 64] rows (ldx), L <= 4 tokens, HW <= 1024:
 *     A[b,l,:] = softmax_i(sum_j wA[l][j] X[b,i,j]),  U[b,l,j] = sum_i A[b,l,i] X[b,i,j],
 *     T[b*strideT + l*ldt + k] = sum_j U[b,l,j] wV[j][k] (+ add[l][k], nullable: the position embedding rows)
 *   ((A X) wV, a reassociation of A (X wV)); A [B,L,HW] and U [B,L,64] are saved.  bwd from dT (same strides):
 *   dX (lddx, overwritten), dwA [L][64], dwV [64][64] (overwritten; per-sample partials in ws, >= B * (L*64 + 4096)
 *   floats, summed in a fixed order).
 * vc_mft_xattn_fwd / _bwd: MCrossAttention's core (MFT.py:42-56), 8 heads over 8-feature slices of Y [B, T, 64]
 *   (2 <= T <= 16), wq / wk / wv [64][8] applied to every slice: q[b,h,:] = wq Y[b,0,8h:8h+8],
 *   k / v[b,h,t,:] = wk / wv Y[b,t,8h:8h+8], a = softmax_t(scale q . k_t), O[b][h*64 + e] = sum_t a_t v[b,h,t,e];
 *   attn [B,8,T] saved.  bwd from dO [B, 512]: dY [B,T,64] (overwritten), dwq / dwk / dwv (overwritten; per-sample
 *   partials in ws, >= B * 1536 floats, summed over heads and batch in a fixed order: no atomics).
 * vc_mft_bcast_add_fwd / _bwd: Block's residual x + h with x [B,1,D] broadcast over h [B,T,D] (MFT.py:101):
 *   out[b,t,:] = h[b,t,:] + a[b,:];  da[b,:] = sum_t dout[b,t,:]. */
VC_API int vc_mft_conv3d_ws_floats(int B, int NC, int P);
VC_API int vc_mft_conv3d_fwd(int B, int NC, int P, const float* x, const float* w, const float* bias, float* y, long ldy,
                             hipStream_t stream);
VC_API int vc_mft_conv3d_wgrad(int B, int NC, int P, const float* x, const float* dy, long lddy, float* dw, float* db,
                               float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_mft_hetconv_pack(int O, int C, int g, const float* gwc_w, const float* pwc_w, const float* gwc_b,
                               const float* pwc_b, float* wt, float* bias, hipStream_t stream);
VC_API int vc_mft_hetconv_unpack(int O, int C, int g, const float* dwt, float* dgwc_w, float* dpwc_w,
                                 hipStream_t stream);
VC_API int vc_mft_tokpool_fwd(int B, int HW, int L, const float* X, long ldx, const float* wA, const float* wV,
                              const float* add, float* A, float* U, float* T, long ldt, long strideT,
                              hipStream_t stream);
VC_API int vc_mft_tokpool_bwd(int B, int HW, int L, const float* X, long ldx, const float* wA, const float* wV,
                              const float* A, const float* U, const float* dT, long ldt, long strideT, float* dX,
                              long lddx, float* dwA, float* dwV, float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_mft_xattn_fwd(int B, int T, const float* Y, const float* wq, const float* wk, const float* wv,
                            float scale, float* O, float* attn, hipStream_t stream);
VC_API int vc_mft_xattn_bwd(int B, int T, const float* Y, const float* wq, const float* wk, const float* wv,
                            const float* attn, const float* dO, float scale, float* dY, float* dwq, float* dwk,
                            float* dwv, float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_mft_bcast_add_fwd(int B, int T, int D, const float* h, const float* a, float* out, hipStream_t stream);
VC_API int vc_mft_bcast_add_bwd(int B, int T, int D, const float* dout, float* da, hipStream_t stream);
/* torch.optim.Adam step with coupled L2 weight decay (MFT's optimizer, model_utils.py:364-376) over a flat buffer:
 * g = grad_scale * grad + weight_decay * p before the moments, then Adam's update; hyper / step as vc_adamw */
VC_API int vc_adam(long n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const float* hyper,
                   float* step, hipStream_t stream);

/* ---------------------------------------------------------------- MDL-RS fusion CNNs (comparison models)
 * model/compare_method/DML_Hong.py (Early / Middle / Late / Cross_fusion_CNN) and losses.py:7-19.  All fp32.
 *
 * vc_maxpool2p_fwd / _bwd: nn.MaxPool2d(kernel_size=2, stride=2, padding=1) (DML_Hong.py:18) over a channels-last map
 *   x [B,H,W,C] (row stride ldx), H, W >= 2: y [B,OH,OW,C] (dense), OH = H/2 + 1, OW = W/2 + 1; output (oh, ow) covers
 *   rows 2 oh - 1, 2 oh and columns 2 ow - 1, 2 ow, taps outside the map are -inf padding; arg (uint8) = kh * 2 + kw of
 *   the first maximum among the in-range taps in (kh, kw) order, as torch.  bn_* (all or none, vc_conv3x3_fwd's
 *   convention): every tap is first mapped through relu((x - mean) * invstd * w + b) with vc_bn_apply's arithmetic,
 *   so BatchNorm apply, ReLU and pool are one pass over the conv output (y is bit-identical to vc_bn_apply with
 *   relu = 1 followed by the plain pool; pooling in front of the affine would be wrong for w < 0).
 *   bwd: dx[b,h,w,c] (ld lddx, overwritten, every element written once) = dy[b,(h+1)/2,(w+1)/2,c] where arg names
 *   that pixel, 0 elsewhere (the windows do not overlap: a gather); with y (the forward's output, nullable) the ReLU
 *   mask y > 0 is folded in, and dx is the gradient of the BatchNorm output: it feeds vc_bn_bwd_ex with no relu_out.
 * vc_avgpool_head_fwd / _bwd: nn.AdaptiveAvgPool2d(1) of G in {1, 2, 3} dense maps f_g [B,HW,C] (C <= 1024) followed
 *   by conv7, a 1x1 conv on a 1x1 map, as a product.  mode 0 (concat, Late_fusion_CNN's cat[x1, x2], :221):
 *   pooled [B, G C] with column g C + c, logits [B, ncls] = pooled W^T + bias, W [ncls, G C]; mode 1 (separate,
 *   Cross_fusion_CNN's three heads, :305-318): pooled [G, B, C], logits [G, B, ncls] = pooled W^T + bias with the one
 *   W [ncls, C].  pooled is kept for the backward.  bwd from dlogits (the logits' shape): dW, db (overwritten) summed
 *   over the batch and, in mode 1, over the G applications in a fixed order (no atomics: a second call gives the same
 *   bits); df_g [B,HW,C] (overwritten) = (dlogits W)[., column] / HW at every pixel.
 * vc_xfusion_loss_fwd_bwd: Cross_fusion_CNN_Loss for o1, o2, o3 [B, ncls]:
 *     loss = CE_weight(o1, target) + mean((o1 - o2)^2) + mean((o1 - o3)^2)   (means over all B ncls elements)
 *   and, for d(loss) = 1, do1 = dCE + 2 (o1 - o2) / n + 2 (o1 - o3) / n, do2 = -2 (o1 - o2) / n, do3 = -2 (o1 - o3) / n,
 *   n = B ncls, in ONE launch.  target int64 (-100 is ignored, nn.CrossEntropyLoss's default), weight may be null.
 *   The cross-entropy half is vc_ce_fwd_bwd's code: with o2 = o3 = o1 loss and do1 are its bits, do2 = do3 = 0. */
VC_API int vc_maxpool2p_fwd(int B, int H, int W, int C, const float* x, long ldx, const float* bn_mean,
                            const float* bn_invstd, const float* bn_w, const float* bn_b, float* y, unsigned char* arg,
                            hipStream_t stream);
VC_API int vc_maxpool2p_bwd(int B, int H, int W, int C, const float* dy, const unsigned char* arg, const float* y,
                            float* dx, long lddx, hipStream_t stream);
VC_API int vc_avgpool_head_fwd(int B, int HW, int C, int G, int ncls, int mode, const float* f0, const float* f1,
                               const float* f2, const float* W, const float* bias, float* pooled, float* logits,
                               hipStream_t stream);
VC_API int vc_avgpool_head_bwd(int B, int HW, int C, int G, int ncls, int mode, const float* dlogits, const float* W,
                               const float* pooled, float* df0, float* df1, float* df2, float* dW, float* db,
                               hipStream_t stream);
VC_API int vc_xfusion_loss_fwd_bwd(int B, int ncls, const float* o1, const float* o2, const float* o3,
                                   const long long* target, const float* weight, float* loss, float* do1, float* do2,
                                   float* do3, hipStream_t stream);

/* ---------------------------------------------------------------- per-pixel models (comparison models)
 * model/compare_method/EndNet.py, spectralformer.py and losses.py:21-35.  All fp32, no atomics, fixed summation order.
 *
 * vc_fc_fused_fwd: one fully-connected layer in ONE launch, y = act(norm(x W^T + b)) for rows x [B, K] (row stride
 *   ldx >= K, any alignment), W [N, K] dense, y [B, N] with row stride ldy >= N (two layers may write the two halves of
 *   one wider buffer: a concat for free).  1 <= K <= VC_FC_KMAX.  mode:
 *     VC_FC_PLAIN    y = z = x W^T + b
 *     VC_FC_SIGMOID  y = 1 / (1 + exp(-z))
 *     VC_FC_BN_RELU  y = relu(xhat gamma + beta), xhat = (z - mean) * rstd, nn.BatchNorm1d's conventions:
 *       train = 1: mean and the biased variance over the B rows (two passes, the second over z - mean), rstd =
 *         1 / sqrt(var + eps); run_mean = (1 - momentum) run_mean + momentum mean, run_var likewise with the unbiased
 *         var B / (B - 1).  A workgroup owns 8 columns and every row, which it keeps in LDS: 2 <= B <=
 *         VC_FC_TRAIN_BMAX, anything else is refused (return 1), never computed differently.
 *       train = 0: mean = run_mean, rstd = 1 / sqrt(run_var + eps); rows are independent, any B.
 *       xhat [B, N] dense (required in training, nullable in eval) and save_mean / save_rstd [N] (likewise) are what
 *       the backward reads.
 * vc_fc_fused_bwd: the same columns' backward in one launch, B <= VC_FC_TRAIN_BMAX, from dy [B, N] (row stride lddy):
 *     g = dy                         (VC_FC_PLAIN)
 *     g = dy y (1 - y)               (VC_FC_SIGMOID, y the forward's output, row stride ldy)
 *     g = dy [y > 0]                 (VC_FC_BN_RELU); dbeta = sum_b g, dgamma = sum_b g xhat, and
 *       dz = gamma rstd (g - dbeta / B - xhat dgamma / B) in training, dz = gamma rstd g in eval;
 *   dz = g in the other modes.  dW[n, :] = sum_b dz[b, n] x[b, :], db[n] = sum_b dz[b, n] (overwritten); dz (nullable,
 *   row stride lddz) is written for the caller's data-gradient GEMM dz W.
 * vc_endnet_loss_fwd_bwd: EndNet_Loss for out [B, ncls], de1 / x1 [B, C1], de2 / x2 [B, C2] (dense):
 *     loss = CE_weight(out, target) + mean((de1 - x1)^2) + mean((de2 - x2)^2)    (means over B C1 and B C2 elements)
 *   and, for d(loss) = 1, dout = dCE, dde1 = 2 (de1 - x1) / (B C1), dde2 = 2 (de2 - x2) / (B C2), in ONE launch.
 *   target int64 (-100 is ignored), weight may be null.  The cross-entropy half is vc_ce_fwd_bwd's code: with
 *   de = x loss and dout are its bits.
 * vc_sf_embed_fwd: SpectralFormer's token rows X [B, T, D], T = C1 + C2 + 1, from x1 [B, C1] and x2 [B, C2] (C1 >= 1;
 *   C2 = 0 with x2 null is a single modality):
 *     X[b, 0, :] = cls + pos[0];  X[b, 1 + n, :] = x[b, n] w + bias + pos[1 + n],  x = cat(x1, x2) along the bands
 *   (Linear(1, D): w, bias [D]); pos [T, D].  With p > 0 the embedding dropout is applied to X with vc_dropout_fwd's
 *   hash over the element index (the same seed gives the same keep mask) and the mask [B T D] bytes is written.
 * vc_sf_embed_bwd: from dX [B, T, D] (with p > 0 first masked and scaled by 1 / (1 - p)):
 *     dpos[t, d] = sum_b dX[b, t, d], dcls[d] = dpos[0, d], dw[d] = sum_{b, n} x[b, n] dX[b, 1 + n, d],
 *     db[d] = sum_{b, n} dX[b, 1 + n, d]   (overwritten; per-(t, d) partials in ws >= T D floats, then a finishing
 *   pass over t: two launches, fixed order). */
#define VC_FC_PLAIN 0
#define VC_FC_BN_RELU 1
#define VC_FC_SIGMOID 2
#define VC_FC_TRAIN_BMAX 1024
#define VC_FC_KMAX 512
VC_API int vc_fc_fused_fwd(int mode, int train, int B, int K, int N, const float* x, long ldx, const float* W,
                           const float* bias, const float* gamma, const float* beta, float* run_mean, float* run_var,
                           float eps, float momentum, float* y, long ldy, float* xhat, float* save_mean,
                           float* save_rstd, hipStream_t stream);
VC_API int vc_fc_fused_bwd(int mode, int train, int B, int K, int N, const float* dy, long lddy, const float* y,
                           long ldy, const float* xhat, const float* x, long ldx, const float* gamma,
                           const float* rstd, float* dz, long lddz, float* dW, float* db, float* dgamma, float* dbeta,
                           hipStream_t stream);
VC_API int vc_endnet_loss_fwd_bwd(int B, int ncls, int C1, int C2, const float* out, const long long* target,
                                  const float* weight, const float* de1, const float* x1, const float* de2,
                                  const float* x2, float* loss, float* dout, float* dde1, float* dde2,
                                  hipStream_t stream);
VC_API int vc_sf_embed_fwd(int B, int C1, int C2, int D, const float* x1, const float* x2, const float* w,
                           const float* bias, const float* cls, const float* pos, float p, unsigned long long seed,
                           float* X, unsigned char* mask, hipStream_t stream);
/* vc_sf_embed_fwd with the seed *seed_dev + site_offset read on the device (see vc_seed_next) */
VC_API int vc_sf_embed_fwd_ds(int B, int C1, int C2, int D, const float* x1, const float* x2, const float* w,
                              const float* bias, const float* cls, const float* pos, float p,
                              const unsigned long long* seed_dev, unsigned long long site_offset, float* X,
                              unsigned char* mask, hipStream_t stream);
VC_API int vc_sf_embed_bwd(int B, int C1, int C2, int D, const float* x1, const float* x2, const float* dX,
                           const unsigned char* mask, float p, float* dw, float* db, float* dpos, float* dcls, float* ws,
                           long ws_floats, hipStream_t stream);

/* ---------------------------------------------------------------- HCTnet (comparison model)
 * model/compare_method/HCTnet.py.  All fp32 with fp32 accumulation, feature width 64, no atomics: every weight gradient
 * is a per-sample partial row in ws summed in a fixed order, so a second call gives the same bits.  Dropout uses
 * vc_dropout_fwd's hash over the element index of the call's whole mask buffer (keep = hash(seed, i) / 2^24 >= p, kept
 * values scaled by 1 / (1 - p)); every keep decision is written out as a byte.  With every p of a call 0 the mask may be
 * null; where it is given, p = 0 sites write 1.
 *
 * vc_hct_tokpool_fwd / _bwd: the tokeniser (HCTnet.py:326-353) for X [B*HW, 64] rows (ldx), 1 <= L <= 8 tokens,
 *   1 <= HW <= 784, into a dense token buffer T [B, L+1, 64]:
 *     A[b,l,:] = softmax_i(sum_j wA[l][j] X[b,i,j]),  U[b,l,j] = sum_i A[b,l,i] X[b,i,j],
 *     T[b,0,:] = drop(cls + pos[0]),  T[b,1+l,k] = drop(sum_j U[b,l,j] wV[j][k] + pos[1+l][k])
 *   ((A X) wV, a reassociation of A (X wV)); A [B,L,HW] and U [B,L,64] are saved, mask [B, L+1, 64] bytes.
 *   bwd from dT [B, L+1, 64] (first masked and scaled): dX (lddx, overwritten) and one partial row per sample,
 *   [L*64 dwA | 4096 dwV | (L+1)*64 dpos], at rows row0 .. row0 + B - 1 of ws (>= (row0 + B) * (L*64 + 4096 + (L+1)*64)
 *   floats).  With dwA / dwV / dpos / dcls given (all or none) rows 0 .. row0 + B - 1 are then summed into them
 *   (overwritten; dcls = dpos[0]): the model's two sources share the parameters, so the HSI call passes row0 = 0 and
 *   no outputs, the LiDAR call row0 = B and the outputs, and both sources' partials are reduced together.
 * vc_hct_encoder_fwd / _bwd: one pre-norm Transformer layer (HCTnet.py:205-219: Attention :56-94, MLP_Block :42-54)
 *   of both branches' sequences X [2][B, T, 64] (branch stride strideX floats), 2 <= T <= 9, in ONE launch; a block
 *   owns one sample of one branch.  W0 / W1: the branch's VC_HCT_ENC_FLOATS packed parameters in module order
 *   [ln1.w 64 | ln1.b 64 | to_qkv.w 192x64 | to_qkv.b 192 | nn1.w 64x64 | nn1.b 64 | ln2.w 64 | ln2.b 64 | fc1.w 8x64 |
 *   fc1.b 8 | fc2.w 64x8 | fc2.b 64] (16-B aligned):
 *     n = LN(x) (eps 1e-5); q | k | v = n Wqkv^T + b split into 8 heads of width 8; a = softmax_j(0.125 q_i . k_j)
 *     (the scale is 64^-0.5, the model width); o = a v; x2 = x + drop_a(o Wnn1^T + b);
 *     y = x2 + drop_o(drop_h(gelu(LN(x2) Wfc1^T + b)) Wfc2^T + b)      (erf GELU)
 *   pa / ph / po: the three sites' p per branch; mask [2][B][T*64 | T*8 | T*64] bytes.
 *   bwd from dY (strideDY): dX (strideDX, overwritten) and dW0 / dW1 in the packed layout (overwritten); the forward's
 *   intermediates are recomputed from X with the forward's code and the saved masks.  ws >= 2 B VC_HCT_ENC_FLOATS.
 * vc_hct_ctattn_fwd / _bwd: the cross-token step (CT_Transformer :152-171, CTAttention :96-131) of both directions in
 *   ONE launch from the encoder output X [2][B, T, 64]: direction d's query is branch d's row 0, its context
 *   c = [LN(x[d][b][0]); x[1-d][b][1..T-1]] (T rows, only row 0 normed).  W0 / W1: VC_HCT_CT_FLOATS packed parameters
 *   [ln.w 64 | ln.b 64 | to_q.w 512x64 | to_kv.w 1024x64 | to_out.w 64x512 | to_out.b 64] (16-B aligned):
 *     q = Wq c_0; per head h (8 heads of width 64): a[h] = softmax_j(0.125 q_h . (Wk_h c_j)), ad = drop_p(a),
 *     o_h = sum_j ad[h][j] Wv_h c_j;  out[d][b] = x[d][b][0] + drop_o(Wo o + bo)
 *   evaluated as r_h = Wk_h^T q_h, score = r_h . c_j and o_h = Wv_h (sum_j ad[h][j] c_j): each weight is read once per
 *   sample.  out [2][B, 64]; mask [2][B][8*T | 64] bytes.  bwd from dout [2][B,64]: dX [2][B,T,64] (strideDX,
 *   overwritten: row 0 of branch d and rows 1.. of branch 1-d by direction d) and dW0 / dW1 packed (overwritten).
 *   ws >= 2 B VC_HCT_CT_FLOATS. */
#define VC_HCT_ENC_FLOATS 17992
#define VC_HCT_CT_FLOATS 131264
VC_API int vc_hct_tokpool_fwd(int B, int HW, int L, const float* X, long ldx, const float* wA, const float* wV,
                              const float* cls, const float* pos, float p, unsigned long long seed, float* A, float* U,
                              float* T, unsigned char* mask, hipStream_t stream);
VC_API int vc_hct_tokpool_bwd(int B, int HW, int L, const float* X, long ldx, const float* wA, const float* wV,
                              const float* A, const float* U, const float* dT, const unsigned char* mask, float p,
                              float* dX, long lddx, float* ws, long ws_floats, int row0, float* dwA, float* dwV,
                              float* dpos, float* dcls, hipStream_t stream);
VC_API int vc_hct_encoder_fwd(int B, int T, const float* X, long strideX, const float* W0, const float* W1, float pa0,
                              float ph0, float po0, float pa1, float ph1, float po1, unsigned long long seed, float* Y,
                              long strideY, unsigned char* mask, hipStream_t stream);
VC_API int vc_hct_encoder_bwd(int B, int T, const float* X, long strideX, const float* W0, const float* W1, float pa0,
                              float ph0, float po0, float pa1, float ph1, float po1, const unsigned char* mask,
                              const float* dY, long strideDY, float* dX, long strideDX, float* dW0, float* dW1,
                              float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_hct_ctattn_fwd(int B, int T, const float* X, long strideX, const float* W0, const float* W1, float pp0,
                             float po0, float pp1, float po1, unsigned long long seed, float* out, unsigned char* mask,
                             hipStream_t stream);
VC_API int vc_hct_ctattn_bwd(int B, int T, const float* X, long strideX, const float* W0, const float* W1, float pp0,
                             float po0, float pp1, float po1, const unsigned char* mask, const float* dout, float* dX,
                             long strideDX, float* dW0, float* dW1, float* ws, long ws_floats, hipStream_t stream);
/* the three forwards with the seed *seed_dev + site_offset read on the device (see vc_seed_next); everything else as
 * the host-seed entries above */
VC_API int vc_hct_tokpool_fwd_ds(int B, int HW, int L, const float* X, long ldx, const float* wA, const float* wV,
                                 const float* cls, const float* pos, float p, const unsigned long long* seed_dev,
                                 unsigned long long site_offset, float* A, float* U, float* T, unsigned char* mask,
                                 hipStream_t stream);
VC_API int vc_hct_encoder_fwd_ds(int B, int T, const float* X, long strideX, const float* W0, const float* W1,
                                 float pa0, float ph0, float po0, float pa1, float ph1, float po1,
                                 const unsigned long long* seed_dev, unsigned long long site_offset, float* Y,
                                 long strideY, unsigned char* mask, hipStream_t stream);
VC_API int vc_hct_ctattn_fwd_ds(int B, int T, const float* X, long strideX, const float* W0, const float* W1,
                                float pp0, float po0, float pp1, float po1, const unsigned long long* seed_dev,
                                unsigned long long site_offset, float* out, unsigned char* mask, hipStream_t stream);

/* ---------------------------------------------------------------- principal components (csrc/pca.hip)
 * The whitened PCA of the HSI cube's pixel spectra (utils.py:85-93 applyPCA, scikit-learn on the host in the reference)
 * as three device ops; the C x C eigendecomposition between them stays on the host (vitcnn_amd/pca.py).  Operands are
 * the rows of an [n, C] fp32 matrix x with leading dimension ld >= C: the [W, H, C] cube with n = W * H, ld = C.
 * Limits: 2 <= n < 2^31 - 64, 1 <= C <= 512, 1 <= K <= min(C, 64), ld >= C, ldy >= K; anything else returns 1 before any
 * launch.  No floating-point atomics: a second call gives the same bits.  Columns ld > C, an unaligned base and
 * C % 4 != 0 are all accepted; nothing outside the logical operands is read into a result.
 *
 * vc_pca_slab_rows: R, the rows of x one block of vc_pca_cov accumulates in fp32 (returned, not a status).
 * vc_pca_cov_workspace: *bytes the caller provides as `workspace` (16-B aligned) to vc_pca_mean and vc_pca_cov at this
 *   n and C (the larger of the two needs: at most 1024 fp64 rows of C, and ceil(n / R) * T (T + 1) / 2 fp32 tiles of
 *   64 x 64 with T = ceil(C / 64)).
 * vc_pca_mean: mean[c] = sum_i x[i][c] / n in fp64 -- per-slab partial rows in the workspace (each lane's rows in
 *   ascending order), then the slabs summed in a fixed order.
 * vc_pca_cov: cov[C][C] (dense, fp64) = sum_i xc_i xc_i^T / (n - 1), xc_i = x[i] - mean32 formed in registers as the
 *   panels are staged (rows past n and columns past C stay exactly zero).  Grid: upper-triangle pairs of 64-column
 *   tiles x slabs of R rows; inner product on v_mfma_f32_16x16x4_f32 (two fma chains of R / 2 per element); one fp32
 *   tile partial per (slab, pair); a second launch sums the slabs in a fixed order in fp64, divides and mirrors, so cov
 *   is exactly symmetric.
 * vc_pca_project: y[i][k] = sum_c (x[i][c] - mean32[c]) wt[c][k], wt [C][K] dense (the whitening folded in by the
 *   caller), on v_mfma_f32_16x16x4_f32 (one fma chain of C per output), one pass over x with wt held in LDS (128 KB at
 *   C = 512, K > 32). */
VC_API int vc_pca_slab_rows(void);
VC_API int vc_pca_cov_workspace(long n, int C, long* bytes);
VC_API int vc_pca_mean(long n, int C, long ld, const float* x, void* workspace, double* mean, hipStream_t stream);
VC_API int vc_pca_cov(long n, int C, long ld, const float* x, const float* mean32, void* workspace, double* cov,
                      hipStream_t stream);
VC_API int vc_pca_project(long n, int C, long ld, int K, const float* x, const float* mean32, const float* wt,
                          float* y, long ldy, hipStream_t stream);

/* ---------------------------------------------------------------- MHST (csrc/mhst.hip)
 * model/compare_method/MHST/ (MHST.py, HSPT.py, Pooling.py, PyConv2D.py).  fp32, no floating-point atomics, every sum
 * in a fixed order: a second call gives the same bits.  Invalid arguments return 1 before any launch.
 *
 * vc_mhst_conv_fwd / _dgrad / _wgrad: a grouped 3-D convolution over channels-last rows, spectral stride sd and
 *   padding pd, square spatial kernel KS (odd, 1..9) with 'same' padding KS / 2 and stride 1:
 *     x rows (b, d, h, w) of C channels (ldx), w [O][C/G][KD][KS][KS] dense, y rows (b, e, h, w) of O columns (ldy;
 *     a caller writing one part of a concatenation offsets y and passes the whole row's ldy), Dout = (D + 2 pd - KD) / sd
 *     + 1 (passed, checked):
 *     y[b,e,h,w,o] = bias[o] + sum_{kd,kh,kw,c < C/G} w[o][c][kd][kh][kw] x[b, e sd - pd + kd, h - KS/2 + kh,
 *                    w - KS/2 + kw, (o / (O/G)) (C/G) + c]           (taps outside the map contribute nothing)
 *   This one family is the model's Conv3d (11,3,3) stride (3,1,1), its four spectral convs (KS 1, each into its 4
 *   columns of the 16), the 3x3x3 conv, and every PyConv2D branch: a 2-D conv is D = KD = Dout = 1, and the grouped 2-D
 *   conv over the `(c d)` reshape of the 3-D stage is KD = D, pd = 0, Dout = 1 on the 3-D rows as they are (its weight
 *   [O][(C/G) D][k][k] IS [O][C/G][D][k][k], and a group of (c d) channels is a group of c since 16 / G is whole).
 *   dgrad: dx = beta dx + the transposed sum (lddx); wgrad: dw (overwritten) and db (may be null) = column sums of dy,
 *   H W <= 64 and O / G <= 16 there: one block of 8 waves per (group, input channel, tap), a lane per spatial position,
 *   the waves splitting the (sample, depth) pairs; per output the wave's xor tree, then the waves in order.
 * vc_mhst_embed_fwd / _bwd: fusion and token embedding (MHST.py:287-301) from the two pooled maps ph, pl [B,16,64]
 *   (rows = the 4x4 positions, 64 channels):
 *     f = wh ph + wl pl;  xcnn[b,j,c] = sum_p W[j][p] f[b,p,c] + bias[j];
 *     X0[b,0,:] = cls + pos[0];  X0[b,1+j,:] = xcnn[b,j,:] + pos[1+j] + pos[0]     (wh, wl: device scalars)
 *   bwd from dX0 [B,65,64] and dxcnn [B,64,64] (the CNN classifier's path): dph, dpl and one partial row per sample
 *   part[b] = [dW 64x16 | dbias 64 | dpos0 64 | dwh, dwl, 0, 0] (VC_MHST_EMBED_PART floats); the caller sums them.
 * vc_mhst_gate_fwd / _bwd: the head gate (HSPT.py:7-63) on the cls rows x[b] = X + b ldx:
 *     logits = Wg x + bg [B,16];  train: v = (logits + n) / tau with n = noise_in where given, else Logistic(0,1) noise
 *     log(u / (1 - u)), u = ((hash(seed, b 16 + h) >> 9) + 0.5) / 2^23 (g1 - g2 of two Gumbel draws is logistic);
 *     eval: v = logits.  y = sigmoid(v), sel = v > 0.  noise_out (may be null) receives n.
 *   bwd (straight-through): dlogits = dsel y (1 - y) scale  (scale = 1 / tau in training, 1 in eval).
 * vc_mhst_headmask_fwd / _bwd: Y[b,t,c] = X[b,t,c] sel[b][(c % 64) / 4] over rows of Wd = 64 or 192 columns (DynaLinear's
 *   output rows of query | key | value, or the input columns of proj / fc1); bwd: dX = dY sel and
 *   dsel[b,h] = beta dsel[b,h] + sum_{t, c of head h} dY X  (per column over t ascending, then the head's columns).
 * vc_mhst_pool_fwd / _bwd: attn_pool (Pooling.py) of q | k | v, X [B,65,192]: per tensor s and head h the depthwise 3x3
 *   conv (pad 1, its 4 channels shared by the 16 heads) over rows 1..64 as an 8x8 grid, row 0 passed, then LayerNorm(4)
 *   of every row of every head.  pw = [conv 4x9 | ln.w 4 | ln.b 4] x 3 (VC_MHST_POOL_FLOATS).  A switched-off head is
 *   computed like any other: its rows come out as ln.b.  bwd: dX and part[b] = the 132 parameter gradients.
 * vc_mhst_attn_fwd / _bwd: per sample and head (16 heads of width 4) over QKV [B,65,192] (pooled q | k | v):
 *     a = softmax_j(scale q_i . k_j);  ad = a keep / (1 - p);  o_i = sum_j ad_ij v_j (+ q_i for i >= 1)
 *   keep = vc_dropout_fwd's hash over the index of mask [B,16,65,65] (bytes, written; may be null at p = 0).  bwd
 *   recomputes a from QKV, one block per (sample, head) holding the head's 65 x 65 dS and ad in LDS.
 * vc_mhst_tail_fwd / _bwd: the dual-softmax tail (MHST.py:308-319): avg[b,k] = mean_t z[b,t,k] over z [B,64,32] (ldz),
 *     p1 = softmax(lg1[b]), p2 = softmax(W2 avg + b2), out = cv p1 + cc p2   (cv, cc device scalars; ncls <= 256)
 *   bwd: dlg1, dz (lddz) and part[b] = [dW2 ncls x 32 | db2 ncls | dcv, dcc] (ncls * 33 + 2 floats).
 *
 * vc_mhst_conv3_fwd / _dgrad / _wgrad: the model's 3x3x3 convolution (16 -> 16 channels, stride 1, padding 1, 8 x 8
 *   planes; vc_mhst_conv_*'s formulas at C = O = 16, G = 1, KD = KS = 3) as an implicit GEMM on v_mfma_f32_16x16x4_f32:
 *   K = 27 taps x 16 channels walked tap-major, N = 16, M = B D 64.  fwd and dgrad (dx = beta dx + ...): one block per
 *   (sample, depth) plane, the weight in LDS; the operand read as float4 runs (x / dy 16-B aligned, ldx / lddy a multiple
 *   of 4).  wgrad: min(VC_MHST_CONV3_WAVES, B D) waves each walk their planes in order with 27 accumulators (the rows are
 *   the MFMA's k) and leave a partial [16][16][27] in ws (vc_mhst_conv3_wgrad_ws_floats floats), then summed in wave
 *   order: a fixed order.  The bias gradient is vc_colsum of dy.
 *
 * vc_mhst_hsattn_fwd / _fwd_ds / _bwd: the chain gate -> head mask -> pooling -> attention -> head mask of a head-select
 *   block FUSED, one block per (sample, head) (each step is independent per head): from the block input's cls rows
 *   (X, ldx) and the raw q | k | v GEMM output QKV [B,65,192],
 *     sel, y, noise, logits as vc_mhst_gate_fwd's (noise index b 16 + h; the dot product summed by a wave's xor tree);
 *     qm = QKV sel (the head's 12 columns);  qp = vc_mhst_pool_fwd(qm);  ao = vc_mhst_attn_fwd(qp) with the same keep
 *     hash and mask bytes [B,16,65,65];  AM [B,65,64] = ao sel
 *   with the head's masked and pooled rows in LDS: only AM (and the gate's 4 x [B,16] values, the mask bytes) is written.
 *   seed_gate / seed_prob: the two sites' seeds (_ds: offsets to *seed_dev).  bwd from dAM: the chain is recomputed from
 *   QKV, the head's 65 x 65 dS and dropped probabilities sit in LDS; dQKV [B,65,192] (gradient of the raw q | k | v),
 *   part[(b 16 + h)] = the head's share of the 132 pooling parameter gradients (VC_MHST_POOL_FLOATS per row, B 16 rows;
 *   the caller sums them in row order), and
 *     dlogits[b,h] = (dsel_in[b,h] + sum dAM ao + sum dqm QKV) y (1 - y) gscale     (dsel_in: the MLP mask's share, may
 *   be null; gscale = 1 / tau in training, 1 in eval; the sums in a fixed order).
 *
 * vc_mhst_pconv_ok / _ws_floats / _fwd / _dgrad / _wgrad (csrc/mhst_pconv.hip): the grouped "whole-depth" convolutions
 *   of the pyramidal stages on 8 x 8 maps as implicit GEMMs on v_mfma_f32_16x16x4_f32, exact fp32 (an MFMA is a k-ordered
 *   fmaf chain).  Exactly vc_mhst_conv_fwd / _dgrad / _wgrad at H = W = 8, KD = D, sd = 1, pd = 0, Dout = 1:
 *     y[b,h,w,o] = bias[o] + sum_{d,kh,kw,c < C/G} w[o][c][d][kh][kw] x[b, d, h - KS/2 + kh, w - KS/2 + kw,
 *                  (o / (O/G)) (C/G) + c]
 *   with the same operands: x rows (b, d, h, w) of C channels (ldx), w [O][C/G][D][KS][KS] dense, y rows (b, h, w) of O
 *   columns written at the caller's column offset inside rows of ldy; dgrad: dx = beta dx + the transposed sum; wgrad:
 *   dw (overwritten) and db (may be null) = the column sums of dy.
 *   vc_mhst_pconv_ok(D, C, O, G, KS, ldx, ldy) is 1 where the family takes the shape (host arithmetic only): KS odd in
 *   3..9, C a multiple of 16, G dividing C and O, C / G a power of two in 2..32, O / G a power of two in 2..16,
 *   1 <= D <= 4096, ldx >= C, ldy >= O (the model's hsi_encoder.conv4, lidar_encoder.conv2 and pyconv_classifier.conv1;
 *   lidar_encoder.conv1 with its 1 to 3 input channels stays on vc_mhst_conv_*).  Alignment contract: ldx and ldy are multiples of 4 floats and the x-side pointer (x, dx), the y-side
 *   pointer as passed (y, dy: base + column offset, so an offset that is a multiple of 4 floats; the model's are
 *   multiples of 16) and ws are 16-byte aligned; w, bias, dw, db need only their natural alignment.
 *   Per group each direction is a skinny GEMM whose N is padded to 16 with zero weights:
 *     fwd    M = (b, position), N = O/G, K = (tap, depth, channel); a block per (2 samples, group, chunk of
 *            VC_MHST_PCONV_CHUNK depths; half that at C/G = 32), the chunk's planes in LDS; more than one chunk: partials
 *            [chunk][b 64][O] in ws, summed in chunk order
 *     dgrad  M = (b, position), N = (depth, channel) in tiles of 16, K = (tap, output)
 *     wgrad  M = O/G, N = (depth, channel) in tiles of 16, K = (b, position) per tap; a block per (group, tile, kernel
 *            row, sample split), its 4 waves summed in wave order, the splits' partials in ws summed in split order
 *   fwd and dgrad first re-lay the weight [k][16] into ws (a pack launch per call; dgrad instead keeps a
 *   group's weight of up to 8192 floats in LDS as it lies).  ws: vc_mhst_pconv_ws_floats(B, ...)
 *   floats, the max over the three directions (-1 on a shape _ok refuses).  Only a group's own columns are read; a tap
 *   outside the map feeds 0 without a read, so row padding and neighbouring columns may hold anything.  Invalid
 *   arguments, a shape _ok refuses and a workspace that is too small return 1 before any launch.
 *
 * vc_mhst_conv1_ws_floats / _fwd / _wgrad and vc_mhst_sconv_ws_floats / _fwd / _dgrad / _wgrad (csrc/mhst_sconv.hip): the
 *   front of the HSI encoder as implicit GEMMs on v_mfma_f32_16x16x4_f32, exact fp32, no atomics, every partial summed
 *   in a fixed order.
 *   conv1: the strided first convolution, exactly vc_mhst_conv_fwd / _wgrad at H = W = 8, C = 1, O = 16, G = 1, KD = 11,
 *   KS = 3, sd = 3, pd = 5, Dout = D1 = (l1 + 2) / 3, any l1 >= 1:
 *     y[b,e,h,w,o] = bias[o] + sum_{kd<11,kh<3,kw<3} w[o][kd][kh][kw] x[b, 3e - 5 + kd, h - 1 + kh, w - 1 + kw]
 *   x the dense patch [B, l1, 8, 8], w [16][1][11][3][3] dense, y rows (b, e, h, w) of 16 columns in rows of ldy.  fwd:
 *   M = (b, e, position), N = 16, K = (kh, kw, kd padded to 12) in 27 MFMA steps; a block per (sample,
 *   VC_MHST_CONV1_CHUNK output depths) with their 3 (chunk - 1) + 11 input planes zero-padded in LDS, so no tap reads
 *   global memory outside the cube.  wgrad: M = 16 outputs, N = 99 taps in 7 tiles, K = (b, e, position);
 *   min(VC_MHST_CONV1_WAVES, B D1) waves each walk their (sample, depth) planes in order, a plane's 11 input planes
 *   staged in LDS once, and leave a partial [dw 16 x 99 | db 16] in ws (the bias gradient is the tile's column of
 *   ones), then summed in wave order.  db = the column sums of dy, may be null.  There is no data gradient: the input
 *   is the patch.
 *   sconv: the four spectral convolutions (16 -> 4 channels each, (k,1,1) kernels, k = 1, 3, 5, 11, padding k / 2, each
 *   writing its 4 columns of the 16) as ONE convolution; with r_i = 0, 1, 2, 5:
 *     y[(b,e,p), 4i + j] = bias_i[j] + sum_{t=-r_i..r_i} sum_{c<16} w_i[j][c][t + r_i] x[(b, e + t, p), c]
 *   (depths outside [0, D) contribute nothing); x rows (b, d, p) of 16 channels (ldx), w_i [4][16][k_i] dense, y rows of
 *   16 columns (ldy).  fwd: M = (b, e, position), N = 16, K = 11 depth offsets x 16 channels over the weight laid
 *   [t][c][16] in LDS with structural zeros where |t| > r_i (issued 11 x 16 x 16 multiply-adds per row against the
 *   nominal 20 x 16 x 4); a block per (sample, VC_MHST_SCONV_CHUNK depths), their chunk + 10 source planes in LDS.
 *   dgrad: dx = beta dx + the sum of the four transposed convolutions, the same kernel with the operand roles swapped
 *   and the offsets mirrored.  wgrad: M = 16 columns, N = 16 channels, one accumulator per depth offset, K = the rows;
 *   min(VC_MHST_SCONV_BLOCKS, B ceil(D / chunk)) blocks walk their (sample, chunk) items in order, a block's 4 waves
 *   are summed in wave order, the blocks' partials in ws in block order, and only the real (i, j, c, tap) entries are
 *   written to the four dw_i; db_i [4] = the column sums of dy, all four given or all four null (as the biases of fwd).
 *   Because of the zero padding a non-finite activation at depth e + t reaches the columns of a convolution whose own
 *   kernel does not extend to t (0 * inf is NaN); with finite activations the result is the sum of the real taps only.
 *   Alignment contract: ldx, ldy, lddy, lddx >= 16 and multiples of 4 floats; the x-side pointers (x, dx), the y-side
 *   pointers (y, dy) and ws 16-byte aligned; weights and biases need their natural alignment.  ws:
 *   vc_mhst_conv1_ws_floats(B, l1) / vc_mhst_sconv_ws_floats(B, D) floats, the max over the family's directions
 *   (negative on bad arguments).  B < 1, l1 < 1, D < 1, a bad leading dimension, a null required operand, a misaligned
 *   pointer, biases partly null and a workspace that is too small return 1 before any launch. */
#define VC_MHST_CONV1_CHUNK 4
#define VC_MHST_CONV1_WAVES 1024
#define VC_MHST_SCONV_CHUNK 4
#define VC_MHST_SCONV_BLOCKS 256
#define VC_MHST_PCONV_CHUNK 4
#define VC_MHST_CONV3_WAVES 512
#define VC_MHST_EMBED_PART 1156
#define VC_MHST_POOL_FLOATS 132
VC_API int vc_mhst_conv_fwd(int B, int D, int H, int W, int C, int O, int G, int KD, int KS, int sd, int pd, int Dout,
                            const float* x, long ldx, const float* w, const float* bias, float* y, long ldy,
                            hipStream_t stream);
VC_API int vc_mhst_conv_dgrad(int B, int D, int H, int W, int C, int O, int G, int KD, int KS, int sd, int pd, int Dout,
                              const float* dy, long lddy, const float* w, float* dx, long lddx, float beta,
                              hipStream_t stream);
VC_API int vc_mhst_conv_wgrad(int B, int D, int H, int W, int C, int O, int G, int KD, int KS, int sd, int pd, int Dout,
                              const float* x, long ldx, const float* dy, long lddy, float* dw, float* db,
                              hipStream_t stream);
VC_API int vc_mhst_conv3_fwd(int B, int D, const float* x, long ldx, const float* w, const float* bias, float* y,
                             long ldy, hipStream_t stream);
VC_API int vc_mhst_conv3_dgrad(int B, int D, const float* dy, long lddy, const float* w, float* dx, long lddx,
                               float beta, hipStream_t stream);
VC_API int vc_mhst_conv3_wgrad_ws_floats(int B, int D);
VC_API int vc_mhst_conv3_wgrad(int B, int D, const float* x, long ldx, const float* dy, long lddy, float* dw, float* ws,
                               long ws_floats, hipStream_t stream);
VC_API int vc_mhst_pconv_ok(int D, int C, int O, int G, int KS, long ldx, long ldy);
VC_API int vc_mhst_pconv_ws_floats(int B, int D, int C, int O, int G, int KS);
VC_API int vc_mhst_pconv_fwd(int B, int D, int C, int O, int G, int KS, const float* x, long ldx, const float* w,
                             const float* bias, float* y, long ldy, float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_mhst_pconv_dgrad(int B, int D, int C, int O, int G, int KS, const float* dy, long lddy, const float* w,
                               float* dx, long lddx, float beta, float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_mhst_pconv_wgrad(int B, int D, int C, int O, int G, int KS, const float* x, long ldx, const float* dy,
                               long lddy, float* dw, float* db, float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_mhst_conv1_ws_floats(int B, int l1);
VC_API int vc_mhst_conv1_fwd(int B, int l1, const float* x, const float* w, const float* bias, float* y, long ldy,
                             float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_mhst_conv1_wgrad(int B, int l1, const float* x, const float* dy, long lddy, float* dw, float* db,
                               float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_mhst_sconv_ws_floats(int B, int D);
VC_API int vc_mhst_sconv_fwd(int B, int D, const float* x, long ldx, const float* w1, const float* w2, const float* w3,
                             const float* w4, const float* b1, const float* b2, const float* b3, const float* b4,
                             float* y, long ldy, float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_mhst_sconv_dgrad(int B, int D, const float* dy, long lddy, const float* w1, const float* w2,
                               const float* w3, const float* w4, float* dx, long lddx, float beta, float* ws,
                               long ws_floats, hipStream_t stream);
VC_API int vc_mhst_sconv_wgrad(int B, int D, const float* x, long ldx, const float* dy, long lddy, float* dw1,
                               float* dw2, float* dw3, float* dw4, float* db1, float* db2, float* db3, float* db4,
                               float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_mhst_embed_fwd(int B, const float* ph, const float* pl, const float* wh, const float* wl, const float* W,
                             const float* bias, const float* pos, const float* cls, float* xcnn, float* X0,
                             hipStream_t stream);
VC_API int vc_mhst_embed_bwd(int B, const float* ph, const float* pl, const float* wh, const float* wl, const float* W,
                             const float* dX0, const float* dxcnn, float* dph, float* dpl, float* part,
                             hipStream_t stream);
VC_API int vc_mhst_gate_fwd(int B, const float* X, long ldx, const float* Wg, const float* bg, const float* noise_in,
                            int train, float tau, unsigned long long seed, float* logits, float* noise_out, float* y,
                            float* sel, hipStream_t stream);
VC_API int vc_mhst_gate_fwd_ds(int B, const float* X, long ldx, const float* Wg, const float* bg, const float* noise_in,
                               int train, float tau, const unsigned long long* seed_dev, unsigned long long site_offset,
                               float* logits, float* noise_out, float* y, float* sel, hipStream_t stream);
VC_API int vc_mhst_gate_bwd(int B, const float* dsel, const float* y, float scale, float* dlogits, hipStream_t stream);
VC_API int vc_mhst_headmask_fwd(int B, int T, int Wd, const float* X, const float* sel, float* Y, hipStream_t stream);
VC_API int vc_mhst_headmask_bwd(int B, int T, int Wd, const float* dY, const float* X, const float* sel, float* dX,
                                float* dsel, float beta, hipStream_t stream);
VC_API int vc_mhst_pool_fwd(int B, const float* X, const float* pw, float eps, float* Y, hipStream_t stream);
VC_API int vc_mhst_pool_bwd(int B, const float* X, const float* pw, float eps, const float* dY, float* dX, float* part,
                            hipStream_t stream);
VC_API int vc_mhst_attn_fwd(int B, const float* QKV, float scale, float p, unsigned long long seed, unsigned char* mask,
                            float* O, hipStream_t stream);
VC_API int vc_mhst_attn_fwd_ds(int B, const float* QKV, float scale, float p, const unsigned long long* seed_dev,
                               unsigned long long site_offset, unsigned char* mask, float* O, hipStream_t stream);
VC_API int vc_mhst_attn_bwd(int B, const float* QKV, float scale, float p, const unsigned char* mask, const float* dO,
                            float* dQKV, hipStream_t stream);
VC_API int vc_mhst_hsattn_fwd(int B, const float* X, long ldx, const float* Wg, const float* bg, const float* noise_in,
                              int train, float tau, unsigned long long seed_gate, unsigned long long seed_prob,
                              const float* QKV, const float* pw, float eps, float scale, float p, unsigned char* mask,
                              float* logits, float* noise_out, float* y, float* sel, float* AM, hipStream_t stream);
VC_API int vc_mhst_hsattn_fwd_ds(int B, const float* X, long ldx, const float* Wg, const float* bg,
                                 const float* noise_in, int train, float tau, const unsigned long long* seed_dev,
                                 unsigned long long gate_offset, unsigned long long prob_offset, const float* QKV,
                                 const float* pw, float eps, float scale, float p, unsigned char* mask, float* logits,
                                 float* noise_out, float* y, float* sel, float* AM, hipStream_t stream);
VC_API int vc_mhst_hsattn_bwd(int B, const float* QKV, const float* sel, const float* y, const float* pw, float eps,
                              float scale, float p, const unsigned char* mask, const float* dAM, const float* dsel_in,
                              float gscale, float* dQKV, float* part, float* dlogits, hipStream_t stream);
VC_API int vc_mhst_tail_fwd(int B, int ncls, const float* lg1, const float* z, long ldz, const float* W2,
                            const float* b2, const float* cv, const float* cc, float* p1, float* p2, float* avg,
                            float* out, hipStream_t stream);
VC_API int vc_mhst_tail_bwd(int B, int ncls, const float* dout, const float* p1, const float* p2, const float* avg,
                            const float* W2, const float* cv, const float* cc, float* dlg1, float* dz, long lddz,
                            float* part, hipStream_t stream);

/* ---------------------------------------------------------------- GLT-Net (the global-local transformer comparison model)
 * model/compare_method/GLT_Net/GLT_Net.py over channels-last rows; P = the model's patch side (even, 2 <= P <= 8 for
 * the fusion kernels), NP = P^2, T = NP + 1, token width 64.  The model's three scales P, 2P, 3P are the centre crops
 * of ONE 3P patch.  All fp32; no float atomics; every sum runs in a fixed order (two runs are bit-identical).
 *
 * vc_glt_crops: x [B, C, 3P, 3P] (NCHW) -> the three centre crops as channels-last rows of ld >= C floats, columns
 *   C .. ld - 1 written 0:  r_k[(b, i, j)][c] = x[b, c, i + o_k, j + o_k],  i, j < k P,  o_1 = P, o_2 = P / 2, o_3 = 0.
 *   One launch; the rows are conv inputs and MSE targets; there is no backward.
 *
 * vc_glt_fuse_fwd / _bwd: fusion, spatial embedding, SA-GDR and the token buffer, one block per sample.  From the
 *   2x2-max-pooled maps of the two modalities at the three scales, pa_k, pb_k [B, n_k, 64], n_k = (k P / 2)^2 (rows =
 *   pooled positions), and device scalars xs1, xs2:
 *     f_k = xs1 pa_k + xs2 pb_k;      e_k[b, j, c] = bias_k[j] + sum_p W_k[j][p] f_k[b, p, c]     (W_k [NP, n_k])
 *     avg = (e_1 + e_2 + e_3) / 3;    mx = max(e_1, e_2, e_3)                                     (per (b, j, c))
 *     g[b, j, c] = sigmoid(sum_{ty, tx < 7} w7[0][ty][tx] avg[b, (jy + ty - 3, jx + tx - 3), c]
 *                                         + w7[1][ty][tx] mx[b, (jy + ty - 3, jx + tx - 3), c])   (zero outside P x P)
 *     xcnn[b, j, :] = g[b, j, :];   X0[b, 0, :] = cls + pos[0];   X0[b, 1 + j, :] = (xcnn[b, j, :] + pos[1 + j]) + pos[0]
 *   e [3, B, NP, 64] is written for the backward.  The backward takes dX0 [B, T, 64] and dxcnn [B, NP, 64] (the CNN
 *   classifier's path), recomputes avg / mx and the arg max (the first maximum in k order) from e, and writes dpa_k,
 *   dpb_k and one partial row per sample,
 *     part[b] = [dW_1 NP x n_1 | dbias_1 NP | dW_2 | dbias_2 | dW_3 | dbias_3 | dw7 98 | dxs1, dxs2]
 *   (vc_glt_fuse_part_floats(P) floats); the caller sums the rows (vc_colsum) and takes dpos / dcls from dX0:
 *   dpos[0] = sum over all B T rows, dpos[1 + j] = sum_b dX0[b, 1 + j], dcls = sum_b dX0[b, 0].
 *
 * vc_glt_upconv_fwd / _wgrad / _dgrad: nn.Upsample(scale_factor = s, nearest) followed by Conv2d(C, O, 3, padding 1)
 *   as ONE implicit GEMM on v_mfma_f32_32x32x2_f32 (vc_conv3x3_tap_*'s structure: tap-major K, Wt from vc_conv3x3_pack
 *   mode 0); the upsampled tensor is never written.  x [B P^2, ldx] rows of a P x P map, y / dy [B (sP)^2, ldy] rows,
 *   s in {1, 2, 3}:
 *     y[b, (i, j), o] = bias[o] + sum_{di, dj < 3} sum_c w[o][c][di][dj] u[b, (i + di - 1, j + dj - 1), c],
 *     u[b, (p, q), c] = x[b, (floor(p / s), floor(q / s)), c] for 0 <= p, q < sP, 0 outside
 *   wgrad: dw [O][C][3][3] (the torch layout) and db [O], both overwritten; dgrad: dx = beta dx + the sum over the
 *   s x s replicas of each input pixel (K = s^2 x 9 taps x O walked in a fixed order).  Small grids split K into
 *   slabs of ws (combined in slice order by a second launch); ws may be null.
 *
 * vc_glt_sigmse_fwd / _bwd: y [rows, C] (ldy) is overwritten by sigmoid(y) and
 *     loss = (accumulate ? loss : 0) + weight / (rows C) * sum (sigmoid(y) - t)^2        (t [rows, C], ldt)
 *   The per-block partial sums (2048 elements each) and their combination are FP64: every block writes its partial to
 *   ws (vc_glt_sigmse_ws_floats(rows, C) floats, 8-B aligned), the last-arriving block (one zeroed arrival counter, left
 *   zero) adds them in block order and rounds once to fp32.  bwd: d[r, c] = dloss * 2 weight / (rows C) *
 *   (sg - t) sg (1 - sg) from the saved sigmoid sg (d may be sg).
 *
 * vc_glt_tail_fwd / _bwd: the classifier tail: avg[b, k] = mean_t z[b, t, k] over z [B, HW, 32] (ldz),
 *     p2 = softmax(W2 avg + b2),  out = c1 lg1 + c2 p2      (raw logits plus probabilities; c1, c2 device scalars;
 *   ncls <= 256).  bwd: dlg1, dz (lddz) and part[b] = [dW2 ncls x 32 | db2 ncls | dc1, dc2] (ncls * 33 + 2 floats). */
VC_API int vc_glt_crops(int B, int C, int P, const float* x, float* r1, float* r2, float* r3, int ld,
                        hipStream_t stream);
VC_API int vc_glt_fuse_part_floats(int P);
VC_API int vc_glt_fuse_fwd(int B, int P, const float* pa1, const float* pb1, const float* pa2, const float* pb2,
                           const float* pa3, const float* pb3, const float* xs1, const float* xs2, const float* W1,
                           const float* b1, const float* W2, const float* b2, const float* W3, const float* b3,
                           const float* w7, const float* pos, const float* cls, float* xcnn, float* X0, float* e,
                           hipStream_t stream);
VC_API int vc_glt_fuse_bwd(int B, int P, const float* pa1, const float* pb1, const float* pa2, const float* pb2,
                           const float* pa3, const float* pb3, const float* xs1, const float* xs2, const float* W1,
                           const float* W2, const float* W3, const float* w7, const float* xcnn, const float* e,
                           const float* dX0, const float* dxcnn, float* dpa1, float* dpb1, float* dpa2, float* dpb2,
                           float* dpa3, float* dpb3, float* part, hipStream_t stream);
VC_API int vc_glt_upconv_fwd(int B, int P, int s, int C, int O, const float* x, long ldx, const float* wt,
                             const float* bias, float* y, long ldy, float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_glt_upconv_wgrad(int B, int P, int s, int C, int O, const float* x, long ldx, const float* dy, long lddy,
                               float* dw, float* db, float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_glt_upconv_dgrad(int B, int P, int s, int C, int O, const float* dy, long lddy, const float* wt,
                               float beta, float* dx, long lddx, float* ws, long ws_floats, hipStream_t stream);
VC_API int vc_glt_sigmse_ws_floats(long rows, int C);
VC_API int vc_glt_sigmse_fwd(long rows, int C, float* y, long ldy, const float* t, long ldt, float weight,
                             int accumulate, float* loss, float* ws, long ws_floats, unsigned int* counter,
                             hipStream_t stream);
VC_API int vc_glt_sigmse_bwd(long rows, int C, const float* sg, long lds, const float* t, long ldt, float weight,
                             const float* dloss, float* d, long ldd, hipStream_t stream);
VC_API int vc_glt_tail_fwd(int B, int ncls, int HW, const float* lg1, const float* z, long ldz, const float* W2,
                           const float* b2, const float* c1, const float* c2, float* p2, float* avg, float* out,
                           hipStream_t stream);
VC_API int vc_glt_tail_bwd(int B, int ncls, int HW, const float* dout, const float* lg1, const float* p2,
                           const float* avg, const float* W2, const float* c1, const float* c2, float* dlg1, float* dz,
                           long lddz, float* part, hipStream_t stream);

#endif /* VITCNN_H */
