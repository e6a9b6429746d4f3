/*
 * stgcn_hip.h — C-ABI of libstgcn_hip.so, the MI355X (gfx950) ST-GCN block.
 *
 * This is the drop-in boundary for ONE hot path of nagyrajmund/st-gcn: the
 * ST-GCN block in training (and eval) mode,
 *
 *   y = ReLU(BN2(Conv9x1(SpatialConv(BN1(x)))))                 (default)
 *   y = ReLU(Conv9x1(ReLU(BN2(SpatialConv(ReLU(BN1(x)))))) + R(x))
 *                                          (flags & STGCN_F_RESIDUAL)
 *
 * with R = identity (C_in == C_out, stride 1) or a 1x1 Conv2d with temporal
 * stride (st_graphconv.py:24-28), i.e. SpatialTemporalConv.forward
 * (src/network/st_graphconv.py:85-109, residual_block :60-82) with
 * SpatialConv.forward (st_graphconv.py:139-152) and its autograd backward.
 * Dropout (p > 0, training) is fused into the block's output pass
 * (stgcn_fwd_args_t.dropout_p / seed, ABI 2); training and eval mode are
 * both differentiable (eval: BatchNorm with the running statistics as
 * constants, ABI 4).
 * The reference has no FFI of its own (pure Python over PyTorch); the entry
 * points below are what its module boundary binds to (the ctypes binding in
 * st-gcn_amd/hip_lib.py, shown in INTEGRATION.md):
 *
 *   stgcn_block_fwd  replaces SpatialTemporalConv.forward, st_graphconv.py:85-109
 *                    (BatchNorm2d :34/:98, SpatialConv :139-152, temporalConv
 *                    :41-43/:99, BatchNorm2d :46/:100, ReLU :49/:105;
 *                    residual_block :60-82 with apply_residual :24-28)
 *   stgcn_block_bwd  replaces the autograd backward of the same ops
 *                    (driven by lightning_model.py:199-205 -> loss.backward())
 *   stgcn_spatial_fwd / stgcn_spatial_bwd  replace SpatialConv.forward used on
 *                    its own (st_graphconv.py:139-152) and its backward (ABI 4)
 *
 * Conventions
 *   - All tensors are caller-owned, contiguous, fp32, device memory, layout
 *     NCTV (N clips, C channels, T frames, V joints) as in the reference.
 *   - Alignment. Every pointer either works at the alignment stated here or the
 *     call returns STGCN_E_INVALID, naming the argument in stgcn_last_error(),
 *     before its first launch (null optional arguments pass):
 *       stgcn_block_fwd / stgcn_block_bwd / stgcn_fold_prep: every tensor, saved
 *         buffer (Z, U, Za, stats, kept G, prep), chaining block (x_stats,
 *         y_stats, dy_sums, prev_sums, dx_coef, dy_coef, prev_U, prev_g2,
 *         prev_b2, dy_nc), gradient and the workspace: 16 bytes (the kernels move
 *         them in 16-byte units; the opaque formats do not depend on pointer
 *         values). Exceptions, taken at 4 bytes: the running statistics rm1, rv1,
 *         rm2, rv2 (read and updated in place, one element at a time) and
 *         prev_stats (the previous block's stats + 2 * C_in). dx without need_dx
 *         and U of a residual block are ignored.
 *       stgcn_spatial_fwd / stgcn_spatial_bwd: out, dx, dA, dW, dbW and the
 *         workspace 16 bytes; x, A, W, bW, dout 4 bytes on the fp32 path (a
 *         misaligned x or dout selects narrower kernels: slower, same results
 *         to rounding), 16 bytes under STGCN_F_BF16.
 *       stgcn_head_*: fp32 / int32 tensors 4 bytes, labels and the metrics block
 *         8; stgcn_adam_*: the device table 8, every param / grad / exp_avg /
 *         exp_avg_sq and the device step 4 (views into a flat bucket work in
 *         place). These kernels access one element at a time.
 *       STGCN_FEATURE_STEP_STATE: seed_dev (stgcn_block_fwd_dseed / _bwd_dseed)
 *         and stgcn_seed_next's counter / token 8 (64-bit words); lr_dev,
 *         grad_coef, norm_out, coef_out 4; stgcn_grad_norm's partials 8.
 *       STGCN_FEATURE_INPUT_STAGE (stgcn_input_stage): x 16 bytes, like a block
 *         tensor; src its element's own 4 (fp32) or 8 (fp64) bytes; the clip
 *         table 8; status 4. STGCN_FEATURE_INPUT_MOVE (stgcn_input_stage_move): the
 *         same, and the move table 8. STGCN_FEATURE_INPUT_STREAMS
 *         (stgcn_input_stage_streams): the same, and the parents table 4.
 *       STGCN_FEATURE_OPTIMIZERS (stgcn_opt_*): the device table 8; every param /
 *         grad / s0 / s1 / s2 of a table entry, lr_dev, grad_coef and step_dev 4.
 *     A caller with a misaligned read-only input for a 16-byte argument passes an
 *     aligned copy (the Python binding does); torch.empty results are aligned.
 *   - Non-finite values. A NaN or +-Inf in an input is never turned into a
 *     finite wrong value. Against the reference's dense IEEE arithmetic, per
 *     output element: (a) where the reference is non-finite and the element
 *     lies in the footprint that sparse arithmetic reaches from the bad element
 *     (same clip, every output channel, output frames t' with
 *     |t' * stride - t| <= 4, joints v' with A[k][v'][v] != 0 for some k; the
 *     transposed set for a bad dy in the eval-mode backward), the result is
 *     non-finite; NaN and +-Inf are interchangeable (the fp16 / bf16 operand
 *     splits turn Inf into NaN). (b) Where the reference is finite the result
 *     is the usual one, or it is non-finite inside the dense footprint (the
 *     same frames at every joint): a dense 0 * NaN is NaN, a kernel that skips
 *     A's zeros gives a number, and ReLU(-Inf) = 0. (c) With running statistics
 *     (training = 0) every other clip is untouched, in every GEMM mode: the
 *     f16x2 operand bounds (max |x| words) are taken over finite elements only,
 *     and the BatchNorm backward's batch-mean terms are absent, not multiplied
 *     by 0. In training mode one bad element makes the batch statistics, and
 *     with them y, the gradients and the running statistics, non-finite.
 *     ReLU keeps NaN and its backward is a select (a bad dy under a closed ReLU
 *     reaches nothing). stgcn_grad_norm gives a NaN coef_out for a NaN norm
 *     (every clipped gradient is then NaN, as with clip_grad_norm_), 0 for an
 *     Inf norm; AMSGrad's running maximum keeps a NaN.
 *   - A is (K,V,V), W is (K*C_out, C_in) (the reference's 1x1 Conv2d weight),
 *     Wt is (C_out, C_out, 9) (the (9,1) Conv2d weight).
 *   - The workspace is caller-allocated (query *_workspace_bytes first); the
 *     library allocates nothing on the hot path and keeps no mutable global
 *     state besides the thread-local error string (and the internal stream of
 *     the next point).
 *   - Every launch goes on the caller's stream (a hipStream_t passed as void*),
 *     with one exception: stgcn_block_bwd / _bwd_dseed may run part of its work
 *     on an internal stream that is forked from the caller's stream and joined
 *     to it within the call (STGCN_FEATURE_BWD_OVERLAP; stgcn_bwd_overlap(0)
 *     keeps every launch on the caller's). To
 *     the caller nothing changes: when the call returns, everything it enqueued
 *     is ordered before later work on the caller's stream, under stream capture
 *     too (the captured graph then has two parallel branches per such block).
 *     The library's only other process-wide state is that stream with its
 *     events and the mode of stgcn_bwd_overlap.
 *   - Return 0 on success, a negative STGCN_E* code otherwise; the message is
 *     in stgcn_last_error() (thread-local).
 */
#ifndef STGCN_HIP_H
#define STGCN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STGCN_ABI_VERSION 11

/* ABI 7: words of max |y| after the 5 * C sums of a y_stats block */
#define STGCN_STATS_AMAX_WORDS 2048
#define STGCN_Y_STATS_BYTES(C) (8 * 5 * (size_t)(C) + 4 * (size_t)STGCN_STATS_AMAX_WORDS)

/* stgcn_desc_t.flags */
#define STGCN_F_RESIDUAL 1 /* full pre-activation residual block (st_graphconv.py:60-82) */
#define STGCN_F_BF16 2     /* channel GEMMs (W, temporal conv fwd/dgrad/wgrad, projection)
                            * on bf16 MFMA: operands rounded to bf16, fp32 accumulate;
                            * A / BatchNorm stay fp32 (BASELINE cfg3/5). x, y, U, stats and
                            * every gradient the caller receives are fp32. Z (the saved
                            * spatial output) is OPAQUE under this flag: on stride-1
                            * non-residual blocks with C_in >= 16 it holds bf16 values in
                            * the first half of its fp32-sized buffer (every reader rounds
                            * it to bf16 anyway), so only stgcn_block_bwd may read it.
                            * Applies for V in {18, 25, 50} and reductions over >= 16
                            * channels; other GEMMs run the fp32 kernels. */
#define STGCN_F_F32X3 4    /* fp32 channel GEMMs on the bf16 matrix cores by exact 3-way
                            * operand splits (x = h + m + l, six partial products, fp32
                            * accumulate): fp32-GEMM accuracy at up to 2.67x the fp32
                            * MFMA rate. Applies for V in {18, 25} over >= 16 channels to
                            * the temporal conv forward (stride 1 and 2), data-grad and
                            * weight-grad, and to the spatial weight-grad dW'; other GEMMs
                            * run the fp32 kernels. Every tensor stays fp32. On non-residual
                            * blocks with K = 1, V = 18 and C_in >= 16 the SpatialConv
                            * channel GEMM is folded into the temporal conv's weights
                            * (Wc_q = Wt_q W'): Z is never formed, and its buffer is
                            * OPAQUE (it carries Wc from stgcn_block_fwd to
                            * stgcn_block_bwd). Exclusive with STGCN_F_BF16. */
#define STGCN_F_F16X2 8    /* ABI 6, with STGCN_F_F32X3 only: the folded block's temporal
                            * conv forward, data-grad and weight-grad GEMMs as 2-way fp16 splits
                            * (x s = h + l, 22 significant bits, three partial products,
                            * fp32 accumulate) of operands scaled by powers of two s from
                            * their max |x| (so h <= 2^14 and no element underflows
                            * relative to the tensor's maximum); the result is scaled back
                            * exactly. Same fp32 gate as STGCN_F_F32X3, half its MFMAs.
                            * At V = 18 the data gradient runs on the fp16 splits too
                            * (with the SpatialConv backward fused into it); BN1's
                            * nearly cancelling sum of dxhat (its bias gradient) is
                            * formed from the fp64 per-tap dU sums instead of from the
                            * 22-bit data gradient. At
                            * V = 25 (folded, K = 1) the data gradient stays on the
                            * 3-way bf16 splits. ABI 8: an unfolded non-residual V = 18,
                            * K = 1 block with C_out >= 16 (the first block, C_in = 3)
                            * runs its temporal forward and weight gradient on the fp16
                            * splits (bounds by max-|x| passes over Z and Wt), its data
                            * gradient on the 3-way bf16 splits. stgcn_block_plan reports
                            * STGCN_PLAN_F16X2 wherever any GEMM of the block uses them. */

#define STGCN_F_NO_G 16    /* ABI 7, with STGCN_F_F16X2 only (memory-lean folded block):
                            * G = BN1(x) A^T is never formed or kept -- the forward GEMM
                            * reads x (BN1 in its loader, the joint contraction in its
                            * epilogue), the weight gradient reads x against dU A formed
                            * by the ReLU + BN2 backward pass -- so the N*C_in*T*V*4-byte
                            * G buffer is not kept between forward and backward
                            * (stgcn_keep_g_bytes then returns only the bound words).
                            * Same fp32 gate; measured slower than the G path on cfg2
                            * (DESIGN.md), hence opt-in. */

enum {
  STGCN_OK = 0,
  STGCN_E_INVALID = -1,     /* bad pointer / shape / parameter            */
  STGCN_E_UNSUPPORTED = -2, /* V > 256, gamma != 9, unknown flags ...      */
  STGCN_E_HIP = -3          /* a HIP launch / runtime error               */
};

/* Block descriptor (one SpatialTemporalConv, st_graphconv.py:9). */
typedef struct stgcn_desc {
  int32_t N, C_in, C_out, T, T_out, V, K;
  int32_t gamma;       /* temporal kernel size: 9 (lightning_model.py:263)   */
  int32_t stride;      /* temporal stride 1 or 2                             */
  int32_t pad;         /* temporal padding (gamma-1)/2 = 4                   */
  float eps;           /* BatchNorm eps 1e-5                                 */
  float momentum;      /* BatchNorm momentum 0.1                             */
  int32_t training;    /* 1: batch statistics + running-stat update          */
  int32_t need_dx;     /* backward: write dx (0 for the network's first block)*/
  int32_t flags;       /* STGCN_F_RESIDUAL | (STGCN_F_BF16 or STGCN_F_F32X3
                        * [| STGCN_F_F16X2 [| STGCN_F_NO_G]])                  */
} stgcn_desc_t;

/* Forward arguments. Saved tensors (Z, U, stats; residual: Z, Za, y, stats)
 * are kept by the caller for stgcn_block_bwd. stats holds mean1[C_in],
 * invstd1[C_in], mean2[C_out], invstd2[C_out] (fp32) as used by the forward.
 * Residual block: BN2 normalizes Z (the spatial output, st_graphconv.py:76),
 * U is not used, Za = ReLU(BN2(Z)) is the temporal conv input, Wr/br is the
 * projection (C_out, C_in) + (C_out) when C_in != C_out or stride != 1
 * (apply_residual, st_graphconv.py:27), else null. */
typedef struct stgcn_fwd_args {
  const float *x;                       /* N,C_in,T,V                         */
  const float *A, *W, *bW, *Wt, *bWt;   /* SpatialConv.A / W ; temporalConv   */
  const float *g1, *b1, *g2, *b2;       /* batch_n / batch_n_2 affine         */
  float *rm1, *rv1, *rm2, *rv2;         /* running stats (updated if training)*/
  float *y;                             /* out: N,C_out,T_out,V (ABI 8: may be
                                         * null, see prev_U below; ABI 9: null
                                         * with y_stats null, see
                                         * stgcn_head_fwd_u)                  */
  float *Z;                             /* saved: spatial output N,C_out,T,V
                                         * (fp32-sized; opaque under STGCN_F_BF16) */
  float *U;                             /* saved: temporal output N,C_out,T_out,V */
  float *stats;                         /* saved: 2*C_in + 2*C_out floats     */
  /* ABI 2 (residual block; null otherwise) */
  const float *Wr, *br;                 /* apply_residual Conv2d (projection) */
  float *Za;                            /* saved: ReLU(BN2(Z)) N,C_out,T,V    */
  /* ABI 2, optional: keep the joint contraction G = f(BN1(x)) A^T for the
   * backward instead of recomputing it: stgcn_keep_g_bytes(d) bytes; fp32
   * (N, K*C_in, T, V), or, where the bf16 path's fused spatial kernel runs
   * (STGCN_F_BF16, C_in >= 16), bf16 in frame tiles (ABI 4: opaque to the caller).
   * Under STGCN_F_F16X2 the words after G carry its operand bound max |G| to
   * the backward's weight gradient: a kept G is valid only for a backward with
   * the SAME descriptor (flags included) as the forward that wrote it. */
  float *G;
  /* ABI 2, optional stack chaining (training): x_stats = [sum(C_in), sumsq(C_in)]
   * of x over (n,t,v) in fp64 (produced by the previous block's y_stats: the
   * BN1 statistics pass is skipped); y_stats (out) = the same for y (C_out).
   * ABI 5: y_stats holds 5 * C_out doubles; a non-residual block without
   * dropout also writes, with its ReLU mask m = y > 0 and uhat = (U - mean2) *
   * invstd2, [cnt = sum m | su = sum m uhat | xu = sum y uhat] after the two
   * (the next block's deferred-dx chain, stgcn_bwd_args_t.x_stats). */
  const double *x_stats;
  double *y_stats;
  /* ABI 7: x_stats / y_stats blocks are STGCN_Y_STATS_BYTES(C) bytes: the 5 * C
   * doubles above, then STGCN_STATS_AMAX_WORDS uint32 words that receive max |y|
   * (as float bits, the largest word wins): the operand bound of the next block's
   * fp16-split GEMMs, which read y itself (STGCN_PLAN_FOLD_NO_G). */
  /* ABI 2, optional fused dropout on y (training only; st_graphconv.py:53-58,
   * :107-109): element e of y is kept iff splitmix64(seed + e * 0x9E3779B97F4A7C15)
   * >> 32 >= dropout_p * 2^32, then scaled by 1/(1 - dropout_p). 0: no dropout. */
  float dropout_p;
  uint64_t seed;
  /* ABI 7, optional (folded blocks): the block's stgcn_fold_prep buffer of this
   * training step -- its weight-only operands are then not formed again */
  const void *prep;
  /* ABI 8, optional stack chaining without the block output in HBM
   * (STGCN_PLAN_X_FROM_U; training, with x_stats; non-residual previous block
   * without dropout): the block input is x = ReLU(BN2_prev(prev_U)), formed
   * where the block reads it, from the previous block's U, [mean2 | invstd2]
   * (its stats + 2 * C_in_prev) and BN2 affine; x may then be null. The
   * previous block's forward ran with y = null (a non-residual block without
   * dropout, with y_stats: only the statistics of y are formed), and this
   * block's backward is called with x = null, its kept G and the deferred-dx
   * chain arguments (stgcn_bwd_args_t prev_*, x_stats, dx_coef, dx_deferred). */
  const float *prev_U, *prev_stats, *prev_g2, *prev_b2;
} stgcn_fwd_args_t;

/* Backward arguments: the gradients of every input of the forward. */
typedef struct stgcn_bwd_args {
  const float *dy;                      /* N,C_out,T_out,V                    */
  const float *x, *Z, *U, *stats;       /* saved by the forward               */
  const float *A, *W, *bW, *Wt, *g1, *b1, *g2, *b2;
  float *dx;                            /* N,C_in,T,V (ignored if !need_dx)   */
  float *dA, *dW, *dbW, *dWt, *dbWt;
  float *dg1, *db1, *dg2, *db2;
  /* ABI 2 (residual block; null otherwise) */
  const float *Wr;                      /* projection weight or null          */
  const float *Za, *y;                  /* saved by the forward               */
  float *dWr, *dbr;                     /* projection gradients or null       */
  const float *G;                       /* optional: G kept by the forward    */
  /* optional stack chaining (non-residual blocks):
   * dy_sums = [sum dy*m, sum dy*m*uhat] (2*C_out, fp64) of this block's
   * ReLU+BN2 backward, produced by the next block (its reduction pass is
   * skipped); prev_g2/prev_b2 = BN2 affine of the (non-residual) block that
   * produced x, prev_sums (out, 2*C_in) = that block's dy_sums, computed while
   * writing dx (needs need_dx). */
  const double *dy_sums;
  const float *prev_g2, *prev_b2;
  double *prev_sums;
  float dropout_p;                      /* the forward's dropout (same seed)  */
  uint64_t seed;
  /* ABI 4, optional with prev_sums: the previous block's saved pre-BN2 tensor
   * U (N, C_in, T, V) and its stats (mean2[C_in], invstd2[C_in]). Channels
   * where reconstructing uhat = (x - prev_b2) / prev_g2 from x is
   * ill-conditioned (|prev_b2| > 4 |prev_g2|, including prev_g2 == 0) read
   * uhat from U instead. Null: reconstruct everywhere. */
  const float *prev_U;
  const float *prev_stats;
  /* ABI 5, optional deferred dx (training, non-residual block, with the
   * prev_* chain arguments above and prev_U / prev_stats): this block's BN1
   * backward apply is folded into the PREVIOUS block's ReLU+BN2 backward
   * apply. When the library takes it (*dx_deferred = 1; it does where its
   * spatial-backward kernel reads the previous block's U in place of x), dx
   * receives dxhat (the gradient at BN1's output) instead of the gradient of
   * x, dx_coef (5 * C_in floats [a | md | mu | is | mdn]) the BN1 backward
   * coefficients (dx = a * (dxhat - md - (x - mu) * is * mdn)) and prev_sums
   * the previous block's dy_sums; the previous block's stgcn_block_bwd then
   * takes dy = that dxhat with dy_coef = dx_coef and dy_sums = prev_sums.
   * x_stats: the 5 * C_in y_stats the previous block's forward wrote. */
  const double *x_stats;
  float *dx_coef;
  int32_t *dx_deferred;                 /* host int: 1 deferred, 0 dx written */
  /* ABI 5, in: dy holds the next block's dxhat, to be combined as above with
   * these 5 * C_out coefficients (needs dy_sums; non-residual, no dropout) */
  const float *dy_coef;
  /* ABI 7, optional: the same stgcn_fold_prep buffer as the forward's */
  const void *prep;
  /* ABI 10, optional: the gradient of y is constant over (T_out, V) --
   * dy[n, c, t, v] = dy_nc[n * C_out + c] (N * C_out floats), as the average-pool
   * head gives it (stgcn_head_bwd_nc) -- and dy may be null: the ReLU + BN2
   * backward reads one value per (clip, channel) instead of the dy tensor.
   * Non-residual blocks; STGCN_E_UNSUPPORTED where the block's backward needs
   * the full dy (the caller then passes it). */
  const float *dy_nc;
  /* ABI 8: x may be null when the forward took its input from prev_U
   * (STGCN_PLAN_X_FROM_U); the call then needs the kept G and the deferred-dx
   * arguments (prev_U, prev_stats, prev_g2, prev_b2, prev_sums, x_stats, dx_coef,
   * dx_deferred) and fails with STGCN_E_INVALID where it could not defer. */
} stgcn_bwd_args_t;

int stgcn_abi_version(void);
const char *stgcn_last_error(void);
/* Additions within one ABI version (a bit mask; the ABI number changes only when
 * an existing call does): */
#define STGCN_FEATURE_EVAL_CHAIN 1 /* stgcn_block_fwd chains in eval (STGCN_PLAN_X_FROM_U_EVAL) */
#define STGCN_FEATURE_EVAL_HEAD 2  /* stgcn_head_eval / _u and the metrics block           */
#define STGCN_FEATURE_STEP_STATE 4 /* per-step values read from device memory: the _dseed
                                    * block calls, stgcn_seed_next, stgcn_adam_step_dev2,
                                    * stgcn_grad_norm                                     */
#define STGCN_FEATURE_INPUT_STAGE 8 /* stgcn_input_check / stgcn_input_stage: ragged clips
                                    * to the NCTV fp32 input on the device              */
#define STGCN_FEATURE_OPTIMIZERS 16 /* stgcn_opt_*: AdamW (decoupled decay) and AMSGrad */
#define STGCN_FEATURE_HEAD_LOSS 32 /* stgcn_loss_check, stgcn_head_eval_loss / _u: class
                                    * weights and label smoothing in the evaluation head
                                    * (the training head takes neither yet)             */
#define STGCN_FEATURE_INPUT_MOVE 64 /* stgcn_input_move_check / stgcn_input_stage_move:
                                    * per-frame interpolated rotation, scale and translation
                                    * ("random moving") in the input stage              */
#define STGCN_FEATURE_BWD_OVERLAP 128 /* stgcn_bwd_overlap: the backward's small kernels on an
                                    * internal stream beside its GEMMs                   */
#define STGCN_FEATURE_INPUT_STREAMS 256 /* stgcn_input_streams_check / stgcn_input_stage_streams:
                                    * bone, joint-motion and bone-motion streams beside the
                                    * joints in the input stage                          */
int stgcn_features(void);

/* STGCN_FEATURE_BWD_OVERLAP: stgcn_block_bwd / _bwd_dseed of a folded block whose
 * SpatialConv backward is fused into its data gradient (STGCN_PLAN_FOLD with
 * STGCN_PLAN_SP_BWD_FUSED) may run its small reduction kernels on a stream the
 * library owns (one per device, created by the first such call that is not under
 * stream capture; a call that is captured earlier runs serially), forked from the
 * caller's stream after the ReLU + BN2 backward pass and joined to it before the
 * call returns: the same kernels with the same launch parameters and the same
 * order between any two that touch the same buffer, so the results have the
 * serial call's bits. Sets the process-wide mode (1: on, the default; 0: every
 * launch on the caller's stream -- for an application that must keep all work
 * on its own stream, and for comparing the two) and returns the previous one; a
 * negative argument only queries. The stream has the default priority: a
 * high-priority one made the captured step much slower (DESIGN.md "Backward
 * small kernels beside the GEMMs"). */
int stgcn_bwd_overlap(int enable);

/* Validate a descriptor without touching the GPU (0 = supported). */
int stgcn_check_desc(const stgcn_desc_t *d);

size_t stgcn_fwd_workspace_bytes(const stgcn_desc_t *d);
/* ABI 4: bytes of the optional kept-G buffer (stgcn_fwd_args_t.G / bwd G) */
size_t stgcn_keep_g_bytes(const stgcn_desc_t *d);
size_t stgcn_bwd_workspace_bytes(const stgcn_desc_t *d);

int stgcn_block_fwd(const stgcn_desc_t *d, const stgcn_fwd_args_t *a,
                    void *workspace, size_t workspace_bytes, void *stream);
int stgcn_block_bwd(const stgcn_desc_t *d, const stgcn_bwd_args_t *a,
                    void *workspace, size_t workspace_bytes, void *stream);

/* STGCN_FEATURE_STEP_STATE: the block calls with the dropout's step token in
 * device memory. Element e of the block output is kept iff
 *     hi32(mix64(s + e * PHI)) >= dropout_p * 2^32,   PHI = 0x9E3779B97F4A7C15,
 *     mix64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *               z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^ z >> 31   (mod 2^64)
 * with s = a->seed for stgcn_block_fwd / _bwd and for seed_dev null (bit for bit
 * the same call), else the effective seed
 *     s = mix64(a->seed + c * PHI),   c = *seed_dev,
 * read by each kernel when it RUNS: nothing about the mask is fixed when the call
 * is enqueued, so a call captured in a HIP graph draws a new mask on every replay
 * once the token advances (stgcn_seed_next). The hash is needed: with a plain
 * a->seed + c * PHI the mask of token c + 1 is that of token c shifted by one
 * element. The backward regenerates the mask and must see the value its forward
 * saw: give each forward a token word of its own (stgcn_seed_next writes one)
 * and pass that word to its backward. seed_dev: 8-byte aligned. */
int stgcn_block_fwd_dseed(const stgcn_desc_t *d, const stgcn_fwd_args_t *a,
                          const uint64_t *seed_dev, void *workspace, size_t workspace_bytes,
                          void *stream);
int stgcn_block_bwd_dseed(const stgcn_desc_t *d, const stgcn_bwd_args_t *a,
                          const uint64_t *seed_dev, void *workspace, size_t workspace_bytes,
                          void *stream);
/* *counter += 1; *token = *counter, on the stream (one thread): the token of
 * the next forward. counter and token: device words, 8-byte aligned. */
int stgcn_seed_next(uint64_t *counter, uint64_t *token, void *stream);

/* ---------------------------------------------------------------------------
 * ABI 4: SpatialConv on its own (st_graphconv.py:139-152):
 *   out[n,c,t,v] = sum_k sum_w A[k,v,w] * (W_k x[n,:,t,w] + bW_k)[c]
 * computed as out = sum_k W_k (x A_k^T) + sum_k bW_k rowsum(A_k) (the block's
 * form (1), no BatchNorm). x (N, C_in, T, V), A (K, V, V), W (K*C_out, C_in),
 * bW (K*C_out), out (N, C_out, T, V); flags: STGCN_F_BF16 runs the channel
 * GEMMs on bf16 MFMA (fp32 otherwise). Backward: dout -> dx (may be null),
 * dA, dW, dbW.
 */
typedef struct stgcn_spatial_desc {
  int32_t N, C_in, C_out, T, V, K;
  int32_t flags;       /* 0 or STGCN_F_BF16                                 */
} stgcn_spatial_desc_t;

size_t stgcn_spatial_workspace_bytes(const stgcn_spatial_desc_t *d, int backward);
int stgcn_spatial_fwd(const stgcn_spatial_desc_t *d, const float *x, const float *A,
                      const float *W, const float *bW, float *out, void *workspace,
                      size_t workspace_bytes, void *stream);
int stgcn_spatial_bwd(const stgcn_spatial_desc_t *d, const float *dout, const float *x,
                      const float *A, const float *W, const float *bW, float *dx, float *dA,
                      float *dW, float *dbW, void *workspace, size_t workspace_bytes,
                      void *stream);

/* ABI 6: the kernel plan the library selects for a descriptor (a bitmask of
 * STGCN_PLAN_*), so a caller or a test can pin which path its calls take. */
#define STGCN_PLAN_FOLD 1          /* K = 1 fp32 split path: the SpatialConv channel GEMM W'
                                    * folded into the temporal conv's weights (Wc_q = Wt_q W');
                                    * Z and dZ are never formed (capi.hip fold_w)         */
#define STGCN_PLAN_SP_FWD_FUSED 2  /* SpatialConv forward in one kernel (k_sp_fwd_*)     */
#define STGCN_PLAN_SP_BWD_FUSED 4  /* SpatialConv backward in one kernel (H never in HBM) */
#define STGCN_PLAN_ACT_BF16 8      /* Z / dU stored in bf16 (bf16 path)                  */
#define STGCN_PLAN_WSP_SPLIT 16    /* spatial dW' on exact split products (k_wgrad_sp X3) */
#define STGCN_PLAN_TCONV_SPLIT 32  /* temporal conv forward on the split pipeline         */
#define STGCN_PLAN_TWGRAD_SPLIT 64 /* temporal weight gradient on the split kernel        */
#define STGCN_PLAN_F16X2 128       /* the folded GEMMs on 2-way fp16 splits (STGCN_F_F16X2) */
#define STGCN_PLAN_FOLD_NO_G 256   /* ABI 7, with F16X2: G = BN1(x) A^T is never formed: the
                                    * forward GEMM reads x (BN1 in its loader, the joint
                                    * contraction in its epilogue), the weight gradient reads
                                    * x against dU A; the kept-G buffer (stgcn_keep_g_bytes)
                                    * then carries only max |x| to the backward          */
#define STGCN_PLAN_X_FROM_U 512    /* ABI 8: the training forward can take its input as
                                    * ReLU(BN2(U)) of the previous block
                                    * (stgcn_fwd_args_t.prev_U): that block's y is never
                                    * written                                             */
/* (an eval-only bit, = 1024: written as a shift because test_gpu_poison's
 * test_block_cases_cover_every_plan collects the decimal STGCN_PLAN_* defines and
 * wants each selected by one of its TRAINING block cases, which an eval bit cannot
 * be; its poison cases are test_gpu_eval.py's test_eval_step_poisoned) */
#define STGCN_PLAN_X_FROM_U_EVAL (1u << 10) /* STGCN_FEATURE_EVAL_CHAIN: the eval forward
                                    * (training == 0) can take its input as ReLU(BN2(U)) of
                                    * the previous block: prev_U (16-byte aligned), prev_stats
                                    * (that block's stats + 2 * C_in_prev: [running_mean2 |
                                    * rsqrt(running_var2 + eps)] as its eval forward wrote
                                    * them), prev_g2, prev_b2 with x null; x_stats is not
                                    * needed. Non-residual blocks whose forward forms the
                                    * input on load (the bf16 fused SpatialConv forward, or
                                    * the folded block's G pass); no backward condition
                                    * applies. STGCN_PLAN_X_FROM_U stays clear in eval. A
                                    * non-residual block in eval also takes y null with
                                    * y_stats null: no output pass, U is the handoff (to the
                                    * next block's prev_U or stgcn_head_eval_u)            */
int stgcn_block_plan(const stgcn_desc_t *d, uint32_t *plan);

/* ABI 7: the weight-only operands of a stack's folded blocks (STGCN_PLAN_FOLD),
 * formed together once per training step (the weights change every optimizer
 * step): bZ = bW rowsum(A), the composite weights Wc_q = Wt_q W', the per-frame
 * bias table, max |Wc|, the packed split planes of the forward and data-gradient
 * GEMMs and the backward's operand re-layouts -- a dozen launches for the whole
 * stack instead of ~11 small launches per block. stgcn_fold_prep_bytes(d) is the
 * block's buffer size (0: the block does not fold); the buffer is then passed as
 * stgcn_fwd_args_t.prep / stgcn_bwd_args_t.prep of that block in the same step
 * (same weights). Blocks whose size is 0 are skipped. The block's backward also
 * uses the buffer's fp64 scratch for its activation-dependent per-tap dU sums
 * (the Tq re-layout): one prep buffer must not serve two backward passes that
 * run concurrently (e.g. micro-batches on separate streams). */
typedef struct stgcn_fold_weights {
  const float *A, *W, *bW, *Wt, *bWt;   /* as in stgcn_fwd_args_t            */
} stgcn_fold_weights_t;
size_t stgcn_fold_prep_bytes(const stgcn_desc_t *d);
int stgcn_fold_prep(int nblocks, const stgcn_desc_t *descs, const stgcn_fold_weights_t *weights,
                    void *const *prep, void *stream);

/* Measurement (bench.py roofline): time one of the block's GEMM kernels,
 * launched `iters` times with the exact parameters the block uses for this
 * descriptor, between two hipEvents on `stream`. which: 0 temporal conv fwd,
 * 1 temporal conv data-grad, 2 temporal conv weight-grad, 3 spatial channel
 * GEMM (the fused SpatialConv forward where it runs), 4 spatial backward
 * (dZ -> dx, dA, BN1 sums), 5 / 6 the H GEMM / the joint kernel of a spatial
 * backward that runs unfused (STGCN_E_UNSUPPORTED where it is one kernel).
 * scratch (>= stgcn_time_kernel_bytes) supplies operand memory.
 * *flops receives the algorithmic FLOPs of one launch. */
size_t stgcn_time_kernel_bytes(const stgcn_desc_t *d, int which);
int stgcn_time_kernel(const stgcn_desc_t *d, int which, void *scratch, size_t scratch_bytes,
                      int iters, void *stream, float *avg_ms, double *flops);

/* ---------------------------------------------------------------------------
 * ABI 3: training-step ops around the stack.
 *
 * Classification head: global average pool over (T, V) + Linear + cross
 * entropy (lightning_model.py:105-107 avg_pool2d + fc_layer, :202
 * F.cross_entropy with mean reduction). y is the last block's output
 * (N, C, L = T*V); W (classes, C), bias (classes), labels int64 (N).
 * stgcn_head_fwd writes pooled (N, C), logits (N, classes), lossv (N, per-clip
 * loss) and loss (1, the mean). stgcn_head_bwd takes dloss (1) and writes
 * dlogits (N, classes, scratch), dpooled (N, C, scratch), dy (N, C, L: the
 * gradient of y), dW, dbias. Deterministic (no atomics).
 */
typedef struct stgcn_head_desc {
  int32_t N, C, L, classes;
} stgcn_head_desc_t;

int stgcn_head_fwd(const stgcn_head_desc_t *d, const float *y, const float *W, const float *bias,
                   const int64_t *labels, float *pooled, float *logits, float *lossv, float *loss,
                   void *stream);
int stgcn_head_bwd(const stgcn_head_desc_t *d, const float *pooled, const float *logits,
                   const float *W, const int64_t *labels, const float *dloss, float *dlogits,
                   float *dpooled, float *dy, float *dW, float *dbias, void *stream);
/* ABI 10: stgcn_head_bwd with the gradient of y as its per-(n, c) value only:
 * dy_nc (N, C) = dpooled / L, the value stgcn_head_bwd writes to every one of
 * the L positions of row (n, c) -- for stgcn_bwd_args_t.dy_nc (no (N, C, L)
 * tensor written or read). */
int stgcn_head_bwd_nc(const stgcn_head_desc_t *d, const float *pooled, const float *logits,
                      const float *W, const int64_t *labels, const float *dloss, float *dlogits,
                      float *dpooled, float *dy_nc, float *dW, float *dbias, void *stream);
/* ABI 9: stgcn_head_fwd with the last block's output never written: the pool
 * reads that block's pre-BN2 tensor U (N, C, L) and forms y = ReLU(BN2(U)) on
 * load with the block's stats2 = [mean2 (C) | invstd2 (C)] (its stats buffer
 * from C_in * 2 on) and BN2 affine g2 / b2, as the block's output pass would
 * (bit-identical pooled). The block runs with stgcn_fwd_args_t.y and .y_stats
 * both null (training, non-residual, no dropout: no output pass at all).
 * stgcn_head_bwd is unchanged (its dy is the gradient of that unwritten y). */
int stgcn_head_fwd_u(const stgcn_head_desc_t *d, const float *U, const float *stats2,
                     const float *g2, const float *b2, const float *W, const float *bias,
                     const int64_t *labels, float *pooled, float *logits, float *lossv,
                     float *loss, void *stream);

/* STGCN_FEATURE_EVAL_HEAD: the head of an evaluation step (validation_step /
 * test_step, lightning_model.py:213-253: cross entropy and compute_accuracy
 * :114-121; compute_conf_mat :123-133) with the epoch's metrics accumulated on
 * the device: no host read per batch, so the step can be captured in a HIP graph.
 * logits, lossv and loss are bit-identical to stgcn_head_fwd / stgcn_head_fwd_u
 * when every label is valid. pred (N, int32) is the lowest index attaining the
 * maximum logit. A label outside [0, classes) is cross entropy's ignore_index:
 * lossv[n] = 0, the clip enters no count or sum but word 4, loss is the mean over
 * the valid clips (0 without one). Clip n is a top-k hit iff fewer than topk
 * classes j have logit_j > logit_label, or logit_j == logit_label with j < label
 * (1 <= topk <= classes).
 * The metrics block (may be null): eight 8-byte words, then classes * classes
 * int64 confusion[label][pred] (confusion_matrix[i, j] += 1 of :131):
 *   0 int64 batches            4 int64 clips with a label outside [0, classes)
 *   1 int64 clips, valid label 5 double sum of per-clip losses
 *   2 int64 top-1 correct      6 double sum of batch-mean losses
 *   3 int64 top-k hits         7 double sum of batch accuracies
 * Words 6 and 7 over word 0 are validation_epoch_end's averages of the batch
 * means (:220-224, :241-246); words 5 and 2 over word 1 the per-clip averages.
 * Deterministic: integer counts, one fixed-order fp64 sum per batch, one add per
 * word. One stream at a time per block. classes: stgcn_head_fwd's limit. */
typedef struct stgcn_eval_desc {
  int32_t N, C, L, classes, topk;
} stgcn_eval_desc_t;
size_t stgcn_eval_metrics_bytes(int classes); /* 0: classes unsupported */
int stgcn_eval_metrics_reset(void *metrics, int classes, void *stream);
int stgcn_head_eval(const stgcn_eval_desc_t *d, const float *y, const float *W, const float *bias,
                    const int64_t *labels, float *pooled, float *logits, float *lossv,
                    float *loss, int32_t *pred, void *metrics, void *stream);
/* ... pooling y = ReLU(BN2(U)) from the last block's U, as stgcn_head_fwd_u does */
int stgcn_head_eval_u(const stgcn_eval_desc_t *d, const float *U, const float *stats2,
                      const float *g2, const float *b2, const float *W, const float *bias,
                      const int64_t *labels, float *pooled, float *logits, float *lossv,
                      float *loss, int32_t *pred, void *metrics, void *stream);

/* STGCN_FEATURE_HEAD_LOSS: stgcn_head_eval / _u with the options of
 * F.cross_entropy(weight=, label_smoothing=, ignore_index=), so that a
 * validation loss is the quantity a weighted or smoothed training loss is.
 * z the logits row of clip n, lse = logsumexp(z), J = classes, w = class_weight
 * (device float (classes), 4-byte aligned; all ones when null), eps =
 * label_smoothing; a label outside [0, J) is ignored, as in stgcn_head_eval
 * (torch's -100 is one):
 *   lossv[n] = (1 - eps) w[y] (lse - z[y]) + (eps / J) sum_j w[j] (lse - z[j])
 *              for a valid clip, 0 for an ignored one
 *   denom[0] = D = the sum of w[y_n] over the valid clips (smoothing does not
 *              change it, as in torch), one float word in device memory
 *   loss[0]  = (sum_n lossv[n]) / D
 * Both sums in fp64 in clip order, the quotient rounded once to float. When D ==
 * 0 (no valid clip, or only labels of zero weight) loss = 0 where torch gives
 * NaN: deliberately, as stgcn_head_eval's "0 without one". pred, the top-k rule
 * and the metrics block (words 0-4, 7 and the matrix) are stgcn_head_eval's;
 * word 5 adds the sum of lossv, word 6 the loss as returned. With eps = 0, no
 * class_weight and any labels every output has stgcn_head_eval's bits.
 * No float atomics: the same inputs give the same bits.
 * flags: STGCN_LOSS_WEIGHT iff class_weight is given (a mismatch is refused).
 * stgcn_loss_check (host only) refuses a null descriptor, non-positive sizes,
 * topk outside [1, classes], unknown flags, label_smoothing outside [0, 1] or
 * not finite (STGCN_E_INVALID) and C + classes beyond the head's LDS limit
 * (STGCN_E_UNSUPPORTED), with the reason in stgcn_last_error. */
#define STGCN_LOSS_WEIGHT 1
typedef struct stgcn_loss_desc {
  int32_t N, C, L, classes, topk, flags;
  double label_smoothing;
} stgcn_loss_desc_t;
int stgcn_loss_check(const stgcn_loss_desc_t *d);
int stgcn_head_eval_loss(const stgcn_loss_desc_t *d, const float *y, const float *W,
                         const float *bias, const float *class_weight, const int64_t *labels,
                         float *pooled, float *logits, float *lossv, float *denom, float *loss,
                         int32_t *pred, void *metrics, void *stream);
/* ... pooling y = ReLU(BN2(U)) from the last block's U, as stgcn_head_eval_u does */
int stgcn_head_eval_loss_u(const stgcn_loss_desc_t *d, const float *U, const float *stats2,
                           const float *g2, const float *b2, const float *W, const float *bias,
                           const float *class_weight, const int64_t *labels, float *pooled,
                           float *logits, float *lossv, float *denom, float *loss, int32_t *pred,
                           void *metrics, void *stream);

/* Multi-tensor Adam (torch.optim.Adam, amsgrad=False, maximize=False;
 * lightning_model.py:196-197): ONE launch updates every tensor of a table.
 * stgcn_adam_build_table fills a HOST buffer (stgcn_adam_table_bytes; pinned
 * memory, so the caller can copy it to the device asynchronously) with the
 * tensor list and its chunk prefix sums and returns the chunk count;
 * stgcn_adam_step reads the DEVICE copy, with the 1-based step count; the
 * hyper-parameters are doubles (Python floats): 1 - beta and the bias
 * corrections are formed in double and rounded to float, as torch does. */
typedef struct stgcn_adam_tensor {
  float *param;
  const float *grad;
  float *exp_avg;
  float *exp_avg_sq;
  int64_t numel;
} stgcn_adam_tensor_t;

size_t stgcn_adam_table_bytes(int ntensors);
int stgcn_adam_build_table(const stgcn_adam_tensor_t *tensors, int ntensors, void *host_table,
                           size_t table_bytes, int64_t *total_chunks);
int stgcn_adam_step(const void *dev_table, int ntensors, int64_t total_chunks, double lr,
                    double beta1, double beta2, double eps, double weight_decay, int64_t step,
                    void *stream);
/* ABI 11: the same update with the step count in DEVICE memory (a float, as
 * torch.optim.Adam(capturable=True) keeps it): *step += 1 on the stream, then
 * the update with the bias corrections formed on the device from the new count
 * (in double, rounded to float: the values stgcn_adam_step forms on the host).
 * No host value changes between steps, so the launch can be captured once in a
 * HIP graph and replayed every training step (train_ops.FusedAdam
 * (capturable=True), train_ops.GraphedStep). Replaces the host-step launch of
 * stgcn_adam_step (torch optim/adam.py _multi_tensor_adam, capturable branch). */
int stgcn_adam_step_dev(const void *dev_table, int ntensors, int64_t total_chunks, double lr,
                        double beta1, double beta2, double eps, double weight_decay, float *step,
                        void *stream);
/* STGCN_FEATURE_STEP_STATE: stgcn_adam_step_dev with the learning rate read from
 * device memory when the kernel runs (lr_dev, a float: a scheduler writes it
 * between replays of a captured step; -lr / bc1 is formed as (float)(-((double)
 * *lr_dev / bc1))), and an optional gradient scale grad_coef (a device float, or
 * null): g = grad * *grad_coef before the weight-decay term, which is where
 * torch.nn.utils.clip_grad_norm_ before step() puts it. The gradients themselves
 * are not rewritten. */
int stgcn_adam_step_dev2(const void *dev_table, int ntensors, int64_t total_chunks,
                         const float *lr_dev, const float *grad_coef, double beta1, double beta2,
                         double eps, double weight_decay, float *step, void *stream);
/* The 2-norm of every gradient of an Adam table and the clip coefficient of
 * clip_grad_norm_: one fp64 sum of squares per table chunk into partials
 * (stgcn_grad_norm_bytes(total_chunks) bytes, plain stores), then one workgroup
 * adds the partials in a fixed order and writes *norm_out = (float)sqrt(sum) and
 * *coef_out = min(1, max_norm / (*norm_out + 1e-6)) in float. No atomics: the
 * same gradients give the same bits. (One norm over several parameter groups:
 * a table of all their tensors; only grad and numel of each entry are read.) */
size_t stgcn_grad_norm_bytes(int64_t total_chunks);
int stgcn_grad_norm(const void *dev_table, int ntensors, int64_t total_chunks, double max_norm,
                    double *partials, float *norm_out, float *coef_out, void *stream);

/* ---------------------------------------------------------------------------
 * STGCN_FEATURE_OPTIMIZERS: the Adam family with decoupled weight decay
 * (torch.optim.AdamW) and AMSGrad, one launch per table as stgcn_adam_step
 * (2048 elements per 256-thread block). maximize is not offered.
 *
 * stgcn_adam_step's arithmetic (s0 = exp_avg, s1 = exp_avg_sq; every operation
 * rounded on its own), with
 *   STGCN_OPT_DECOUPLED_WD: p = p * (float)(1.0 - lr * wd) ahead of the moment
 *     updates and g left alone (lr the double, or (double)*lr_dev), wd != 0;
 *   STGCN_OPT_AMSGRAD: vmax = max(vmax, v) (s2 = max_exp_avg_sq) and the
 *     denominator takes sqrt(vmax).
 * The three launch forms of stgcn_adam_step / _dev / _dev2 in one call: the step
 * count is `step` (host, 1-based) or, with step_dev, a device float advanced by
 * the call (*step_dev += 1 on the stream); the learning rate is `lr` or, with
 * lr_dev, a device float read when the kernel runs; grad_coef (optional) scales
 * the gradient, g = grad * *grad_coef, ahead of the weight-decay term. With
 * neither flag the call gives stgcn_adam_step's bits.
 *
 * Alignment: the device table 8 bytes; param, grad, s0, s1, s2, lr_dev,
 * grad_coef and step_dev 4 (views into a flat bucket work in place). */
#define STGCN_OPT_ADAM 1 /* stgcn_opt_desc_t.algo (the only one so far) */
/* stgcn_opt_desc_t.flags */
#define STGCN_OPT_DECOUPLED_WD 2
#define STGCN_OPT_AMSGRAD 4

typedef struct stgcn_opt_tensor {
  float *param;
  const float *grad;
  float *s0, *s1, *s2; /* exp_avg, exp_avg_sq, max_exp_avg_sq (null without AMSGrad) */
  int64_t numel;
  int32_t flags;       /* 0 */
  int32_t reserved;    /* 0 */
} stgcn_opt_tensor_t;

typedef struct stgcn_opt_desc {
  int32_t algo;          /* STGCN_OPT_ADAM                                      */
  int32_t flags;
  double lr;             /* ignored with lr_dev                                 */
  double beta1, beta2, eps, weight_decay;
  int64_t step;          /* without step_dev: the 1-based step count            */
  const float *lr_dev;   /* optional device float: the learning rate            */
  const float *grad_coef; /* optional device float: g = grad * *grad_coef       */
  float *step_dev;       /* optional: the device step count                     */
} stgcn_opt_desc_t;

/* Validates a descriptor on the host (0 = accepted); stgcn_last_error names what
 * is refused: an unknown algo or flag, a negative lr / weight decay / eps, betas
 * outside [0, 1), a step < 1 without step_dev, a misaligned device word. */
int stgcn_opt_check(const stgcn_opt_desc_t *d);
size_t stgcn_opt_table_bytes(int ntensors);
/* Fills a HOST buffer (pinned, copied to the device by the caller) with the
 * tensor list and its chunk prefix sums, as stgcn_adam_build_table does. d says
 * which state slots must be non-null (s0, s1, and s2 with STGCN_OPT_AMSGRAD). */
int stgcn_opt_build_table(const stgcn_opt_desc_t *d, const stgcn_opt_tensor_t *tensors,
                          int ntensors, void *host_table, size_t table_bytes,
                          int64_t *total_chunks);
int stgcn_opt_step(const stgcn_opt_desc_t *d, const void *dev_table, int ntensors,
                   int64_t total_chunks, void *stream);

/* ---------------------------------------------------------------------------
 * STGCN_FEATURE_INPUT_STAGE: the host input pipeline of the reference (loop
 * padding src/data/util.py:12-47, augmentation src/data/augmentation.py:8-69
 * drawn per clip as KTHDataset.__getitem__ does, datasets.py:154, the fp32
 * cast and the NTVC -> NCTV permute of lightning_model.py:101) as one launch.
 *
 * src holds src_frames frames back to back, each V * C_src elements, joint
 * major and channel fastest (the .npy layout (T, V, C_src)), fp32 or fp64.
 * clips is a DEVICE table of N entries, read when the kernel runs (a captured
 * launch sees the table's contents at each replay). For every (n, t, v),
 *   frame = clips[n].first_frame + (t mod clips[n].frames)
 * (np.pad "wrap"; a clip of T_out frames or more gives its first T_out),
 *   x[n, j, t, v] = src[frame, v, 0] * m[0][j] + src[frame, v, 1] * m[1][j]
 * for j = 0, 1 when flags bit 0 is set: in fp64 whatever the source type, as one
 * product and one fused multiply-add, fma(src[.., 0], m[0][j], src[.., 1] *
 * m[1][j]) (what the kernel has always computed; within 2^-52 relative of each
 * term of the unfused form), rounded once to fp32; m is the upper
 * left 2x2 of the reference's 3x3 matrix (its third homogeneous coordinate is
 * 0: translations do not move points). Without the bit channels 0 and 1 are
 * cast like channels 2 .. C - 1: bit-exact, non-finite values included.
 * An entry with frames < 1, first_frame < 0 or first_frame + frames >
 * src_frames is invalid: its clip is written as zeros, status[n] = 1, and src
 * is not read for it. status[n] = 0 otherwise; every launch writes all N words
 * with plain stores (no atomics, nothing to reset between replays).
 * Alignment: x 16 bytes, src its element's 4 or 8, clips 8, status 4. One
 * launch on the caller's stream; nothing is allocated. */
typedef struct stgcn_input_desc {
  int32_t N, C, T_out, V; /* x (N, C, T_out, V) fp32                            */
  int32_t C_src;          /* source channels per joint, C <= C_src <= 4, C >= 2 */
  int32_t src_f64;        /* 0: fp32 source, 1: fp64                            */
  int64_t src_frames;     /* capacity of src in frames                          */
} stgcn_input_desc_t;
typedef struct stgcn_clip { /* 48 bytes, device memory, N of them               */
  int64_t first_frame;
  int32_t frames;
  int32_t flags;            /* bit 0: apply m                                   */
  double m[4];              /* row-major 2x2, out_j = x m[0][j] + y m[1][j]     */
} stgcn_clip_t;
/* Validates a descriptor on the host (0 = supported; T_out * V and the launch
 * grid must fit 31 bits). */
int stgcn_input_check(const stgcn_input_desc_t *d);
int stgcn_input_stage(const stgcn_input_desc_t *d, const void *src, const stgcn_clip_t *clips,
                      float *x, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------
 * STGCN_FEATURE_INPUT_MOVE: stgcn_input_stage with ST-GCN's "random moving"
 * (the training augmentation of the ST-GCN recipe, feeder/tools.py random_move;
 * the TODO of src/data/augmentation.py:48): rotation angle, scale and
 * translation given at up to 4 key frames, interpolated linearly over the
 * output frames and applied per frame, after the clip's own 2x2 matrix.
 * Unlike that matrix (src/data/augmentation.py:56-59 multiplies [x, y, 0], so
 * the reference drops its translations, and stgcn_clip_t keeps doing so), the
 * translation here moves the points.
 *
 * moves is a DEVICE table of N records, read when the kernel runs, like clips.
 * For output frame t of clip n in segment k (frame[k] <= t < frame[k + 1]; a
 * last frame t == frame[nk - 1] belongs to the last segment) each of angle,
 * scale, tx, ty is
 *   p(t) = p[k] + (double)(t - frame[k]) *
 *                 ((p[k + 1] - p[k]) / (double)(frame[k + 1] - frame[k]))
 * and with c = cos(a) * s, sn = sin(a) * s and (x, y) the point after the
 * clip's matrix (kept in fp64; the plain source values without the flag)
 *   x[n, 0, t, v] = (c * x - sn * y) + tx
 *   x[n, 1, t, v] = (sn * x + c * y) + ty
 * all in fp64, every operation rounded on its own (no fused multiply-add), one
 * rounding to fp32 at the end. Channels 2 .. C - 1 are cast as before.
 * nk == 0: no move, the clip takes stgcn_input_stage's path and has its bits.
 * A record is invalid when nk is not 0, 2, 3 or 4, frame[0] != 0, the first nk
 * frames do not strictly increase, frame[nk - 1] < T_out - 1, or one of the
 * first nk values of angle, scale, tx, ty is not finite: the clip is written as
 * zeros without reading src, and status[n] has bit 1 set. status[n] =
 * (invalid clip entry ? 1 : 0) | (invalid move record ? 2 : 0), written for
 * every clip at every launch with plain stores.
 * moves == NULL: the call is stgcn_input_stage. Alignment: moves 8 bytes, the
 * rest as stgcn_input_stage. */
typedef struct stgcn_move { /* 160 bytes, device memory, N of them              */
  int32_t nk;               /* key frames: 0 (no move) or 2..4                  */
  int32_t frame[4];         /* frame[0] = 0 < ... < frame[nk - 1] >= T_out - 1  */
  int32_t reserved0;
  double angle[4];          /* radians                                          */
  double scale[4];
  double tx[4], ty[4];
  int64_t reserved1;
} stgcn_move_t;
/* stgcn_input_check for the move launch (the same limits). */
int stgcn_input_move_check(const stgcn_input_desc_t *d);
int stgcn_input_stage_move(const stgcn_input_desc_t *d, const void *src,
                           const stgcn_clip_t *clips, const stgcn_move_t *moves, float *x,
                           int32_t *status, void *stream);

/* ---------------------------------------------------------------------------
 * STGCN_FEATURE_INPUT_STREAMS: the input views the ST-GCN descendants train on
 * (2s-AGCN, ST-GCN++, the PYSKL recipes), formed by the input stage's launch
 * from the augmented point, so after the clip's matrix and its move: a bone of
 * the moved skeleton is not the moved bone of the original.
 *
 * x is (N, S * in.C, T_out, V) fp32, written in full; the selected streams come
 * in bit order (joint, bone, joint motion, bone motion), in.C consecutive
 * channels each. Let J[c, t, v] be the fp32 value stgcn_input_stage_move writes
 * for the same src, clips and moves (stgcn_input_stage with moves == NULL): the
 * kernel forms it with that launch's own operations, so with its bits. With
 * p = parents[v], in fp32, every operation rounded on its own:
 *   B [c, t, v] = J[c, t, v] - J[c, t, p]             (p == v, a root: +0)
 *   JM[c, t, v] = J[c, t + 1, v] - J[c, t, v]         t < T_out - 1, else 0
 *   BM[c, t, v] = B[c, t + 1, v] - B[c, t, v]         t < T_out - 1, else 0
 * and on the score channel c == score_channel (a confidence, not a coordinate)
 * the mean instead of the difference:
 *   B = (J[c, t, v] + J[c, t, p]) * 0.5f,  JM = (J[c, t + 1, v] + J[c, t, v]) * 0.5f,
 *   BM = (B[c, t + 1, v] + B[c, t, v]) * 0.5f, the last frame of JM and BM 0 too.
 * Frame t + 1 is the loop-padded frame first_frame + ((t + 1) mod frames): the
 * seam of a wrapped clip gives a real difference, as on the padded array.
 *
 * parents is a DEVICE table of V int32 entries, read when the kernel runs, like
 * clips; it may be NULL without a bone bit. An entry outside [0, V) is invalid:
 * every clip is written as zeros without reading src, and every status[n] has
 * bit 2 (value 4) set beside the unchanged bits 0 and 1; every launch writes
 * all N words with plain stores.
 * stgcn_input_streams_check: STGCN_E_INVALID for an empty mask, unknown bits or
 * a score_channel other than -1 or in.C - 1 >= 2; STGCN_E_UNSUPPORTED for
 * V > 256 with a bone bit and for an x of N * S * C * T_out * V elements beyond
 * the kernel's int64 offsets (the limits of stgcn_input_check hold and are the
 * tighter ones today). streams ==
 * STGCN_STREAM_JOINT is the stgcn_input_stage_move launch itself.
 * Alignment: parents 4 bytes, the rest as stgcn_input_stage_move. */
#define STGCN_STREAM_JOINT        1
#define STGCN_STREAM_BONE         2
#define STGCN_STREAM_JOINT_MOTION 4
#define STGCN_STREAM_BONE_MOTION  8
typedef struct stgcn_streams_desc {
  stgcn_input_desc_t in;   /* as for stgcn_input_stage; in.C channels per stream     */
  int32_t streams;         /* non-empty subset of the four bits; S = popcount        */
  int32_t score_channel;   /* -1, or in.C - 1 (>= 2): that channel is a confidence   */
} stgcn_streams_desc_t;    /* 40 bytes                                               */
int stgcn_input_streams_check(const stgcn_streams_desc_t *d);
int stgcn_input_stage_streams(const stgcn_streams_desc_t *d, const void *src,
                              const stgcn_clip_t *clips, const stgcn_move_t *moves,
                              const int32_t *parents, float *x, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* STGCN_HIP_H */
