// C-ABI entry points of libstgcn_hip.so (declared in include/stgcn_hip.h).
//
// stgcn_block_fwd / stgcn_block_bwd enqueue the kernel sequence of one
// ST-GCN block on the caller's stream (the fused folded backward: its small
// kernels on a side stream forked from and joined to it, BwdCtx::fk). The
// reference op order of the default
// (non-residual) block
// (st_graphconv.py:97-109, :148-150) is
//     BN1 -> Y = W x + b -> Z = sum_k Y_k A_k^T -> Conv9x1 -> BN2 -> ReLU;
// here the joint contraction is applied on the narrower (input-channel) side,
//     Z = sum_k W_k (BN1(x) A_k^T) + (sum_k b_k rowsum(A_k))          (1)
// which is the same linear map (exact in real arithmetic) and never
// materialises the K*C_out-channel Y. The residual block (st_graphconv.py:60-82)
// reuses the same kernels: ReLU folded into the joint contraction's BN1
// input, BN2 statistics from the spatial GEMM epilogue, and the residual add +
// final ReLU in the temporal conv's epilogue.
//
// Paths, workspace layouts and GEMM launch parameters are planned in block_plan.h;
// here: error handling, argument checks, the entry points and their stages.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/stgcn_hip.h"
#include "host_common.h"
#include "internal.h"
#include "block_plan.h"

using namespace stgcn;

namespace {
thread_local std::string g_err;
}  // namespace

namespace stgcn {
void set_last_error(const std::string &msg) { g_err = msg; }
}  // namespace stgcn

namespace {

// a stage of an entry point: its status ends the call
#define STAGE(expr) \
  do { if (int rc_ = (expr)) return rc_; } while (0)

#define STGCN_P(s, m) NamedPtr{(s)->m, #m}

// bytes of a y_stats / x_stats block (ABI 7): 5 * C doubles of sums, then the
// max |y| words (block_amax slots)
size_t y_stats_bytes(int C) {
  return sizeof(double) * 5 * C + sizeof(unsigned) * STGCN_STATS_AMAX_WORDS;
}
static_assert(STGCN_STATS_AMAX_WORDS == kAmaxWords, "ABI 7: the amax block of y_stats");

// the fused dropout of a call (training and 0 < p < 1; p >= 1: everything dropped)
// (seed_dev: the step token of the _dseed entry points, internal.h Dropout)
Dropout make_dropout(const stgcn_desc_t *d, float p, uint64_t seed, const uint64_t *seed_dev) {
  Dropout dr;
  if (!d->training || !(p > 0.f)) return dr;
  dr.seed = seed;
  dr.seed_dev = seed_dev;
  const double t = (double)p * 4294967296.0;
  dr.thresh = t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
  dr.scale = p < 1.f ? (float)(1.0 / (1.0 - (double)p)) : 0.f;
  return dr;
}

}  // namespace

extern "C" {

int stgcn_abi_version(void) { return STGCN_ABI_VERSION; }

const char *stgcn_last_error(void) { return g_err.c_str(); }

int stgcn_check_desc(const stgcn_desc_t *d) {
  if (!d) return fail(STGCN_E_INVALID, "null descriptor");
  if (d->N <= 0 || d->C_in <= 0 || d->C_out <= 0 || d->T <= 0 || d->V <= 0 || d->K <= 0)
    return fail(STGCN_E_INVALID, "non-positive dimension");
  if ((d->flags & ~(STGCN_F_RESIDUAL | STGCN_F_BF16 | STGCN_F_F32X3 | STGCN_F_F16X2 |
                    STGCN_F_NO_G)) != 0)
    return fail(STGCN_E_UNSUPPORTED, "unknown flags");
  if ((d->flags & STGCN_F_NO_G) && !(d->flags & STGCN_F_F16X2))
    return fail(STGCN_E_INVALID, "STGCN_F_NO_G needs STGCN_F_F16X2");
  if ((d->flags & STGCN_F_BF16) && (d->flags & STGCN_F_F32X3))
    return fail(STGCN_E_INVALID, "STGCN_F_BF16 and STGCN_F_F32X3 are exclusive");
  if ((d->flags & STGCN_F_F16X2) && !(d->flags & STGCN_F_F32X3))
    return fail(STGCN_E_INVALID, "STGCN_F_F16X2 needs STGCN_F_F32X3");
  if (d->gamma != 9 || d->pad != 4)
    return fail(STGCN_E_UNSUPPORTED, "only gamma=9, pad=4 (the reference default)");
  if (d->stride != 1 && d->stride != 2) return fail(STGCN_E_UNSUPPORTED, "stride must be 1 or 2");
  if (d->T_out != (d->T + 2 * d->pad - d->gamma) / d->stride + 1)
    return fail(STGCN_E_INVALID, "T_out inconsistent with T, stride, pad");
  if (d->V > kTileCols) return fail(STGCN_E_UNSUPPORTED, "V > 256");
  if (d->K * d->V * d->V > 8192) return fail(STGCN_E_UNSUPPORTED, "K*V*V > 8192");
  if ((int64_t)d->N * d->K * d->C_in * d->T * d->V > INT32_MAX ||
      (int64_t)d->N * d->C_out * d->T * d->V > INT32_MAX)
    return fail(STGCN_E_UNSUPPORTED, "tensor too large for 32-bit element indexing");
  if (!geometry_supported(d))
    return fail(STGCN_E_UNSUPPORTED, "tile geometry exceeds LDS for this V / channel count");
  return STGCN_OK;
}

int stgcn_block_plan(const stgcn_desc_t *d, uint32_t *plan) {
  int rc = stgcn_check_desc(d);
  if (rc) return rc;
  if (!plan) return fail(STGCN_E_INVALID, "null plan pointer");
  uint32_t f = 0;
  if (fold_w(d)) f |= STGCN_PLAN_FOLD;
  if (fused_sp(d)) f |= STGCN_PLAN_SP_FWD_FUSED;
  if (fused_spb(d) || fold_spb(d)) f |= STGCN_PLAN_SP_BWD_FUSED;
  if (act_bf16(d)) f |= STGCN_PLAN_ACT_BF16;
  if (!fold_w(d) && !fused_sp(d)) {  // the spatial dW' GEMM of the unfolded block
    WgradParams w = wgrad_spatial(d, nullptr, nullptr, nullptr);
    if (w.bf16 == 3) f |= STGCN_PLAN_WSP_SPLIT;
  }
  if (f32x3(d)) {
    const int Cred = fold_w(d) ? d->C_in : d->C_out;  // (the temporal conv forward's reduction)
    if (conv_x3_supported(tconv_fwd(d, Cred, nullptr, nullptr, nullptr, nullptr)))
      f |= STGCN_PLAN_TCONV_SPLIT;
    WgradParams w = make_wgrad_taps(d, nullptr, nullptr, nullptr, fold_w(d) ? d->C_in : 0);
    if (w.bf16 == 3) f |= STGCN_PLAN_TWGRAD_SPLIT;
  }
  if (f16x2_tw(d)) f |= STGCN_PLAN_F16X2;
  if (fold_bna(d)) f |= STGCN_PLAN_FOLD_NO_G;
  if (x_from_u(d)) f |= STGCN_PLAN_X_FROM_U;
  if (x_from_u_eval(d)) f |= STGCN_PLAN_X_FROM_U_EVAL;
  *plan = f;
  return STGCN_OK;
}

size_t stgcn_fwd_workspace_bytes(const stgcn_desc_t *d) {
  if (stgcn_check_desc(d) != STGCN_OK) return 0;
  return fwd_layout(d, nullptr).total;
}

size_t stgcn_keep_g_bytes(const stgcn_desc_t *d) {
  if (stgcn_check_desc(d) != STGCN_OK) return 0;
  if (fused_sp(d)) return sp_keep_g_bytes(d->N, d->C_in, d->T, d->V, d->K);
  // (no G: only the forward's max |x| for the backward's weight gradient)
  if (fold_bna(d)) return sizeof(unsigned) * kAmaxWords;
  // (f16x2: + one word after G, its max |G| for the backward's weight gradient)
  return sizeof(float) * (size_t)d->N * d->K * d->C_in * d->T * d->V +
         (f16x2_tw(d) ? sizeof(unsigned) * kAmaxWords : 0);
}

size_t stgcn_fold_prep_bytes(const stgcn_desc_t *d) {
  if (stgcn_check_desc(d) != STGCN_OK || !prep_applies(d)) return 0;
  return prep_layout(d, nullptr).total;
}

int stgcn_fold_prep(int nblocks, const stgcn_desc_t *descs, const stgcn_fold_weights_t *weights,
                    void *const *prep, void *stream) {
  if (nblocks < 0 || (nblocks > 0 && (!descs || !weights || !prep)))
    return fail(STGCN_E_INVALID, "null fold_prep argument");
  std::vector<FoldPrepSpec> sp;
  std::vector<PackJob> pk;
  for (int i = 0; i < nblocks; ++i) {
    const stgcn_desc_t *d = descs + i;
    int rc = stgcn_check_desc(d);
    if (rc) return rc;
    if (!prep_applies(d)) continue;  // (stgcn_fold_prep_bytes == 0: not a folded block)
    const stgcn_fold_weights_t &w = weights[i];
    if (!prep[i] || !w.A || !w.W || !w.bW || !w.Wt || !w.bWt)
      return fail(STGCN_E_INVALID, "null fold_prep weights / buffer of a folded block");
    if ((rc = check_aligned({NamedPtr{w.A, "A"}, NamedPtr{w.W, "W"}, NamedPtr{w.bW, "bW"},
                             NamedPtr{w.Wt, "Wt"}, NamedPtr{w.bWt, "bWt"},
                             NamedPtr{prep[i], "prep"}},
                            16)))
      return rc;
    const PrepLayout P = prep_layout(d, prep[i]);
    FoldPrepSpec b{};
    b.A = w.A;
    b.W = w.W;
    b.bW = w.bW;
    b.Wt = w.Wt;
    b.bWt = w.bWt;
    b.R = d->C_out;
    b.C = d->C_in;
    b.V = d->V;
    b.T = d->T;
    b.To = d->T_out;
    b.stride = d->stride;
    b.bZ = P.bZ;
    b.Wc = P.Wc;
    b.BT = P.BT;
    b.fscr_f = P.fscr_f;
    b.fscr_b = P.fscr_b;
    b.bq = P.bq;
    b.f64 = P.f64;
    b.amax = P.amax;
    sp.push_back(b);
    // the split-plane packs of the forward and data-gradient GEMMs (with max |Wc|)
    ConvGemmParams f =
        tconv_fwd(d, d->C_in, nullptr, P.Wc, nullptr, reinterpret_cast<float *>(P.wpk_f));
    f.amax_w = P.amax;
    pk.push_back(conv_x3_pack_job(f, fold_fwd_npl(d)));
    for (int ph = 0; ph < tconv_dgrad_phases(d); ++ph) {
      ConvGemmParams g = tconv_dgrad(d, d->C_in, ph, nullptr, P.Wc, nullptr,
                                     reinterpret_cast<float *>(P.wpk_d[ph]));
      g.amax_w = P.amax;
      pk.push_back(conv_x3_pack_job(g, fold_dgrad_npl(d)));
    }
  }
  if (sp.empty()) return STGCN_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(launch_fold_prep(sp.data(), (int)sp.size(), s));
  HIP_TRY(launch_pack_jobs(pk.data(), (int)pk.size(), s));
  return STGCN_OK;
}

size_t stgcn_bwd_workspace_bytes(const stgcn_desc_t *d) {
  if (stgcn_check_desc(d) != STGCN_OK) return 0;
  return bwd_layout(d, nullptr).total;
}

}  // extern "C"

// ---- stgcn_block_fwd in stages ----
namespace {

struct FwdCtx {
  const stgcn_desc_t *d;
  const stgcn_fwd_args_t *a;
  FwdLayout L;
  hipStream_t s;
  bool res;         // residual block
  bool xu;          // ABI 8: x from the previous block's U (STGCN_PLAN_X_FROM_U)
  bool fold, bna;   // the folded block (G only; W' rides on the temporal conv's weights); no G
  bool pre;         // ABI 7: the folded block's weight-only operands from stgcn_fold_prep
  PrepLayout P;
  bool stat_parts;  // the folded forward on k_conv_x3: BN2 statistics as per-tile partials
  bool no_memset;
  float *st1, *st2;  // [mean | invstd] of BN1 / BN2 in a->stats (the finalize kernels' output)
  BnRef bn1, bn2;    // ... with gamma and beta, as the kernels read them
  const unsigned *xmax = nullptr;  // (bna: max |x|, the fp16 operand bound's input)
  const uint64_t *seed_dev = nullptr;  // the dropout's step token (stgcn_block_fwd_dseed)
  const float *Gfold = nullptr;    // the folded block's G (spatial stage -> temporal stage)
};

int fwd_check_args(const stgcn_desc_t *d, const stgcn_fwd_args_t *a, void *workspace) {
  int rc;
  const bool res = residual(d);
  // ABI 8: x from the previous block's U (STGCN_PLAN_X_FROM_U); y null: statistics only
  const bool xu = a && a->prev_U;
  const bool ystats_only = a && !a->y && a->y_stats && d->training && !res && a->dropout_p == 0.f;
  // ABI 9: y and y_stats both null: no output pass (stgcn_head_fwd_u pools from U)
  // (eval, non-residual: the same, U is the handoff -- dropout is inert there)
  const bool no_out = a && !a->y && !a->y_stats && !res &&
                      (d->training ? a->dropout_p == 0.f : true);
  if (!a || (!a->x && !xu) || !a->A || !a->W || !a->bW || !a->Wt || !a->bWt || !a->g1 ||
      !a->b1 || !a->g2 || !a->b2 || (!a->y && !ystats_only && !no_out) || !a->Z ||
      (!res && !a->U) ||
      !a->stats)
    return fail(STGCN_E_INVALID, "null tensor argument");
  if (res && (!a->Za || (projection(d) && (!a->Wr || !a->br))))
    return fail(STGCN_E_INVALID, "residual block: null Za / projection weights");
  if (!a->rm1 || !a->rv1 || !a->rm2 || !a->rv2)
    return fail(STGCN_E_INVALID, "null running-stat buffer");
  // (eval, STGCN_PLAN_X_FROM_U_EVAL: BN1 takes the running statistics, no x_stats)
  if (xu && (!(x_from_u(d) || x_from_u_eval(d)) || (d->training && !a->x_stats) ||
             !a->prev_stats || !a->prev_g2 || !a->prev_b2 ||
             ((uintptr_t)a->prev_U & 15) != 0))
    return fail(STGCN_E_INVALID,
                "prev_U input: needs STGCN_PLAN_X_FROM_U, x_stats, prev_stats / prev_g2 / "
                "prev_b2 and a 16-byte aligned prev_U");
  // the alignment contract (stgcn_hip.h): 16 bytes, but 4 for the running
  // statistics (updated in place by scalar accesses, k_bn_finalize[_parts]) and
  // for prev_stats (the previous block's stats + 2 * C_in_prev by construction)
  if ((rc = check_aligned(
           {STGCN_P(a, x), STGCN_P(a, A), STGCN_P(a, W), STGCN_P(a, bW), STGCN_P(a, Wt),
            STGCN_P(a, bWt), STGCN_P(a, g1), STGCN_P(a, b1), STGCN_P(a, g2), STGCN_P(a, b2),
            STGCN_P(a, y), STGCN_P(a, Z), NamedPtr{res ? nullptr : a->U, "U"}, STGCN_P(a, stats),
            STGCN_P(a, Wr), STGCN_P(a, br), STGCN_P(a, Za), STGCN_P(a, G), STGCN_P(a, x_stats),
            STGCN_P(a, y_stats), STGCN_P(a, prep), STGCN_P(a, prev_U), STGCN_P(a, prev_g2),
            STGCN_P(a, prev_b2), NamedPtr{workspace, "workspace"}},
           16)) ||
      (rc = check_aligned({STGCN_P(a, rm1), STGCN_P(a, rv1), STGCN_P(a, rm2), STGCN_P(a, rv2),
                           STGCN_P(a, prev_stats)},
                          4)))
    return rc;
  return STGCN_OK;
}

// BN1 statistics of the block input (st_graphconv.py:98)
// (the caller may hand over the previous block's y statistics: x_stats)
int fwd_bn1_stats(FwdCtx &c, void *workspace) {
  const stgcn_desc_t *d = c.d;
  const stgcn_fwd_args_t *a = c.a;
  const FwdLayout &L = c.L;
  hipStream_t s = c.s;
  const int N = d->N, C = d->C_in, T = d->T, V = d->V;
  // (folded training forward with the previous block's statistics: nothing in the
  // workspace's fp64 area accumulates -- BN2 goes to per-tile partials -- except
  // the f16x2 max |G| / |Wc| words, which the BN1 finalize zeroes: no memset)
  if (!c.no_memset) HIP_TRY(hipMemsetAsync(workspace, 0, L.dbl_bytes, s));
  const double *xs1 = L.s1, *xq1 = L.q1;
  c.xmax = L.amax;
  if (d->training && a->x_stats) {
    xs1 = a->x_stats;
    xq1 = a->x_stats + C;
    c.xmax = reinterpret_cast<const unsigned *>(a->x_stats + 5 * C);  // (ABI 7: after the sums)
  } else if (d->training) {
    HIP_TRY(launch_bn_stats(a->x, N, C, T * V, L.s1, L.q1, s, c.bna ? L.amax : nullptr));
  } else if (c.bna) {
    HIP_TRY(launch_absmax(a->x, (int64_t)N * C * T * V, L.amax, s));
  }
  HIP_TRY(launch_bn_finalize(xs1, xq1, C, (int64_t)N * T * V, d->eps, d->momentum, d->training,
                             a->rm1, a->rv1, c.st1, c.st1 + C, s,
                             c.no_memset ? L.amax : nullptr, c.no_memset ? 2 * kAmaxWords : 0));
  return STGCN_OK;
}

// Spatial graph conv (st_graphconv.py:139-152) in the form (1).
// (residual block: SpatialConv sees ReLU(BN1(x)), st_graphconv.py:72-74)
int fwd_spatial(FwdCtx &c) {
  const stgcn_desc_t *d = c.d;
  const stgcn_fwd_args_t *a = c.a;
  const FwdLayout &L = c.L;
  hipStream_t s = c.s;
  const int N = d->N, C = d->C_in, R = d->C_out, T = d->T, V = d->V, K = d->K;
  const bool res = c.res, xu = c.xu;
  if (!c.pre) HIP_TRY(launch_bias_rv(a->A, a->bW, L.biasZ, K, R, V, s));
  const float *Wz = a->W;
  if (K > 1) {
    HIP_TRY(launch_pack_w(a->W, L.Wpk, K, R, C, s));
    Wz = L.Wpk;
  }
  // (x = ReLU(BN2_prev(prev_U)) formed on staging / on load)
  SpatialFwd f = spatial_fwd(d, xu ? a->prev_U : a->x, c.bn1, a->A);
  if (xu) f.prev = prev_bn(a->prev_stats, C, a->prev_g2, a->prev_b2);
  if (fused_sp(d)) {
    // bf16 path: BN1 + joint contraction + W' GEMM in one kernel; G kept in bf16
    // for the backward when the caller asks (stgcn_keep_g_bytes)
    f.W = a->W;
    f.biasZ = L.biasZ;
    f.wpk = L.wpk;
    f.Z = a->Z;
    f.z_bf16 = z_bf16(d) ? 1 : 0;
    f.Gk = reinterpret_cast<__bf16 *>(a->G);
    if (res && d->training) {  // BN2 of the residual block normalizes Z (:76)
      f.ssum = L.s2;
      f.ssq = L.q2;
    }
    HIP_TRY(launch_sp_fwd_bf16(f, s));
  } else if (!c.bna) {
    f.G = a->G ? a->G : L.G;  // kept for the backward when the caller asks
    f.amax = f16x2(d) ? L.amax : nullptr;  // (f16x2: max |G|)
    HIP_TRY(launch_gather_fwd(f, s));
    c.Gfold = f.G;
    if (!c.fold) {
      ConvGemmParams p = spatial_gemm(d, f.G, Wz, a->Z, L.biasZ, L.wpk);
      if (res && d->training) {  // BN2 of the residual block normalizes Z (:76)
        p.stat_sum = L.s2;
        p.stat_sq = L.q2;
      }
      HIP_TRY(launch_conv_gemm(p, s));
      // (the unfolded fp16-split block: max |Z| for the temporal GEMMs' operand
      // scale, one pass over Z -- tracking it in the spatial GEMM's epilogue cost
      // that kernel 65 registers, half its occupancy)
      if (f16x2_unfold(d)) HIP_TRY(launch_absmax(a->Z, (int64_t)N * R * T * V, L.amax, s));
    }
  }
  return STGCN_OK;
}

// Residual block after the spatial conv (st_graphconv.py:75-80, :105):
//   Za = ReLU(BN2(Z)); y = ReLU(Conv9x1(Za) + bt + R(x)),
// R = x (identity) or Wr x + br with temporal stride (projection).
int residual_fwd_tail(FwdCtx &c) {
  const stgcn_desc_t *d = c.d;
  const stgcn_fwd_args_t *a = c.a;
  const FwdLayout &L = c.L;
  hipStream_t s = c.s;
  const int N = d->N, R = d->C_out, T = d->T, To = d->T_out, V = d->V;
  HIP_TRY(launch_bn_finalize(L.s2, L.q2, R, (int64_t)N * T * V, d->eps, d->momentum,
                             d->training, a->rm2, a->rv2, c.st2, c.st2 + R, s));
  HIP_TRY(launch_bn_relu_fwd(a->Z, c.bn2, a->Za, N, R, T * V, nullptr, nullptr, Dropout(), s));
  const float *resid = a->x;
  if (projection(d)) {  // apply_residual: Conv2d(C_in, C_out, 1, stride (s,1)) (:27)
    HIP_TRY(launch_conv_gemm(proj_fwd(d, a->x, a->Wr, L.Rp, a->br, L.wpk), s));
    resid = L.Rp;
  }
  ConvGemmParams p = tconv_fwd(d, R, a->Za, a->Wt, a->y, L.wpk);
  p.bias_r = a->bWt;
  p.res = resid;
  p.relu_out = 1;
  p.drop = make_dropout(d, a->dropout_p, a->seed, c.seed_dev);
  if (d->training && a->y_stats) {  // next block's BN1 statistics from the epilogue
    HIP_TRY(hipMemsetAsync(a->y_stats, 0, y_stats_bytes(R), s));
    p.stat_sum = a->y_stats;
    p.stat_sq = a->y_stats + R;
  }
  HIP_TRY(launch_conv_gemm(p, s));
  if (d->training && a->y_stats)  // (ABI 7: max y after the sums, the next block's bound)
    HIP_TRY(launch_absmax(a->y, (int64_t)N * R * To * V,
                          reinterpret_cast<unsigned *>(a->y_stats + 5 * R), s));
  return STGCN_OK;
}

// Temporal (9,1) conv, stride (s,1), pad (4,0), bias (st_graphconv.py:41-43,99),
// with the BN2 batch statistics accumulated in the epilogue.
int fwd_temporal(FwdCtx &c) {
  const stgcn_desc_t *d = c.d;
  const stgcn_fwd_args_t *a = c.a;
  const FwdLayout &L = c.L;
  const PrepLayout &P = c.P;
  hipStream_t s = c.s;
  const int N = d->N, C = d->C_in, R = d->C_out, T = d->T, To = d->T_out, V = d->V, K = d->K;
  ConvGemmParams p;
  if (c.fold) {  // U = sum_q Wc_q G[s t + q - 4] + BT[o, t, v]  (kernels_fold.hip)
    float *Wc = fold_wc_in_z(d) ? a->Z : L.Wc;  // (kept for the backward)
    const float *BT = L.BT;
    const unsigned *amax_wc = L.amax + kAmaxWords;
    if (c.pre) {  // (formed for the whole stack by stgcn_fold_prep)
      Wc = P.Wc;
      BT = P.BT;
      amax_wc = P.amax;
    } else {
      HIP_TRY(launch_fold_fwd(a->Wt, a->W, a->bWt, L.biasZ, R, C, V, T, To, d->stride, Wc, L.bq,
                              L.BT, L.fscr, s));
      if (f16x2(d)) HIP_TRY(launch_absmax(Wc, (int64_t)R * C * 9, L.amax + kAmaxWords, s));
    }
    p = tconv_fwd(d, C, c.Gfold, Wc, a->U, L.wpk);
    p.res = BT;
    p.res_shared = 1;
    if (c.pre) {
      p.wpk = reinterpret_cast<float *>(P.wpk_f);
      p.wpk_ready = 1;
    }
    if (f16x2(d)) {  // the fp16 splits' operand scales: max |G| (gather), max |Wc|
      p.f16x2 = 1;
      p.amax_in = L.amax;
      p.amax_w = amax_wc;
      if (a->G)  // (the kept G carries its bound to the backward)
        p.amax_keep = reinterpret_cast<unsigned *>(a->G + (size_t)N * C * T * V);
    }
    if (c.bna) {  // x in, BN1 in the loader, A in the epilogue (G never formed)
      p.in = a->x;
      p.bna = 1;
      p.amax_in = c.xmax;
      p.sA = a->A;
      p.bn1 = c.bn1;
      // (the kept "G" buffer holds only max |x|, for the backward's weight gradient)
      p.amax_keep = a->G ? reinterpret_cast<unsigned *>(a->G) : nullptr;
    }
  } else {
    p = tconv_fwd(d, R, a->Z, a->Wt, a->U, L.wpk);
    p.bias_r = a->bWt;
    if (f16x2_unfold(d)) {  // fp16 splits: max |Z| (spatial epilogue), max |Wt|
      HIP_TRY(launch_absmax(a->Wt, (int64_t)R * R * 9, L.amax + kAmaxWords, s));
      p.f16x2 = 1;
      p.amax_in = L.amax;
      p.amax_w = L.amax + kAmaxWords;
      if (a->G)  // (the kept G carries max |Z| to the backward's weight gradient)
        p.amax_keep = reinterpret_cast<unsigned *>(a->G + (size_t)N * K * C * T * V);
    }
  }
  p.in_bf16 = z_bf16(d) ? 1 : 0;
  if (d->training) {
    p.stat_sum = L.s2;
    p.stat_sq = L.q2;
  }
  // (the folded forward on k_conv_x3: BN2 statistics as per-tile partials)
  if (c.stat_parts) p.stat_part = L.s2part;
  HIP_TRY(launch_conv_gemm(p, s));
  return STGCN_OK;
}

// BN2 (st_graphconv.py:100) + ReLU (:105)
int fwd_bn2_out(FwdCtx &c) {
  const stgcn_desc_t *d = c.d;
  const stgcn_fwd_args_t *a = c.a;
  const FwdLayout &L = c.L;
  hipStream_t s = c.s;
  const int N = d->N, R = d->C_out, To = d->T_out, V = d->V;
  double *ys = (d->training && a->y_stats) ? a->y_stats : nullptr;
  if (c.stat_parts)  // (zeroes y_stats on the way)
    HIP_TRY(launch_bn_finalize_parts(L.s2part, fold_stat_tiles(d), R, (int64_t)N * To * V, d->eps,
                                     d->momentum, d->training, a->rm2, a->rv2, c.st2, c.st2 + R, s,
                                     ys, kAmaxWords));
  else
    HIP_TRY(launch_bn_finalize(L.s2, L.q2, R, (int64_t)N * To * V, d->eps, d->momentum,
                               d->training, a->rm2, a->rv2, c.st2, c.st2 + R, s));
  const Dropout ydrop = make_dropout(d, a->dropout_p, a->seed, c.seed_dev);
  // (ABI 5: y_stats holds 5 * C_out sums; the last three -- over the ReLU mask --
  // feed the next block's deferred-dx chain, meaningless under dropout; ABI 7:
  // then max y in STGCN_STATS_AMAX_WORDS words, the next block's operand bound;
  // ABI 8, y null: only these -- k_bn_relu_stats; ABI 9, y and y_stats null:
  // nothing -- the consumer forms ReLU(BN2(U)) itself)
  if (!a->y && !ys) return STGCN_OK;
  if (ys && !c.stat_parts) HIP_TRY(hipMemsetAsync(ys, 0, y_stats_bytes(R), s));
  HIP_TRY(launch_bn_relu_fwd(a->U, c.bn2, a->y, N, R, To * V, ys, ys ? ys + R : nullptr, ydrop, s,
                             (ys && !ydrop.thresh) ? ys + 2 * R : nullptr,
                             ys ? reinterpret_cast<unsigned *>(ys + 5 * R) : nullptr));
  return STGCN_OK;
}

}  // namespace

extern "C" int stgcn_block_fwd(const stgcn_desc_t *d, const stgcn_fwd_args_t *a, void *workspace,
                               size_t workspace_bytes, void *stream) {
  return stgcn_block_fwd_dseed(d, a, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int stgcn_block_fwd_dseed(const stgcn_desc_t *d, const stgcn_fwd_args_t *a,
                                     const uint64_t *seed_dev, void *workspace,
                                     size_t workspace_bytes, void *stream) {
  STAGE(stgcn_check_desc(d));
  STAGE(check_aligned({NamedPtr{seed_dev, "seed_dev"}}, 8));
  STAGE(fwd_check_args(d, a, workspace));
  FwdCtx c{d, a, fwd_layout(d, workspace), (hipStream_t)stream};
  c.seed_dev = seed_dev;
  if (!workspace || workspace_bytes < c.L.total)
    return fail(STGCN_E_INVALID, "workspace too small");
  c.res = residual(d);
  c.xu = a->prev_U != nullptr;
  c.fold = fold_w(d);
  c.bna = fold_bna(d);
  c.pre = c.fold && a->prep && prep_applies(d);
  c.P = c.pre ? prep_layout(d, a->prep) : PrepLayout{};
  c.stat_parts = fold_stat_parts(d) && c.L.s2part;
  c.no_memset = c.stat_parts && a->x_stats;
  c.st1 = a->stats;
  c.st2 = a->stats + 2 * d->C_in;
  c.bn1 = bn_ref(c.st1, d->C_in, a->g1, a->b1);
  c.bn2 = bn_ref(c.st2, d->C_out, a->g2, a->b2);
  STAGE(fwd_bn1_stats(c, workspace));
  STAGE(fwd_spatial(c));
  if (c.res) return residual_fwd_tail(c);
  STAGE(fwd_temporal(c));
  return fwd_bn2_out(c);
}

// ---- stgcn_block_bwd in stages ----
namespace {

struct BwdCtx {
  const stgcn_desc_t *d;
  const stgcn_bwd_args_t *a;
  BwdLayout L;
  hipStream_t s;
  bool res;
  bool defer;  // deferred dx (ABI 5; bwd_spatial_dgrad)
  Dropout drop;
  BnRef bn1, bn2;
  // (Tq's fp64 re-layout goes straight into launch_fold_sdz's scratch slot in
  // this call's workspace -- never into the prep buffer, which holds only the
  // step's weight-only operands and may be shared by concurrent backwards)
  double *tqT;
  PrevBn pvb;        // defer: the previous block's BN2, the chain sums s1 / s2
  const float *xin;  // defer: the previous block's U in place of x
  // The fused folded block (fold_spb): its small kernels run on the library's
  // side stream beside the data- and weight-gradient GEMMs (host_common.h
  // SideFork; DESIGN.md "Backward small kernels beside the GEMMs"). Not forked:
  // side() == s, and the stages below are the serial sequence.
  bool overlap;
  SideFork fk;
  hipStream_t side() const { return fk.forked() ? fk.side() : s; }
};

int bwd_check_args(const stgcn_desc_t *d, const stgcn_bwd_args_t *a, void *workspace) {
  int rc;
  const bool res = residual(d);
  // ABI 8: x null after a forward from prev_U -- the fused folded backward (or the
  // bf16 spatial backward in prev mode) reads prev_U (deferred dx) and the kept
  // G, nothing else reads x
  const bool xnull = a && !a->x;
  if (xnull && (!x_from_u(d) || !a->G))
    return fail(STGCN_E_INVALID, "x null: needs STGCN_PLAN_X_FROM_U and the kept G");
  if (!a || (!a->dy && !a->dy_nc) || (!a->x && !xnull) || !a->Z || (!res && !a->U) || !a->stats || !a->A || !a->W ||
      !a->bW || !a->Wt || !a->g1 || !a->b1 || !a->g2 || !a->b2 || !a->dA || !a->dW || !a->dbW ||
      !a->dWt || !a->dbWt || !a->dg1 || !a->db1 || !a->dg2 || !a->db2 || (d->need_dx && !a->dx))
    return fail(STGCN_E_INVALID, "null tensor argument");
  if (res && (!a->Za || !a->y || (projection(d) && (!a->Wr || !a->dWr || !a->dbr))))
    return fail(STGCN_E_INVALID, "residual block: null Za / y / projection tensors");
  if (res && a->dy_sums)
    return fail(STGCN_E_INVALID, "dy_sums applies to the non-residual block only");
  // ABI 10: dy as one value per (clip, channel): the three ReLU + BN2 backward
  // passes of the non-residual block (not the residual block's ReLU backward, nor
  // the frame-wise dU A pass of the block without G)
  if (a->dy_nc && (res || (cols_sums(d) && fold_bna(d))))
    return fail(STGCN_E_UNSUPPORTED, "dy_nc: this block's backward needs the full dy");
  const Dropout drop = make_dropout(d, a->dropout_p, a->seed, nullptr);
  if (drop.thresh && a->dy_sums)
    return fail(STGCN_E_INVALID, "dy_sums cannot be combined with dropout");
  if (!d->training && (a->dy_sums || a->prev_sums))
    return fail(STGCN_E_INVALID, "stack chaining applies to training mode only");
  if (a->dy_coef && (!a->dy_sums || res || drop.thresh))
    return fail(STGCN_E_INVALID, "dy_coef needs dy_sums, a non-residual block, no dropout");
  // the alignment contract (stgcn_hip.h): 16 bytes, 4 for prev_stats. With x and
  // prev_U aligned, the deferred-dx decision (spatial_dx_prev_supported,
  // which assumes aligned pointers) and the launch agree.
  if ((rc = check_aligned(
           {STGCN_P(a, dy), STGCN_P(a, x), STGCN_P(a, Z), NamedPtr{res ? nullptr : a->U, "U"},
            STGCN_P(a, stats), STGCN_P(a, A), STGCN_P(a, W), STGCN_P(a, bW), STGCN_P(a, Wt),
            STGCN_P(a, g1), STGCN_P(a, b1), STGCN_P(a, g2), STGCN_P(a, b2),
            NamedPtr{d->need_dx ? a->dx : nullptr, "dx"}, STGCN_P(a, dA), STGCN_P(a, dW),
            STGCN_P(a, dbW), STGCN_P(a, dWt), STGCN_P(a, dbWt), STGCN_P(a, dg1), STGCN_P(a, db1),
            STGCN_P(a, dg2), STGCN_P(a, db2), STGCN_P(a, Wr), STGCN_P(a, Za), STGCN_P(a, y),
            STGCN_P(a, dWr), STGCN_P(a, dbr), STGCN_P(a, G), STGCN_P(a, dy_sums),
            STGCN_P(a, prev_g2), STGCN_P(a, prev_b2), STGCN_P(a, prev_sums), STGCN_P(a, prev_U),
            STGCN_P(a, x_stats), STGCN_P(a, dx_coef), STGCN_P(a, dy_coef), STGCN_P(a, prep),
            STGCN_P(a, dy_nc), NamedPtr{workspace, "workspace"}},
           16)) ||
      (rc = check_aligned({STGCN_P(a, prev_stats)}, 4)))
    return rc;
  return STGCN_OK;
}

// A ReLU + BN2 backward over U (N, C_out, L) with the workspace's sums: what the
// block's own (bwd_relu_bn2) and the residual block's over Z share
Bn2Bwd bn2_bwd(const BwdCtx &c, const float *dy, const float *U, float *dU, int L) {
  Bn2Bwd q;
  q.dy = dy;
  q.U = U;
  q.bn = c.bn2;
  q.sg = c.L.sg;
  q.sgu = c.L.sgu;
  q.dU = dU;
  q.sdu = c.L.sdu;
  q.N = c.d->N;
  q.C = c.d->C_out;
  q.L = L;
  q.training = c.d->training;
  return q;
}

// Non-residual block: ReLU + BN2 backward -> dU, dgamma2, dbeta2, d(temporal
// bias); the reduction comes from the next block when it was chained (dy_sums).
// Residual block: final ReLU backward -> dU (= d(conv out) = d(residual));
// temporal and projection bias grads are its per-channel sums
int bwd_relu_bn2(BwdCtx &c) {
  const stgcn_desc_t *d = c.d;
  const stgcn_bwd_args_t *a = c.a;
  const BwdLayout &L = c.L;
  hipStream_t s = c.s;
  const int N = d->N, R = d->C_out, T = d->T, To = d->T_out, V = d->V;
  const Dropout &drop = c.drop;
  if (c.res) {
    HIP_TRY(launch_relu_bwd(a->dy, a->y, L.dU, L.sdu, N, R, To * V, drop.thresh ? drop.scale : 1.f,
                            s));
    HIP_TRY(launch_bn_grads_out(L.sdu, L.sdu, nullptr, R, a->dbWt, a->dbr ? a->dbr : a->dbWt,
                                nullptr, s));
    return STGCN_OK;
  }
  Bn2Bwd q = bn2_bwd(c, a->dy, a->U, L.dU, To * V);
  q.dy_nc = a->dy_nc;
  q.drop = drop;
  q.du_bf16 = du_bf16(d) ? 1 : 0;
  q.dy_coef = a->dy_coef;
  if (a->dy_sums) {
    q.sg = a->dy_sums;
    q.sgu = a->dy_sums + R;
  } else {
    HIP_TRY(launch_bn_relu_bwd_reduce(q, L.sg, L.sgu, s));
  }
  // (with the clip-chunk sums of dU: sum_{n,t} dZ follows from them per tap,
  // no pass over dZ)
  if (cols_sums(d)) {
    q.cs = L.fcs;
    if (fold_bna(d)) {  // + dU A (the weight gradient's P) in dZ's buffer
      q.dUA = L.dZ;
      q.amax = L.amax;
      q.amaxa = L.amax + 2 * kAmaxWords;
      q.A = a->A;
      q.V = V;
      HIP_TRY(launch_bn_relu_bwd_apply_fr(q, s));
    } else {
      q.amax = f16x2_tw(d) ? L.amax : nullptr;  // (f16x2: max |dU|)
      HIP_TRY(launch_bn_relu_bwd_apply_cols(q, s));
    }
    // (fork: the small kernels from here to launch_chain_coef need the apply
    // pass's sums, never the GEMMs' tensors)
    if (c.overlap) HIP_TRY(c.fk.begin(s));
    HIP_TRY(launch_fold_tq(L.fcs, apply_cols_chunks(N), R, T, To, V, d->stride, L.ftq, c.tqT,
                           c.side()));
  } else {
    HIP_TRY(launch_bn_relu_bwd_apply(q, s));
  }
  HIP_TRY(launch_bn_grads_out(q.sg, q.sgu, L.sdu, R, a->dg2, a->db2, a->dbWt, c.side()));
  return STGCN_OK;
}

// The folded block (kernels_fold.hip): Wc_q = Wt_q W'; the data gradient
// with Wc gives H = W'^T dZ directly (C_in channels), the weight gradient
// over G gives dWc, and dWt, dW', sum_{n,t} dZ follow from dWc and the dU sums.
int bwd_fold_temporal(BwdCtx &c) {
  const stgcn_desc_t *d = c.d;
  const stgcn_bwd_args_t *a = c.a;
  const BwdLayout &L = c.L;
  hipStream_t s = c.s;
  const int N = d->N, C = d->C_in, R = d->C_out, T = d->T, V = d->V, K = d->K;
  // (ABI 7: the weight-only operands from stgcn_fold_prep, same step)
  const bool pre = a->prep && prep_applies(d);
  const PrepLayout P = pre ? prep_layout(d, a->prep) : PrepLayout{};
  const float *Wc = a->Z;  // (left there by the forward)
  const float *bZ = L.bZ, *fscr = L.fscr;
  double *f64scr = L.f64scr;
  const unsigned *amax_wc = L.amax + kAmaxWords;
  if (pre) {
    Wc = P.Wc;
    bZ = P.bZ;
    fscr = P.fscr_b;
    f64scr = P.f64;
    amax_wc = P.amax;
  } else {
    if (!fold_wc_in_z(d)) {
      HIP_TRY(launch_fold_w(a->Wt, a->W, R, C, L.Wc, L.fscr, s));
      Wc = L.Wc;
    }
    HIP_TRY(launch_bias_rv(a->A, a->bW, L.bZ, K, R, V, s));
    HIP_TRY(launch_fold_prep_bwd(a->Wt, a->W, R, C, L.fscr, s));
    HIP_TRY(c.fk.to_side());  // (forked: launch_fold_sdz reads this Wc)
  }
  if (fold_spb(d)) {  // dbW and the bias part of dA first: the data gradient adds to dA;
    // BN1's sd from the dU sums (fp64, exact against the cancellation in sum dxhat)
    // (forked: beside the data gradient, which with sd_given and partial slots
    // touches neither sd nor dA; launch_dA_reduce follows on the same stream)
    HIP_TRY(launch_fold_sdz(f64scr, a->Wt, Wc, L.ftq, R, C, V, L.SdZ, L.SdH, c.side(), pre,
                            c.tqT));
    HIP_TRY(launch_fold_small_sd(L.SdZ, a->A, a->bW, R, V, a->dbW, a->dA, L.SdH, C, L.sd,
                                 c.side()));
  }
  if (f16x2_dgrad(d) && !pre)  // the fp16 splits' operand scales: max |dU| (apply pass), max |Wc|
    HIP_TRY(launch_absmax(Wc, (int64_t)R * C * 9, L.amax + kAmaxWords, s));
  {
    // (deterministic dA: every workgroup's partial in its own slot, summed below)
    int64_t dparts = 0;
    const int dnpl = fold_dgrad_npl(d);
    auto dA_slots = [&](ConvGemmParams &q) {
      q.dA_part = nullptr;  // (no slots: fp32 atomics into dA)
      if (!fold_spb(d) || !L.dApart) return;
      const int rows = conv_x3_tile_rows(q, dnpl);
      const int64_t nb = (int64_t)N * q.n_mtiles * ((q.R + rows - 1) / rows);
      if (dparts + nb > L.dA_cap) return;
      q.dA_part = L.dApart + dparts * V * V;
      dparts += nb;
    };
    for (int ph = 0; ph < tconv_dgrad_phases(d); ++ph) {
      ConvGemmParams p = tconv_dgrad(d, C, ph, L.dU, Wc, L.H, L.wpk);
      if (p.M <= 0) continue;
      if (f16x2_dgrad(d)) {
        p.f16x2 = 1;
        p.amax_in = L.amax;
        p.amax_w = amax_wc;
      }
      if (fold_spb(d)) {  // dxhat -> dx; BN1 / chain sums and dA from the tile (H on chip)
        p.spb = 1;
        p.out = d->need_dx ? a->dx : nullptr;
        p.sx = c.xin;
        p.sA = a->A;
        p.bn1 = c.bn1;
        if (c.defer) p.prev = c.pvb;
        p.sd = L.sd;
        p.sd_given = 1;
        p.sdn = L.sdn;
        p.dA = a->dA;
      }
      if (pre) {
        p.wpk = reinterpret_cast<float *>(P.wpk_d[ph]);
        p.wpk_ready = 1;
      }
      dA_slots(p);
      // (no slots: the launch's atomics into dA must follow launch_fold_small_sd's
      // store -- joined here, the call is serial from this launch on)
      if (!p.dA_part) HIP_TRY(c.fk.join());
      HIP_TRY(launch_conv_gemm(p, s));
    }
    HIP_TRY(c.fk.to_side());  // (forked: the partials, and chain_coef's sdn / s1 / s2)
    HIP_TRY(launch_dA_reduce(L.dApart, dparts, V * V, L.dAlvl, a->dA, c.side()));
  }
  WgradParams w;
  if (fold_bna(d)) {  // dWc = sum (dU A) BN1(x): Q = x with BN1 at staging, P = dU A
    const unsigned *xmax = reinterpret_cast<const unsigned *>(a->G);  // (the forward's max |x|)
    if (!xmax) {
      HIP_TRY(launch_absmax(a->x, (int64_t)N * C * T * V, L.amax + 3 * kAmaxWords, s));
      xmax = L.amax + 3 * kAmaxWords;
    }
    w = make_wgrad_taps(d, L.dZ, a->x, L.slab, C);
    if (w.bf16 != 3) return fail(STGCN_E_HIP, "bna weight gradient: no split plan");
    w.f16x2 = 1;
    w.amax_p = L.amax + 2 * kAmaxWords;
    w.amax_q = xmax;
    w.q_bn = c.bn1;
  } else {
    const float *G = a->G;  // kept fp32 G (f16x2: its max |G| follows it), else recomputed
    const unsigned *amax_g = G ? reinterpret_cast<const unsigned *>(G + (size_t)N * C * T * V)
                               : L.amax + 2 * kAmaxWords;
    if (!G) {
      SpatialFwd f = spatial_fwd(d, a->x, c.bn1, a->A);
      f.G = L.G;
      f.amax = f16x2(d) ? L.amax + 2 * kAmaxWords : nullptr;
      HIP_TRY(launch_gather_fwd(f, s));
      G = L.G;
    }
    w = make_wgrad_taps(d, L.dU, G, L.slab, C);
    if (f16x2(d) && w.bf16 == 3) {  // max |dU| (apply pass), max |G|
      w.f16x2 = 1;
      w.amax_p = L.amax;
      w.amax_q = amax_g;
    }
  }
  HIP_TRY(launch_wgrad_taps(w, s));
  HIP_TRY(c.fk.to_main());  // (forked: Tq, and whatever a serial tail reads, is on the side stream)
  HIP_TRY(launch_fold_grads(L.slab, w.S, fscr, bZ, L.ftq, R, C, V, L.dWc, a->dWt, a->dW, s));
  return STGCN_OK;
}

// The unfolded block's temporal conv backward: data gradient dZ = conv^T(dU),
// weight gradient dWt, and the residual block's BN2 + ReLU backward over Z
int bwd_unfold_temporal(BwdCtx &c) {
  const stgcn_desc_t *d = c.d;
  const stgcn_bwd_args_t *a = c.a;
  const BwdLayout &L = c.L;
  hipStream_t s = c.s;
  const int N = d->N, C = d->C_in, R = d->C_out, T = d->T, To = d->T_out, V = d->V, K = d->K;
  // Temporal conv data-gradient: dZ = conv^T(dU)
  for (int ph = 0; ph < tconv_dgrad_phases(d); ++ph) {
    ConvGemmParams p = tconv_dgrad(d, R, ph, L.dU, a->Wt, L.dZ, L.wpk);
    if (p.M <= 0) continue;
    p.in_bf16 = du_bf16(d) ? 1 : 0;
    HIP_TRY(launch_conv_gemm(p, s));
  }
  // Temporal conv weight-gradient: dWt[co][ci][q] = sum dU[co] * Z[ci](shifted)
  {
    WgradParams w = make_wgrad_taps(d, L.dU, c.res ? a->Za : a->Z, L.slab);
    w.q_bf16 = z_bf16(d) ? 1 : 0;
    w.p_bf16 = du_bf16(d) ? 1 : 0;
    if (f16x2_unfold(d) && w.bf16 == 3) {  // fp16 splits: max |dU| (apply pass), max |Z|
      if (!cols_sums(d))  // (the apply pass without the column sums forms no max |dU|)
        HIP_TRY(launch_absmax(L.dU, (int64_t)N * R * To * V, L.amax, s));
      const unsigned *zmax =
          a->G ? reinterpret_cast<const unsigned *>(a->G + (size_t)N * K * C * T * V) : nullptr;
      if (!zmax) {  // (no kept G: a pass over Z)
        HIP_TRY(launch_absmax(a->Z, (int64_t)N * R * T * V, L.amax + 3 * kAmaxWords, s));
        zmax = L.amax + 3 * kAmaxWords;
      }
      w.f16x2 = 1;
      w.amax_p = L.amax;
      w.amax_q = zmax;
    }
    HIP_TRY(launch_wgrad_taps(w, s));
    HIP_TRY(launch_slab_reduce(L.slab, w.S, (int64_t)R * R * 9, a->dWt, 0, R, 1, R, s));
  }
  if (c.res) {
    // BN2 + ReLU backward over Z (residual block, st_graphconv.py:76-77): dZ in place
    const Bn2Bwd q = bn2_bwd(c, L.dZ, a->Z, L.dZ, T * V);
    HIP_TRY(launch_bn_relu_bwd_reduce(q, L.sg, L.sgu, s));
    HIP_TRY(launch_bn_relu_bwd_apply(q, s));
    HIP_TRY(launch_bn_grads_out(L.sg, L.sgu, nullptr, R, a->dg2, a->db2, nullptr, s));
  }
  return STGCN_OK;
}

// Spatial conv backward. Recompute G = f(BN1(x)) A^T (f = ReLU in the
// residual block), then
//   dW' = dZ G^T (split-K), H_k = W_k^T dZ, dxhat = sum_k H_k A_k,
//   dA = sum H_k^T f(BN1(x)) + bias part, dbW = sum dZ rowsum(A_k).
// This stage: dW' of the unfolded block (and the residual block's pass over dZ
// for sum_{n,t} dZ)
int bwd_spatial_wgrad(BwdCtx &c) {
  const stgcn_desc_t *d = c.d;
  const stgcn_bwd_args_t *a = c.a;
  const BwdLayout &L = c.L;
  hipStream_t s = c.s;
  const int N = d->N, C = d->C_in, R = d->C_out, T = d->T, V = d->V, K = d->K;
  WgradParams w;
  if (fused_sp(d) && a->G) {
    // the bf16 G kept by the fused forward (k_sp_fwd_bf16) -> k_wgrad_gemm_gk
    w = wgrad_gk(d, L.dZ, a->G, L.slab);
    HIP_TRY(launch_wgrad_gk(w, s));
  } else {
    const float *G = fused_sp(d) ? nullptr : a->G;  // kept fp32 G, else recomputed
    if (!G) {
      SpatialFwd f = spatial_fwd(d, a->x, c.bn1, a->A);
      f.G = L.G;
      HIP_TRY(launch_gather_fwd(f, s));
      G = L.G;
    }
    w = wgrad_spatial(d, L.dZ, G, L.slab);
    HIP_TRY(launch_wgrad(w, s));
  }
  HIP_TRY(launch_slab_reduce(L.slab, w.S, (int64_t)R * K * C, a->dW, 1, R, K, C, s));
  if (!cols_sums(d)) HIP_TRY(launch_sum_nt(L.dZ, N, R, T, V, L.SdZ, s));
  return STGCN_OK;
}

// Spatial data gradient: dbW and the bias part of dA from sum_{n,t} dZ, then dZ
// (or the folded block's H) -> dx, dA and the BN1 sums.
// Deferred dx (ABI 5): the BN1 backward apply of this block is folded into the
// previous block's ReLU+BN2 backward apply (launch_bn_relu_bwd_apply with
// dy_coef). The spatial backward then reads the previous block's U in place of
// x (PrevBn: x rebuilt, that block's mask / uhat sums), dx receives dxhat, and
// launch_chain_coef forms dg1 / db1, the coefficients and the previous block's
// ReLU+BN2 sums: dx never makes its own HBM round trip.
int bwd_spatial_dgrad(BwdCtx &c) {
  const stgcn_desc_t *d = c.d;
  const stgcn_bwd_args_t *a = c.a;
  const BwdLayout &L = c.L;
  hipStream_t s = c.s;
  const int C = d->C_in, R = d->C_out, V = d->V, K = d->K;
  // (done in the folded block's data gradient: kernels_x3.hip spb_epilogue)
  if (fold_spb(d)) return STGCN_OK;
  // sum_{n,t} dZ: from the temporal weight and the per-tap dU sums on the
  // non-residual block (dZ = conv^T(dU)); the residual block's dZ passes BN2
  // (the fused folded backward did both before its data gradient)
  if (cols_sums(d))
    HIP_TRY(launch_fold_sdz(L.f64scr, a->Wt, nullptr, L.ftq, R, C, V, L.SdZ, nullptr, s));
  HIP_TRY(launch_spatial_small(L.SdZ, a->A, a->bW, K, R, V, a->dbW, a->dA, s));
  // (fused: from dZ; else from H, which the H GEMM or the folded data gradient wrote)
  SpatialBwd b = spatial_bwd(d, fused_spb(d) ? L.dZ : L.H, c.xin, c.bn1, a->A, a->dx, a->dA, L.sd,
                             L.sdn);
  if (c.defer) b.prev = c.pvb;
  if (fused_spb(d)) {
    // H = W'^T dZ, dx = sum_k H_k A_k, dA, BN1 sums in one kernel (H stays on chip)
    b.W = a->W;
    b.wpk = L.wpk;
    HIP_TRY(launch_sp_bwd_fused(b, s));
    return STGCN_OK;
  }
  // The H GEMM and the joint kernel run over the whole batch at once (clip
  // slices sized to the Infinity Cache measured slower: cfg5 2126 vs 2324 clips/s,
  // the persistent joint kernels flush dA and the BN1 sums once per launch).
  if (!fold_w(d)) {  // (the folded block's data gradient wrote H)
    const float *Wz = a->W;
    if (K > 1) {
      HIP_TRY(launch_pack_w(a->W, L.Wpk, K, R, C, s));
      Wz = L.Wpk;
    }
    HIP_TRY(launch_conv_gemm(h_gemm(d, L.dZ, Wz, L.H, L.wpk), s));
  }
  // (deterministic dA: the joint kernel's workgroup partials, if it takes them)
  int64_t sparts = 0;
  b.dA_part = L.dApart;
  b.part_cap = L.dA_cap;
  b.nparts = &sparts;
  HIP_TRY(launch_spatial_dx(b, s));
  HIP_TRY(launch_dA_reduce(L.dApart, sparts, K * V * V, L.dAlvl, a->dA, s));
  return STGCN_OK;
}

// BN1 backward (deferred: only its coefficients, launch_chain_coef) and the
// residual path gradient (added to dx after the BN1 backward)
int bwd_bn1_tail(BwdCtx &c) {
  const stgcn_desc_t *d = c.d;
  const stgcn_bwd_args_t *a = c.a;
  const BwdLayout &L = c.L;
  hipStream_t s = c.s;
  const int N = d->N, C = d->C_in, R = d->C_out, T = d->T, V = d->V;
  if (c.defer) {  // (forked: after launch_dA_reduce on the side stream, beside launch_fold_grads)
    HIP_TRY(launch_chain_coef(L.sd, L.sdn, c.bn1, L.s1, L.s2, a->x_stats, C, (int64_t)N * T * V,
                              a->dg1, a->db1, a->dx_coef, a->prev_sums, c.side()));
    return STGCN_OK;
  }
  HIP_TRY(launch_bn_grads_out(L.sd, L.sdn, nullptr, C, a->dg1, a->db1, nullptr, s));
  const float *add = nullptr;
  if (c.res && !projection(d)) add = L.dU;  // identity: d(res) = dU
  if (projection(d)) {
    // dWr[co][ci] = sum dU[co](m) x[ci](s*m)
    WgradParams w = wgrad_proj(d, L.dU, a->x, L.slab);
    HIP_TRY(launch_wgrad(w, s));
    HIP_TRY(launch_slab_reduce(L.slab, w.S, (int64_t)R * C, a->dWr, 0, R, 1, C, s));
    if (d->need_dx) {  // Rg[ci](s*m) = sum_co Wr[co][ci] dU[co](m); other frames 0
      HIP_TRY(hipMemsetAsync(L.Rg, 0, sizeof(float) * (size_t)N * C * T * V, s));
      HIP_TRY(launch_conv_gemm(proj_dgrad(d, L.dU, a->Wr, L.Rg, L.wpk), s));
      add = L.Rg;
    }
  }
  if (d->need_dx) {
    const bool chain = d->training && a->prev_g2 && a->prev_b2 && a->prev_sums;
    const bool chain_u = chain && a->prev_U && a->prev_stats;
    if (chain) HIP_TRY(hipMemsetAsync(a->prev_sums, 0, sizeof(double) * 2 * C, s));
    BnRef pbn2;  // the previous block's BN2: gamma / beta (chain), statistics (chain_u)
    if (chain) pbn2 = bn_ref(nullptr, 0, a->prev_g2, a->prev_b2);
    if (chain_u) pbn2 = bn_ref(a->prev_stats, C, a->prev_g2, a->prev_b2);
    HIP_TRY(launch_bn1_bwd_apply(a->dx, a->x, c.bn1, L.sd, L.sdn, add, N, C, T * V,
                                 (int64_t)N * T * V, d->training, pbn2,
                                 chain ? a->prev_sums : nullptr, chain_u ? a->prev_U : nullptr, s));
  }
  return STGCN_OK;
}

}  // namespace

extern "C" int stgcn_block_bwd(const stgcn_desc_t *d, const stgcn_bwd_args_t *a, void *workspace,
                               size_t workspace_bytes, void *stream) {
  return stgcn_block_bwd_dseed(d, a, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int stgcn_block_bwd_dseed(const stgcn_desc_t *d, const stgcn_bwd_args_t *a,
                                     const uint64_t *seed_dev, void *workspace,
                                     size_t workspace_bytes, void *stream) {
  STAGE(stgcn_check_desc(d));
  STAGE(check_aligned({NamedPtr{seed_dev, "seed_dev"}}, 8));
  STAGE(bwd_check_args(d, a, workspace));
  BwdCtx c{d, a, bwd_layout(d, workspace), (hipStream_t)stream};
  if (!workspace || workspace_bytes < c.L.total)
    return fail(STGCN_E_INVALID, "workspace too small");
  c.res = residual(d);
  c.drop = make_dropout(d, a->dropout_p, a->seed, seed_dev);
  const int N = d->N, C = d->C_in, R = d->C_out, T = d->T, V = d->V, K = d->K;
  c.bn1 = bn_ref(a->stats, C, a->g1, a->b1);
  c.bn2 = bn_ref(a->stats + 2 * C, R, a->g2, a->b2);
  // deferred dx (ABI 5; bwd_spatial_dgrad)
  c.defer = d->need_dx && d->training && !c.res && a->prev_g2 && a->prev_b2 && a->prev_sums &&
            a->prev_U && a->prev_stats && a->x_stats && a->dx_coef && a->dx_deferred &&
            (fused_spb(d) || fold_spb(d) || spatial_dx_prev_supported(N, C, T, V, K));
  if (!a->x && !c.defer)
    return fail(STGCN_E_INVALID,
                "x null: the backward must defer dx (prev_U, prev_stats, prev_g2 / prev_b2, "
                "prev_sums, x_stats, dx_coef, dx_deferred)");
  if (c.defer) {
    c.pvb = prev_bn(a->prev_stats, C, a->prev_g2, a->prev_b2);
    c.pvb.s1 = c.L.s1;
    c.pvb.s2 = c.L.s2;
  }
  c.xin = c.defer ? a->prev_U : a->x;
  if (cols_sums(d)) c.tqT = fold_sdz_tq_slot(c.L.f64scr, R, C);
  // (every other path -- unfolded, bf16 / K = 3 spatial backward, residual -- is serial)
  c.overlap = fold_w(d) && fold_spb(d) && !c.res && cols_sums(d);

  HIP_TRY(hipMemsetAsync(workspace, 0, c.L.dbl_bytes, c.s));
  STAGE(bwd_relu_bn2(c));
  if (a->dx_deferred) *a->dx_deferred = c.defer ? 1 : 0;
  if (fold_w(d)) {
    STAGE(bwd_fold_temporal(c));
  } else {
    STAGE(bwd_unfold_temporal(c));
    STAGE(bwd_spatial_wgrad(c));
  }
  STAGE(bwd_spatial_dgrad(c));
  STAGE(bwd_bn1_tail(c));
  // (forked: the caller's stream waits for the side stream's last kernel, so the
  // call returns as a serial one does; on an error above c's destructor joins)
  HIP_TRY(c.fk.join());
  return STGCN_OK;
}

extern "C" int stgcn_bwd_overlap(int enable) {
  std::atomic<int> &mode = bwd_overlap_mode();
  return enable < 0 ? mode.load() : mode.exchange(enable ? 1 : 0);
}

// ---------------------------------------------------------------------------
// Measurement entry points (bench.py roofline): run ONE of the block's GEMM
// kernels `iters` times on the caller's stream between two hipEvents. The
// launch parameters come from the builders stgcn_block_fwd / _bwd use
// (block_plan.h) with operands carved from the scratch; where a timed launch
// still differs from the block's, plan_timed says so at the override
// (DESIGN.md lists the differences next to the roofline).
//   which 0: temporal (9,1) conv forward      (k_conv_gemm<9>)
//         1: temporal conv data-gradient      (k_conv_gemm<9> or <5>+<4>)
//         2: temporal conv weight-gradient    (k_wgrad<9>, slab reduce excluded)
//         3: spatial channel GEMM Z = W' G    (k_conv_gemm<1>; with the fused bf16
//            spatial forward: that kernel, joint contraction FLOPs included)
//         4: spatial backward dZ -> dx, dA, BN1 sums (k_sp_bwd_fused where it
//            applies, else the stacked H GEMM + the joint kernel; H GEMM and
//            joint contraction FLOPs)
//         5: the stacked H GEMM of the unfused spatial backward alone
//            (V = 50 fused: its dx kernel k_sp50_dx alone)
//         6: the joint kernel of the unfused spatial backward alone
//            (V = 50 fused: its dA kernel k_sp50_dA alone)
//            (k_spatial_bwd5 / _bwd6 / _bwd3: dx, dA, BN1 sums from H)
//         (5 and 6 fail with STGCN_E_UNSUPPORTED where k_sp_bwd_fused<25> runs)
// flops = the algorithmic FLOPs of one launch (SURVEY.md §8d terms).
// ---------------------------------------------------------------------------
namespace {
struct TimedPlan {
  ConvGemmParams cp[2];
  int ncp = 0;
  WgradParams wp{};
  bool wgrad = false;
  // which 3 on the fused bf16 spatial forward (k_sp_fwd_bf16 / k_sp_fwd_wide)
  bool spf = false;
  SpatialFwd sf;
  // which 4: the spatial backward (5: its H GEMM only, 6: its joint kernel only)
  bool spb = false, spb_gemm = true, spb_joint = true;
  SpatialBwd sb;
  // f16x2: the operands whose max |x| the fp16 splits scale by (computed once
  // before the timed launches, as the block does before its GEMMs)
  unsigned *amax = nullptr;
  const float *ax[2] = {nullptr, nullptr};
  int64_t an[2] = {0, 0};
  size_t bytes = 0;
  double flops = 0;
};

TimedPlan plan_timed(const stgcn_desc_t *d, int which, void *scratch) {
  TimedPlan P;
  Carve c(scratch);
  const int N = d->N, C = d->C_in, R = d->C_out, T = d->T, To = d->T_out, V = d->V, K = d->K;
  // (the folded block: the temporal GEMMs run over C_in channels on the G side)
  const bool fold = fold_w(d);
  const int CZ = fold ? C : R;
  const double tflops = 2.0 * 9 * R * (double)CZ * To * V * N;
  float *wpk = c.take<float>(wpk_floats(d));
  if (f16x2_tw(d) && which <= 2) P.amax = c.take<unsigned>(2 * kAmaxWords);
  if (which == 0) {
    const float *in = c.take<float>((size_t)N * CZ * T * V);
    const float *w = c.take<float>((size_t)R * CZ * 9);
    float *out = c.take<float>((size_t)N * R * To * V);
    const float *bias = c.take<float>(R);
    ConvGemmParams p = tconv_fwd(d, CZ, in, w, out, wpk);
    // differs from the block: BN2 sums always by the stat_sum / stat_sq atomics (the
    // block: in training only, and the folded training block per-tile stat_part)
    p.stat_sum = c.take<double>(R);
    p.stat_sq = c.take<double>(R);
    p.in_bf16 = z_bf16(d) ? 1 : 0;
    // differs from the block: a residual block's epilogue (residual add, final
    // ReLU, dropout) is not timed
    if (fold) {
      p.res = c.take<float>((size_t)R * To * V);
      p.res_shared = 1;
    } else {
      p.bias_r = bias;
    }
    if (P.amax) {
      p.f16x2 = 1;
      p.amax_in = P.amax;
      p.amax_w = P.amax + kAmaxWords;
      P.ax[0] = p.in;
      P.an[0] = (int64_t)N * CZ * T * V;
      P.ax[1] = p.w;
      P.an[1] = (int64_t)R * CZ * 9;
    }
    // differs from the block: the weights are always packed by the launch (no
    // stgcn_fold_prep pack, wpk_ready) and no bound is kept (amax_keep)
    if (fold_bna(d)) {  // x in: BN1 in the loader, the joint contraction in the epilogue
      p.bna = 1;
      p.sA = c.take<float>((size_t)V * V);
      p.bn1 = bn_packed(c.take<float>((size_t)4 * C), C);
    }
    P.cp[P.ncp++] = p;
    // (bna: + the joint contraction 2 K C_out T V^2 of the spatial forward, now here)
    P.flops = tflops + (fold_bna(d) ? 2.0 * K * R * (double)To * V * V * N : 0.0);
  } else if (which == 1) {
    const float *dU = c.take<float>((size_t)N * R * To * V);
    const float *w = c.take<float>((size_t)R * CZ * 9);
    float *out = c.take<float>((size_t)N * CZ * T * V);
    const bool f16 = P.amax && f16x2_dgrad(d);
    if (f16) {
      P.ax[0] = dU;
      P.an[0] = (int64_t)N * R * To * V;
      P.ax[1] = w;
      P.an[1] = (int64_t)R * CZ * 9;
    }
    // the fused SpatialConv backward epilogue's operands
    const float *sx = nullptr, *sA = nullptr, *st = nullptr;
    double *sd = nullptr;
    float *dA = nullptr;
    if (fold_spb(d)) {
      sx = c.take<float>((size_t)N * C * T * V);
      sA = c.take<float>((size_t)V * V);
      st = c.take<float>((size_t)4 * C);
      sd = c.take<double>((size_t)2 * C);
      dA = c.take<float>((size_t)V * V);
    }
    for (int ph = 0; ph < tconv_dgrad_phases(d); ++ph) {
      ConvGemmParams p = tconv_dgrad(d, CZ, ph, dU, w, out, wpk);
      if (p.M <= 0) continue;
      p.in_bf16 = du_bf16(d) ? 1 : 0;
      if (f16) {
        p.f16x2 = 1;
        p.amax_in = P.amax;
        p.amax_w = P.amax + kAmaxWords;
      }
      if (fold_spb(d)) {
        p.spb = 1;
        p.sx = sx;
        p.sA = sA;
        p.bn1 = bn_packed(st, C);
        p.sd = sd;
        p.sdn = sd + C;
        p.dA = dA;
        // differs from the block: dxhat is always stored and x is read as is (the
        // block: out null without need_dx; prev set when dx defers)
        p.sd_given = 0;       // differs from the block (1): the epilogue also sums sd
        p.dA_part = nullptr;  // differs from the block (partial slots): fp32 atomics into dA
      }
      p.wpk_ready = 0;  // differs from the block with stgcn_fold_prep: packed by the launch
      P.cp[P.ncp++] = p;
    }
    // (fused: + the joint contractions dxhat = H A and dA = H^T BN1(x))
    P.flops = tflops + (fold_spb(d) ? 4.0 * K * C * (double)T * V * V * N : 0.0);
  } else if (which == 2) {
    const float *dU = c.take<float>((size_t)N * R * To * V);
    const float *Z = c.take<float>((size_t)N * CZ * T * V);
    WgradParams w = make_wgrad_taps(d, dU, Z, nullptr, CZ);
    w.q_bf16 = z_bf16(d) ? 1 : 0;
    w.p_bf16 = du_bf16(d) ? 1 : 0;
    w.slab = c.take<float>((size_t)w.S * R * CZ * 9);
    if (P.amax && w.bf16 == 3) {
      w.f16x2 = 1;
      w.amax_p = P.amax;
      w.amax_q = P.amax + kAmaxWords;
      P.ax[0] = dU;
      P.an[0] = (int64_t)N * R * To * V;
      P.ax[1] = Z;
      P.an[1] = (int64_t)N * CZ * T * V;
    }
    if (fold_bna(d) && w.bf16 == 3) {  // P = dU A, Q = x with BN1 at staging
      // (taken whether or not scratch is given: the size query must match)
      w.q_bn = bn_packed(c.take<float>((size_t)4 * C), C);
    }
    P.wp = w;
    P.wgrad = true;
    P.flops = tflops;
  } else if (which >= 4) {
    // differs from the block (stgcn_time_kernel's launches): the joint kernel adds
    // dA by fp32 atomics (no partial slots) and no launch reads x in prev mode
    P.spb = true;
    P.spb_gemm = which != 6 && !fold;  // (folded: the data gradient wrote H)
    P.spb_joint = which != 5;
    const float *x = c.take<float>((size_t)N * C * T * V);
    const float *st = c.take<float>((size_t)4 * C);
    const float *A = c.take<float>((size_t)K * V * V);
    const float *W = c.take<float>((size_t)K * R * C);
    const float *dZ = c.take<float>((size_t)N * R * T * V);
    float *dx = c.take<float>((size_t)N * C * T * V);
    float *dA = c.take<float>((size_t)K * V * V);
    double *sd = c.take<double>((size_t)2 * C);
    float *H = fused_spb(d) ? nullptr : c.take<float>((size_t)N * K * C * T * V);
    if (!fused_spb(d) && !fold) {
      const float *Wz = c.take<float>((size_t)R * K * C);  // (the packed W' of the block)
      P.cp[P.ncp++] = h_gemm(d, dZ, Wz, H, wpk);
    }
    P.sb = spatial_bwd(d, fused_spb(d) ? dZ : H, x, bn_packed(st, C), A, dx, dA, sd, sd + C);
    P.sb.write_dx = 1;  // differs from the block without need_dx: dx is always written
    P.sb.W = W;
    P.sb.wpk = wpk;
    P.sb.only = P.spb_gemm && P.spb_joint ? 0 : (P.spb_gemm ? 1 : 2);
    P.flops = (P.spb_gemm ? 2.0 * K * C * (double)R * T * V * N : 0.0) +
              (P.spb_joint ? 4.0 * K * C * (double)T * V * V * N : 0.0);
    if (fused_spb50(d) && which >= 5)  // k_sp50_dx / _dA: each its H GEMM + its contraction
      P.flops = 2.0 * K * C * (double)R * T * V * N + 2.0 * K * C * (double)T * V * V * N;
  } else if (fused_sp(d)) {
    // the forward's fused spatial kernel (G kept in bf16 as in the stack)
    // differs from the block: a residual block's BN2 sums of Z are not taken
    P.spf = true;
    const float *x = c.take<float>((size_t)N * C * T * V);
    const float *st = c.take<float>((size_t)4 * C);
    P.sf = spatial_fwd(d, x, bn_packed(st, C), c.take<float>((size_t)K * V * V));
    P.sf.wpk = wpk;
    P.sf.W = c.take<float>((size_t)K * R * C);
    P.sf.biasZ = c.take<float>((size_t)R * V);
    P.sf.Z = c.take<float>((size_t)N * R * T * V);
    P.sf.z_bf16 = z_bf16(d) ? 1 : 0;
    P.sf.Gk = reinterpret_cast<__bf16 *>(c.take<char>(sp_keep_g_bytes(N, C, T, V, K)));
    P.flops = 2.0 * K * C * (double)R * T * V * N + 2.0 * K * C * (double)T * V * V * N;
  } else {
    const float *G = c.take<float>((size_t)N * K * C * T * V);
    const float *Wz = c.take<float>((size_t)R * K * C);
    float *Z = c.take<float>((size_t)N * R * T * V);
    const float *biasZ = c.take<float>((size_t)R * V);
    // differs from the block: a residual block's BN2 sums of Z (stat_sum / stat_sq
    // in training) are not taken
    P.cp[P.ncp++] = spatial_gemm(d, G, Wz, Z, biasZ, wpk);
    P.flops = 2.0 * K * C * (double)R * T * V * N;
  }
  P.bytes = c.off;
  return P;
}
}  // namespace

extern "C" {

size_t stgcn_time_kernel_bytes(const stgcn_desc_t *d, int which) {
  if (stgcn_check_desc(d) != STGCN_OK || which < 0 || which > 6) return 0;
  if (which >= 5 && fused_spb(d) && !fused_spb50(d)) return 0;
  if ((which == 3 || which == 5) && fold_w(d)) return 0;  // (no spatial / H GEMM there)
  if (which >= 4 && fold_spb(d)) return 0;  // (inside the data gradient, which 1)
  return plan_timed(d, which, nullptr).bytes;
}

int stgcn_time_kernel(const stgcn_desc_t *d, int which, void *scratch, size_t scratch_bytes,
                      int iters, void *stream, float *avg_ms, double *flops) {
  int rc = stgcn_check_desc(d);
  if (rc) return rc;
  if (which < 0 || which > 6 || iters <= 0 || !avg_ms || !flops)
    return fail(STGCN_E_INVALID, "bad timing request");
  if (which >= 5 && fused_spb(d) && !fused_spb50(d))
    return fail(STGCN_E_UNSUPPORTED, "the spatial backward is one fused kernel here (which 4)");
  if ((which == 3 || which == 5) && fold_w(d))
    return fail(STGCN_E_UNSUPPORTED, "the folded block has no spatial / H GEMM");
  if (which >= 4 && fold_spb(d))
    return fail(STGCN_E_UNSUPPORTED, "the folded block's spatial backward runs inside its data "
                                     "gradient (which 1)");
  TimedPlan P = plan_timed(d, which, scratch);
  if (!scratch || scratch_bytes < P.bytes) return fail(STGCN_E_INVALID, "scratch too small");
  hipStream_t s = (hipStream_t)stream;
  auto launch = [&]() -> hipError_t {
    if (P.wgrad) return launch_wgrad_taps(P.wp, s);
    if (P.spb) {
      if (fused_spb(d)) return launch_sp_bwd_fused(P.sb, s);
      if (P.spb_gemm) {
        hipError_t e = launch_conv_gemm(P.cp[0], s);
        if (e != hipSuccess || !P.spb_joint) return e;
      }
      return launch_spatial_dx(P.sb, s);
    }
    if (P.spf) return launch_sp_fwd_bf16(P.sf, s);
    for (int i = 0; i < P.ncp; ++i) {
      hipError_t e = launch_conv_gemm(P.cp[i], s);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  };
  if (P.amax) {  // the f16x2 operand scales (not timed)
    HIP_TRY(hipMemsetAsync(P.amax, 0, 2 * kAmaxWords * sizeof(unsigned), s));
    for (int i = 0; i < 2; ++i)
      if (P.ax[i]) HIP_TRY(launch_absmax(P.ax[i], P.an[i], P.amax + i * kAmaxWords, s));
  }
  HIP_TRY(launch());  // warm-up
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  HIP_TRY(hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) HIP_TRY(launch());
  HIP_TRY(hipEventRecord(e1, s));
  HIP_TRY(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *avg_ms = ms / iters;
  *flops = P.flops;
  return STGCN_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// SpatialConv on its own (st_graphconv.py:139-152), ABI 4: the block's
// spatial kernels with BatchNorm replaced by the identity (mean 0, invstd 1,
// gamma 1, beta 0: (x - 0) * 1 * 1 + 0 == x exactly in fp32).
//   fwd: G = x A_k^T (joint contraction), out = W' G + sum_k bW_k rowsum(A_k)
//   bwd: dW' = dout G^T, H = W'^T dout, dx = sum_k H_k A_k,
//        dA = sum H_k^T x + bias part, dbW = sum dout rowsum(A_k)
// ---------------------------------------------------------------------------
namespace {

// A block descriptor with the spatial shape (stride 1; the temporal fields
// only satisfy the planner).
stgcn_desc_t spatial_as_block(const stgcn_spatial_desc_t *sd) {
  stgcn_desc_t d{};
  d.N = sd->N;
  d.C_in = sd->C_in;
  d.C_out = sd->C_out;
  d.T = sd->T;
  d.T_out = sd->T;
  d.V = sd->V;
  d.K = sd->K;
  d.gamma = 9;
  d.stride = 1;
  d.pad = 4;
  d.eps = 1e-5f;
  d.momentum = 0.1f;
  d.training = 1;
  d.need_dx = 1;
  d.flags = sd->flags & STGCN_F_BF16;
  return d;
}

int spatial_check(const stgcn_spatial_desc_t *sd, stgcn_desc_t *d) {
  if (!sd) return fail(STGCN_E_INVALID, "null descriptor");
  if (sd->flags & ~STGCN_F_BF16) return fail(STGCN_E_UNSUPPORTED, "unknown spatial flags");
  *d = spatial_as_block(sd);
  return stgcn_check_desc(d);
}

hipError_t fill_identity_bn(float *ident, int C, hipStream_t s, BnRef *bn) {
  *bn = bn_packed(ident, C);
  hipError_t e = hipMemsetD32Async((hipDeviceptr_t)ident, 0u, (size_t)C, s);  // mean 0
  if (e == hipSuccess)  // invstd 1, gamma 1
    e = hipMemsetD32Async((hipDeviceptr_t)(ident + C), 0x3f800000u, (size_t)2 * C, s);
  if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)(ident + 3 * C), 0u, (size_t)C, s);
  return e;
}

}  // namespace

extern "C" {

size_t stgcn_spatial_workspace_bytes(const stgcn_spatial_desc_t *sd, int backward) {
  stgcn_desc_t d;
  if (spatial_check(sd, &d) != STGCN_OK) return 0;
  return spatial_layout(&d, nullptr, backward != 0).total;
}

int stgcn_spatial_fwd(const stgcn_spatial_desc_t *sd, const float *x, const float *A,
                      const float *W, const float *bW, float *out, void *workspace,
                      size_t workspace_bytes, void *stream) {
  stgcn_desc_t dd;
  int rc = spatial_check(sd, &dd);
  if (rc) return rc;
  const stgcn_desc_t *d = &dd;
  if (!x || !A || !W || !bW || !out) return fail(STGCN_E_INVALID, "null tensor argument");
  // the alignment contract (stgcn_hip.h): the fp32 path reads x, A, W, bW at their
  // natural alignment (a misaligned x takes k_gather3 / k_gather_fwd, the rest is
  // read one element at a time); the bf16 kernels are given 16 bytes throughout
  if ((rc = check_aligned({NamedPtr{x, "x"}, NamedPtr{A, "A"}, NamedPtr{W, "W"}, NamedPtr{bW, "bW"}},
                          bf16(d) ? 16 : 4)) ||
      (rc = check_aligned({NamedPtr{out, "out"}, NamedPtr{workspace, "workspace"}}, 16)))
    return rc;
  const SpatialLayout L = spatial_layout(d, workspace, false);
  if (!workspace || workspace_bytes < L.total) return fail(STGCN_E_INVALID, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int C = d->C_in, R = d->C_out, V = d->V, K = d->K;
  BnRef ident;
  HIP_TRY(fill_identity_bn(L.ident, C, s, &ident));
  HIP_TRY(launch_bias_rv(A, bW, L.biasZ, K, R, V, s));
  const float *Wz = W;
  if (K > 1) {
    HIP_TRY(launch_pack_w(W, L.Wpk, K, R, C, s));
    Wz = L.Wpk;
  }
  SpatialFwd f = spatial_fwd(d, x, ident, A);
  f.G = L.G;
  HIP_TRY(launch_gather_fwd(f, s));
  HIP_TRY(launch_conv_gemm(spatial_gemm(d, L.G, Wz, out, L.biasZ, L.wpk), s));
  return STGCN_OK;
}

int stgcn_spatial_bwd(const stgcn_spatial_desc_t *sd, const float *dout, const float *x,
                      const float *A, const float *W, const float *bW, float *dx, float *dA,
                      float *dW, float *dbW, void *workspace, size_t workspace_bytes,
                      void *stream) {
  stgcn_desc_t dd;
  int rc = spatial_check(sd, &dd);
  if (rc) return rc;
  const stgcn_desc_t *d = &dd;
  if (!dout || !x || !A || !W || !bW || !dA || !dW || !dbW)
    return fail(STGCN_E_INVALID, "null tensor argument");
  // (as stgcn_spatial_fwd; a misaligned dout takes k_sum_nt, the 4-byte staging of
  // k_wgrad_sp and the 4-byte input DMA of the H GEMM, a misaligned x k_gather3 and
  // k_spatial_bwd3 / k_spatial_dx)
  if ((rc = check_aligned({NamedPtr{dout, "dout"}, NamedPtr{x, "x"}, NamedPtr{A, "A"},
                           NamedPtr{W, "W"}, NamedPtr{bW, "bW"}},
                          bf16(d) ? 16 : 4)) ||
      (rc = check_aligned({NamedPtr{dx, "dx"}, NamedPtr{dA, "dA"}, NamedPtr{dW, "dW"},
                           NamedPtr{dbW, "dbW"}, NamedPtr{workspace, "workspace"}},
                          16)))
    return rc;
  const SpatialLayout L = spatial_layout(d, workspace, true);
  if (!workspace || workspace_bytes < L.total) return fail(STGCN_E_INVALID, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int N = d->N, C = d->C_in, R = d->C_out, T = d->T, V = d->V, K = d->K;
  BnRef ident;
  HIP_TRY(fill_identity_bn(L.ident, C, s, &ident));
  HIP_TRY(hipMemsetAsync(L.sd, 0, sizeof(double) * C, s));
  HIP_TRY(hipMemsetAsync(L.sdn, 0, sizeof(double) * C, s));
  HIP_TRY(hipMemsetAsync(L.SdZ, 0, sizeof(double) * R * V, s));
  SpatialFwd f = spatial_fwd(d, x, ident, A);
  f.G = L.G;
  HIP_TRY(launch_gather_fwd(f, s));
  {
    WgradParams w = wgrad_spatial(d, dout, L.G, L.slab);
    HIP_TRY(launch_wgrad(w, s));
    HIP_TRY(launch_slab_reduce(L.slab, w.S, (int64_t)R * K * C, dW, 1, R, K, C, s));
  }
  HIP_TRY(launch_sum_nt(dout, N, R, T, V, L.SdZ, s));
  HIP_TRY(launch_spatial_small(L.SdZ, A, bW, K, R, V, dbW, dA, s));
  const float *Wz = W;
  if (K > 1) {
    HIP_TRY(launch_pack_w(W, L.Wpk, K, R, C, s));
    Wz = L.Wpk;
  }
  HIP_TRY(launch_conv_gemm(h_gemm(d, dout, Wz, L.H, L.wpk), s));
  // dx = sum_k H_k A_k (BatchNorm identity: dx is dxhat; sd/sdn unused)
  SpatialBwd b = spatial_bwd(d, L.H, x, ident, A, dx, dA, L.sd, L.sdn);
  b.write_dx = dx != nullptr;
  HIP_TRY(launch_spatial_dx(b, s));
  return STGCN_OK;
}

}  // extern "C"
