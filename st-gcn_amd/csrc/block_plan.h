// The planner of the C-ABI layer (host only; included by capi.hip alone): for a
// block descriptor, which kernel path runs (the path predicates), where every
// workspace tensor lies (the layouts) and the parameters of every GEMM launch
// (the builders, one per kind of GEMM). capi.hip holds the entry points and
// their stages, which set on a built launch only what is particular to the call.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/stgcn_hip.h"
#include "internal.h"

namespace stgcn {

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// Frames per conv tile: as many whole frames as fit 256 columns.
inline int conv_ft(int V) { return std::max(1, kTileCols / V); }
// Frames per wgrad work item: as many whole frames as fit 80 columns.
inline int wgrad_ft(int V) { return std::max(1, 80 / V); }

inline int64_t nT(const stgcn_desc_t *d) { return (int64_t)d->T * d->V; }
inline int64_t nTo(const stgcn_desc_t *d) { return (int64_t)d->T_out * d->V; }
inline bool residual(const stgcn_desc_t *d) { return (d->flags & STGCN_F_RESIDUAL) != 0; }
inline bool bf16(const stgcn_desc_t *d) { return (d->flags & STGCN_F_BF16) != 0; }
inline bool f32x3(const stgcn_desc_t *d) { return (d->flags & STGCN_F_F32X3) != 0; }
inline bool f16x2_flag(const stgcn_desc_t *d) { return (d->flags & STGCN_F_F16X2) != 0; }

// ---- Path predicates that the descriptor alone decides ----

// the fused spatial forward (kernels_fused.hip) of the bf16 path applies (other
// shapes: the unfused gather + GEMM kernels)
inline bool fused_sp(const stgcn_desc_t *d) {
  return bf16(d) && sp_fwd_bf16_supported(d->C_in, d->V, d->K, d->C_out, residual(d));
}
// the fused spatial backward (kernels_spbwd.hip) applies: bf16 path only (other
// shapes, and the fp32 split path: the H GEMM + k_spatial_bwd5/6 pair, which at
// K = 1 measured faster than an exact-split fused kernel, cfg2 L1 281 vs 351 us)
inline bool fused_spb(const stgcn_desc_t *d) {
  return bf16(d) && !f32x3(d) &&
         sp_bwd_fused_supported(d->C_in, d->V, d->K, d->C_out, d->T);
}
// the fused backward of the two-person graph: two kernels (k_sp50_dx, k_sp50_dA),
// timed apart as which 5 / 6
inline bool fused_spb50(const stgcn_desc_t *d) { return fused_spb(d) && d->V == 50; }
// The folded block (kernels_fold.hip): with one adjacency partition the
// SpatialConv channel GEMM W' folds into the temporal conv's weights
// (Wc_q = Wt_q W'), so the temporal conv reads G = BN1(x) A^T (C_in channels)
// and Z / dZ are never formed; the backward's data gradient yields H directly.
// fp32 split path, K = 1: V = 18 (cfg2) and V = 25 (the reference's default
// L_STGCN graph: NTU joints, unilabeling partition, lightning_model.py:271),
// non-residual blocks over >= 16 input and output channels (the data gradient
// reduces over C_out: k_conv_x3 needs >= 16 there); every other block runs the
// unfolded kernels.
inline bool fold_w(const stgcn_desc_t *d) {
  return f32x3(d) && !residual(d) && d->K == 1 && d->C_in >= 16 && d->C_out >= 16 &&
         (d->V == 18 || d->V == 25);
}
// The folded block's SpatialConv backward inside its data gradient (kernels_x3.hip
// spb_epilogue, V = 18): dxhat = H A, dA, the BN1 / chain sums from the tile
// while H is on chip. V = 25: the data gradient stores H and the unfused spatial
// backward (k_spatial_bwd5) reads it.
inline bool fold_spb(const stgcn_desc_t *d) { return fold_w(d) && d->V == 18; }

// The folded block's temporal GEMMs on 2-way fp16 splits (STGCN_F_F16X2; k_conv_x3 /
// k_wgrad_x3 with NPL = 2), operand scales from max |x| words (launch_absmax)
inline bool f16x2(const stgcn_desc_t *d) { return fold_w(d) && f16x2_flag(d); }
// ... and the unfolded K = 1 split block (the first block: C_in < 16) with its
// temporal conv forward and weight gradient on fp16 splits: max |Z| by a pass
// over Z, kept after G for the backward;
// its data gradient stays on the 3-way splits (it feeds BN1's nearly cancelling sums)
inline bool f16x2_unfold(const stgcn_desc_t *d) {
  return f16x2_flag(d) && f32x3(d) && !fold_w(d) && !residual(d) && d->K == 1 && d->V == 18 &&
         d->C_out >= 16;
}
// the temporal forward / weight gradient on fp16 splits (folded or not)
inline bool f16x2_tw(const stgcn_desc_t *d) { return f16x2(d) || f16x2_unfold(d); }
// ... the data gradient included: its output feeds BN1's sum of dxhat over N T V
// elements of a zero-mean dU (heavy cancellation; the 2^-22 operand
// representation measured 2.5x the fp32 reference's own error on the BN1 bias
// gradient at N = 32, T = 300), which the folded block takes from the fp64 dU
// sums instead (kernels_fold.hip k_fold_sd).
// (only where BN1's sum comes from the fp64 dU sums: the fused backward, fold_spb;
// elsewhere the data gradient stays on the 3-way bf16 splits)
inline bool f16x2_dgrad(const stgcn_desc_t *d) { return f16x2(d) && fold_spb(d); }
inline int fold_fwd_npl(const stgcn_desc_t *d) { return f16x2(d) ? 2 : 3; }
inline int fold_dgrad_npl(const stgcn_desc_t *d) { return f16x2_dgrad(d) ? 2 : 3; }

// sum_{n,t} dZ of the non-residual block from per-tap sums of dU (clip-chunk
// sums written by the ReLU + BN2 backward apply, k_fold_tq, one small GEMM with
// Wt) instead of a pass over dZ (the folded block has no dZ at all): cfg3 5632
// vs 5604, cfg5 2658 vs 2631 clips/s in one A/B call. Residual blocks still
// make the pass over dZ.
inline bool cols_sums(const stgcn_desc_t *d) { return !residual(d); }
// The folded forward leaves Wc in the (otherwise unused) Z buffer for the
// backward when it fits (Z is opaque to the caller under STGCN_F_F32X3 then)
inline bool fold_wc_in_z(const stgcn_desc_t *d) {
  return fold_w(d) && (int64_t)d->N * d->C_out * d->T * d->V >= (int64_t)d->C_out * d->C_in * 9;
}
// residual block with a 1x1 projection (apply_residual Conv2d, st_graphconv.py:27)
inline bool projection(const stgcn_desc_t *d) {
  return residual(d) && (d->C_in != d->C_out || d->stride != 1);
}

// ---- Builders: the launch parameters of each kind of GEMM, once ----
// Pure functions of the descriptor and the operand pointers (null pointers: a
// "supported?" or a size question); the ConvGemmParams come back tiled. A call
// site adds only what is its own: the epilogue extras (bias_r, stat_*, res,
// relu_out, drop), the operands' storage format (in_bf16), the f16x2 bound
// pointers, the spb / bna operand block, dA_part and wpk_ready. The spatial
// launches' descriptors follow the same rule (spatial_fwd / spatial_bwd below).

inline ConvGemmParams conv_base(const stgcn_desc_t *d, float *wpk) {
  ConvGemmParams p{};
  p.wpk = wpk;
  p.V = d->V;
  p.FT = conv_ft(d->V);
  p.N = d->N;
  p.bf16 = bf16(d) ? 1 : (f32x3(d) ? 3 : 0);
  return p;
}

inline void conv_tiles(ConvGemmParams &p) {
  p.n_mtiles = (p.M + p.FT - 1) / p.FT;
  p.n_rtiles = (p.R + kTileRows - 1) / kTileRows;
}

// The one-tap channel GEMMs, out[n, r, s_out*m] = sum_c W[r][c] in[n, c, s_in*m] for
// m < M: in holds C channels of T_in frames, out R rows of T_o frames; wT: w is
// stored transposed ([C][R]: the data-gradient side of a weight)
inline ConvGemmParams gemm_1x1(const stgcn_desc_t *d, const float *in, const float *w, float *out,
                               float *wpk, int C, int T_in, int s_in, int R, int T_o, int s_out,
                               int M, bool wT) {
  ConvGemmParams p = conv_base(d, wpk);
  p.in = in;
  p.w = w;
  p.out = out;
  p.in_bstride = (int64_t)C * T_in * d->V;
  p.out_bstride = (int64_t)R * T_o * d->V;
  p.w_sr = wT ? 1 : C;
  p.w_sc = wT ? R : 1;
  p.w_sq = 0;
  p.C = C;
  p.R = R;
  p.NQ = 1;
  p.s_in = s_in;
  p.off = 0;
  p.s_out = s_out;
  p.p_out = 0;
  p.M = M;
  p.T_src = T_in;
  p.T_dst = T_o;
  conv_tiles(p);
  return p;
}

// Spatial channel GEMM Z = W' G + biasZ over the K * C_in channels of G
// (Wz: W for K = 1, else the packed [W_0 | ... | W_{K-1}], launch_pack_w)
inline ConvGemmParams spatial_gemm(const stgcn_desc_t *d, const float *G, const float *Wz, float *Z,
                                   const float *biasZ, float *wpk) {
  ConvGemmParams p = gemm_1x1(d, G, Wz, Z, wpk, d->K * d->C_in, d->T, 1, d->C_out, d->T, 1,
                              d->T, false);
  p.bias_rv = biasZ;
  return p;
}

// H = W'^T dZ for all partitions in one GEMM (rows k*C_in + ci of H are
// the channels of H_k): dZ is read once instead of K times
inline ConvGemmParams h_gemm(const stgcn_desc_t *d, const float *dZ, const float *Wz, float *H,
                             float *wpk) {
  return gemm_1x1(d, dZ, Wz, H, wpk, d->C_out, d->T, 1, d->K * d->C_in, d->T, 1, d->T, true);
}

// The residual projection (apply_residual: Conv2d(C_in, C_out, 1, stride (s,1)),
// st_graphconv.py:27): Rp = Wr x + br at the strided frames ...
inline ConvGemmParams proj_fwd(const stgcn_desc_t *d, const float *x, const float *Wr, float *Rp,
                               const float *br, float *wpk) {
  ConvGemmParams p = gemm_1x1(d, x, Wr, Rp, wpk, d->C_in, d->T, d->stride, d->C_out, d->T_out, 1,
                              d->T_out, false);
  p.bias_r = br;
  return p;
}
// ... and its data gradient Rg[ci](s*m) = sum_co Wr[co][ci] dU[co](m) (the other
// frames of Rg are not written: the caller zeroes it)
inline ConvGemmParams proj_dgrad(const stgcn_desc_t *d, const float *dU, const float *Wr, float *Rg,
                                 float *wpk) {
  return gemm_1x1(d, dU, Wr, Rg, wpk, d->C_out, d->T_out, 1, d->C_in, d->T, d->stride, d->T_out,
                  true);
}

// Temporal (9,1) conv forward, stride (s,1), pad (4,0), over Cred input channels
// of w [C_out][Cred][9]: C_out (Z in, Wt), or C_in for the folded block (G in, Wc).
// Everything but the w4 mark, which asks fold_bna, which asks this.
inline ConvGemmParams tconv_fwd_unmarked(const stgcn_desc_t *d, int Cred, const float *in,
                                         const float *w, float *out, float *wpk) {
  const int R = d->C_out;
  ConvGemmParams p = conv_base(d, wpk);
  p.in = in;
  p.w = w;
  p.out = out;
  p.in_bstride = (int64_t)Cred * nT(d);
  p.out_bstride = (int64_t)R * nTo(d);
  p.w_sr = (int64_t)Cred * 9;
  p.w_sc = 9;
  p.w_sq = 1;
  p.C = Cred;
  p.R = R;
  p.NQ = 9;
  p.s_in = d->stride;
  p.off = -d->pad;
  p.s_out = 1;
  p.p_out = 0;
  p.M = d->T_out;
  p.T_src = d->T;
  p.T_dst = d->T_out;
  conv_tiles(p);
  return p;
}

// ... and G never formed (north star N1; kernels_x3.hip bna_contract): the
// forward GEMM reads x, applies BN1 in its window loader and the joint
// contraction with A in its epilogue (U = A U' + BT), the weight gradient reads
// x (BN1 at staging) against dU A (written by the ReLU + BN2 backward apply
// pass), so the gather kernel and G's HBM round trips are gone
// Opt-in (STGCN_F_NO_G, the memory-lean mode: G is not kept between forward and
// backward): measured 4% slower per cfg2 step than forming G once with k_gather4
//  -- the joint contraction then runs on the VALU inside
// latency-bound GEMM kernels instead of inside an HBM-bound pass.
inline bool fold_bna(const stgcn_desc_t *d) {
  if (!f16x2(d) || !(d->flags & STGCN_F_NO_G)) return false;
  return conv_x3_bna_supported(
      tconv_fwd_unmarked(d, d->C_in, nullptr, nullptr, nullptr, nullptr));
}
// The fp16-split stride-1 temporal forward (folded, or the unfolded first
// block) on 4-wave 64-row tiles, two workgroups per CU (kernels_x3.hip x3_w4):
// marks the GEMM's parameters wherever its weights are packed or it is launched
inline bool fwd_w4(const stgcn_desc_t *d) {
  return d->stride == 1 && ((f16x2(d) && !fold_bna(d)) || f16x2_unfold(d));
}

inline ConvGemmParams tconv_fwd(const stgcn_desc_t *d, int Cred, const float *in, const float *w,
                                float *out, float *wpk) {
  ConvGemmParams p = tconv_fwd_unmarked(d, Cred, in, w, out, wpk);
  p.w4 = fwd_w4(d) ? 1 : 0;
  return p;
}

// Temporal conv data gradient dIn = conv^T(dU) with the flipped taps of
// w [C_out][Crows][9] (Crows output rows: C_out for dZ with Wt, or C_in for the
// folded block's H with Wc). Stride 1: one launch; stride 2: phase 0 (even
// output frames, taps 8, 6, .., 0) and phase 1 (odd frames, taps 7, .., 1).
// A phase with M <= 0 frames (T = 1) is not launched: the caller skips it.
inline int tconv_dgrad_phases(const stgcn_desc_t *d) { return d->stride == 1 ? 1 : 2; }
inline ConvGemmParams tconv_dgrad(const stgcn_desc_t *d, int Crows, int ph, const float *dU,
                                  const float *w, float *out, float *wpk) {
  const int R = d->C_out, T = d->T;
  ConvGemmParams p = conv_base(d, wpk);
  p.in = dU;
  p.out = out;
  p.in_bstride = (int64_t)R * nTo(d);
  p.out_bstride = (int64_t)Crows * nT(d);
  p.w_sr = 9;
  p.w_sc = (int64_t)Crows * 9;
  p.C = R;
  p.R = Crows;
  p.T_src = d->T_out;
  p.T_dst = T;
  p.s_in = 1;
  if (d->stride == 1) {
    p.w = w ? w + 8 : nullptr;
    p.w_sq = -1;
    p.NQ = 9;
    p.off = -4;
    p.s_out = 1;
    p.p_out = 0;
    p.M = T;
  } else {
    p.w = w ? w + (ph == 0 ? 8 : 7) : nullptr;
    p.w_sq = -2;
    p.NQ = ph == 0 ? 5 : 4;
    p.off = ph == 0 ? -2 : -1;
    p.s_out = 2;
    p.p_out = ph;
    p.M = ph == 0 ? (T + 1) / 2 : T / 2;
  }
  conv_tiles(p);
  return p;
}

inline int wgrad_splits(int tiles, int items) {
  int S = (512 + tiles - 1) / tiles;
  return std::max(1, std::min(S, items));
}

// The plan of a one-tap weight gradient (wgrad_spatial, wgrad_proj below)
inline WgradParams make_wgrad(const stgcn_desc_t *d, const float *P, int64_t pb, int R, int Mframes,
                              const float *Q, int64_t qb, int C, int T_src, int NQ, int s_in,
                              int off, float *slab) {
  WgradParams w{};
  w.P = P;
  w.Q = Q;
  w.slab = slab;
  w.p_bstride = pb;
  w.q_bstride = qb;
  w.R = R;
  w.C = C;
  w.NQ = NQ;
  w.s_in = s_in;
  w.off = off;
  w.M = Mframes;
  w.T_src = T_src;
  w.V = d->V;
  w.FT = wgrad_ft(d->V);
  while (w.FT > 1 && wgrad_lds_bytes(w) > 80 * 1024) --w.FT;  // 2 workgroups per CU
  w.n_mtiles = (Mframes + w.FT - 1) / w.FT;
  w.n_rtiles = (R + 63) / 64;
  w.n_jtiles = wgrad_ntiles_j(C, NQ);
  w.N = d->N;
  w.S = wgrad_splits(w.n_rtiles * w.n_jtiles, d->N * w.n_mtiles);
  if (wgrad_sp_applies(w)) plan_wgrad_sp(w);
  if (bf16(d)) plan_wgrad_bf16(w);  // k_wgrad_bf16 where it covers the shape
  // fp32 path of STGCN_F_F32X3: the spatial dW' on exact bf16 splits (k_wgrad_sp<.., X3>)
  if (f32x3(d) && wgrad_sp_applies(w)) w.bf16 = 3;
  return w;
}

// Spatial weight gradient dW' = dZ G^T (slab [S][C_out][K*C_in], split-K)
inline WgradParams wgrad_spatial(const stgcn_desc_t *d, const float *dZ, const float *G,
                                 float *slab) {
  const int KC = d->K * d->C_in, R = d->C_out;
  return make_wgrad(d, dZ, (int64_t)R * nT(d), R, d->T, G, (int64_t)KC * nT(d), KC, d->T, 1, 1, 0,
                    slab);
}
// Projection weight gradient dWr[co][ci] = sum dU[co](m) x[ci](s*m)
inline WgradParams wgrad_proj(const stgcn_desc_t *d, const float *dU, const float *x, float *slab) {
  const int C = d->C_in, R = d->C_out;
  return make_wgrad(d, dU, (int64_t)R * nTo(d), R, d->T_out, x, (int64_t)C * nT(d), C, d->T, 1,
                    d->stride, 0, slab);
}
// dW' from the bf16 G kept by the fused forward (k_sp_fwd_bf16) -> k_wgrad_gemm_gk
inline WgradParams wgrad_gk(const stgcn_desc_t *d, const float *dZ, const float *Gk, float *slab) {
  WgradParams w{};
  w.P = dZ;
  w.Q = Gk;
  w.slab = slab;
  w.p_bstride = (int64_t)d->C_out * nT(d);
  w.R = d->C_out;
  w.C = d->K * d->C_in;
  w.NQ = 1;
  w.s_in = 1;
  w.M = d->T;
  w.T_src = d->T;
  w.V = d->V;
  w.N = d->N;
  plan_wgrad_gk(w, d->T);
  return w;
}

// Temporal-conv weight gradient plan (k_wgrad_taps): dWt = sum dU (x) Z(shifted).
// (Cq: channels of the Q operand, C_out; C_in for the folded block's dWc = sum dU G^T)
inline WgradParams make_wgrad_taps(const stgcn_desc_t *d, const float *dU, const float *Z,
                                   float *slab, int Cq = 0) {
  const int R = d->C_out;
  if (Cq <= 0) Cq = R;
  WgradParams w{};
  w.P = dU;
  w.Q = Z;
  w.slab = slab;
  w.p_bstride = (int64_t)R * d->T_out * d->V;
  w.q_bstride = (int64_t)Cq * d->T * d->V;
  w.R = R;
  w.C = Cq;
  w.NQ = 9;
  w.s_in = d->stride;
  w.off = -d->pad;
  w.M = d->T_out;
  w.T_src = d->T;
  w.V = d->V;
  w.N = d->N;
  w.FT = std::max(1, 80 / d->V);
  while (w.FT > 1 && !wgrad_taps_supported(w)) --w.FT;
  w.n_mtiles = (w.M + w.FT - 1) / w.FT;
  w.n_rtiles = (R + 63) / 64;
  w.n_jtiles = (Cq + wgrad_taps_cb(w) - 1) / wgrad_taps_cb(w);
  const int tiles = w.n_rtiles * w.n_jtiles;
  w.S = std::max(1, std::min((256 + tiles - 1) / tiles, d->N * w.n_mtiles));
  if (bf16(d)) plan_wgrad_bf16(w);
  // k_wgrad_x3 where it covers the shape (its S x R x C x 9 slab fits the fp32
  // plan's: twice the tiles, half the splits)
  if (f32x3(d)) plan_wgrad_x3(w, f16x2_tw(d));
  return w;
}

// x = ReLU(BN2_prev(U_prev)) of the previous block (ABI 8; PrevBn in internal.h):
// its statistics [mean | invstd] over C channels, gamma2 and beta2
inline PrevBn prev_bn(const float *prev_stats, int C, const float *g2, const float *b2) {
  PrevBn pv;
  pv.bn = bn_ref(prev_stats, C, g2, b2);
  return pv;
}

// The spatial launches (internal.h SpatialFwd / SpatialBwd): the shape, BN1 and
// the residual block's ReLU on BN1(x) from the descriptor. A call site adds what
// is its own: the outputs of the kernel it launches (G, amax | W, biasZ, wpk, Z,
// Gk, the Z sums), prev, the dA partial slots, only.
inline SpatialFwd spatial_fwd(const stgcn_desc_t *d, const float *x, const BnRef &bn1,
                              const float *A) {
  SpatialFwd f;
  f.x = x;
  f.bn = bn1;
  f.A = A;
  f.N = d->N;
  f.C = d->C_in;
  f.R = d->C_out;
  f.T = d->T;
  f.V = d->V;
  f.K = d->K;
  f.relu = residual(d) ? 1 : 0;
  return f;
}
// in: dZ (launch_sp_bwd_fused, with W and wpk) or H = W'^T dZ (launch_spatial_dx)
inline SpatialBwd spatial_bwd(const stgcn_desc_t *d, const float *in, const float *x,
                              const BnRef &bn1, const float *A, float *dx, float *dA, double *sd,
                              double *sdn) {
  SpatialBwd b;
  b.in = in;
  b.x = x;
  b.bn = bn1;
  b.A = A;
  b.dx = dx;
  b.dA = dA;
  b.sd = sd;
  b.sdn = sdn;
  b.N = d->N;
  b.C = d->C_in;
  b.R = d->C_out;
  b.T = d->T;
  b.V = d->V;
  b.K = d->K;
  b.write_dx = d->need_dx;
  b.relu = residual(d) ? 1 : 0;
  b.bf16ops = bf16(d) ? 1 : 0;
  return b;
}

// ---- Path predicates that ask a built launch ----

// ABI 8 (STGCN_PLAN_X_FROM_U): the training forward of a folded block that forms
// G (k_gather4) can read its input as ReLU(BN2_prev(U_prev)) of the previous
// block -- that block then writes only y's statistics, not y -- and its fused
// backward (spb_epilogue, deferred dx) already reads U_prev in place of x
// The bf16 blocks (cfg3 / cfg5) too (verdict r5 item 4): their fused spatial
// forward (k_sp_fwd_bf16 / k_sp_fwd_wide) forms ReLU(BN2_prev(U_prev)) on
// staging, and their spatial backward (k_sp_bwd_fused, k_sp50_*, or the H GEMM
// + joint kernel) reads U_prev in prev mode wherever dx defers; the weight
// gradient of W' reads the kept bf16 G -- so x is read by nothing.
inline bool x_from_u(const stgcn_desc_t *d) {
  if (!d->training || residual(d)) return false;
  if (fused_sp(d))
    return fused_spb(d) || spatial_dx_prev_supported(d->N, d->C_in, d->T, d->V, d->K);
  return fold_spb(d) && !fold_bna(d) && d->K == 1 && gather_prev_supported(d->C_in, d->T, d->V);
}
// STGCN_PLAN_X_FROM_U_EVAL: the same input form in the eval forward (training ==
// 0). BN1 and BN2 are per-channel constants there and no backward follows, so
// only the forward kernels decide: the bf16 fused spatial forward stages
// ReLU(BN2_prev(U_prev)) whatever the partition count, and any folded block that
// forms G (V = 18 and V = 25) runs k_gather4 in prev mode where its blocks do
// not cross a clip.
inline bool x_from_u_eval(const stgcn_desc_t *d) {
  if (d->training || residual(d)) return false;
  if (fused_sp(d)) return true;
  return fold_w(d) && !fold_bna(d) && gather_prev_supported(d->C_in, d->T, d->V);
}

// The folded training forward's BN2 statistics as per-tile partials
// (k_conv_x3's row-major epilogue; ConvGemmParams.stat_part)
inline bool fold_stat_parts(const stgcn_desc_t *d) {
  return fold_w(d) && d->training &&
         conv_x3_supported(tconv_fwd(d, d->C_in, nullptr, nullptr, nullptr, nullptr));
}

inline int fold_stat_tiles(const stgcn_desc_t *d) {
  return d->N * ((d->T_out + conv_ft(d->V) - 1) / conv_ft(d->V));
}

// (the block takes a prep buffer: folded, with split-plane forward and data gradient)
inline bool prep_applies(const stgcn_desc_t *d) {
  if (!fold_w(d)) return false;
  if (!conv_x3_supported(tconv_fwd(d, d->C_in, nullptr, nullptr, nullptr, nullptr))) return false;
  for (int ph = 0; ph < tconv_dgrad_phases(d); ++ph)
    if (!conv_x3_supported(tconv_dgrad(d, d->C_in, ph, nullptr, nullptr, nullptr, nullptr)))
      return false;
  return true;
}

// Activations stored in bf16 on the bf16 path's non-residual blocks: Z (the
// SpatialConv output) and dU (the gradient at the temporal conv output). Every
// reader of them rounds them to bf16 anyway -- Z: the temporal conv forward
// (k_conv_x3 one-plane) and the weight gradient's Q (k_wgrad_bf16); dU: the
// data gradient (k_conv_x3 one-plane, stride-2 phases included) and the weight
// gradient's P -- so the results are bit-identical to fp32 storage and half
// the bytes move; the bias / BN gradients use the fp32 sums of the producing
// passes. The tensors keep their fp32-sized buffers (the first half holds the
// bf16 data). Producers: the fused spatial forward's epilogues (so C_in >= 16)
// and the BN2 + ReLU backward pass. (fp32 storage there measured slower: cfg3
// 5,831 vs 5,948 and cfg5 2,528 vs 2,731 clips/s.)
inline bool act_bf16(const stgcn_desc_t *d) {
  // Stride-2 blocks at odd V keep fp32: their weight gradient (k_wgrad_bf16<9,V,2>)
  // staged bf16 pairs by registers slower than fp32 (cfg5 2.19 -> 2.66 ms per
  // step), more than the strided forward and data-gradient phases gained; at even
  // V it stages them by LDS-DMA (fp32 there: cfg5 2592 vs 2644 clips/s).
  const bool s2 = d->stride == 2 && d->V % 2 == 0;
  if (!fused_sp(d) || residual(d) || (d->stride != 1 && !s2)) return false;
  // the temporal conv forward and data gradient
  if (!conv_b1_supported(tconv_fwd(d, d->C_out, nullptr, nullptr, nullptr, nullptr))) return false;
  WgradParams w = make_wgrad_taps(d, nullptr, nullptr, nullptr);
  return w.bf16 == 1;
}
inline bool z_bf16(const stgcn_desc_t *d) { return act_bf16(d); }
inline bool du_bf16(const stgcn_desc_t *d) { return act_bf16(d); }

// dZ (the gradient at the SpatialConv output) stays in fp32 on every path:
// bf16 storage measured slower in one A/B call (cfg3 5285 vs 5415, cfg5 2126 vs
// 2137 clips/s).

// Every GEMM launch of the block fits its LDS budget.
inline bool geometry_supported(const stgcn_desc_t *d) {
  WgradParams w1 = make_wgrad_taps(d, nullptr, nullptr, nullptr);
  WgradParams w2 = wgrad_spatial(d, nullptr, nullptr, nullptr);
  if (!(w1.bf16 || wgrad_taps_supported(w1)) || !(w2.bf16 || wgrad_supported(w2))) return false;
  if (!conv_gemm_supported(tconv_fwd(d, d->C_out, nullptr, nullptr, nullptr, nullptr)))
    return false;
  if (!conv_gemm_supported(spatial_gemm(d, nullptr, nullptr, nullptr, nullptr, nullptr)))
    return false;
  if (projection(d)) {  // the strided 1x1 projection
    WgradParams w3 = wgrad_proj(d, nullptr, nullptr, nullptr);
    if (!conv_gemm_supported(proj_fwd(d, nullptr, nullptr, nullptr, nullptr, nullptr)) ||
        !(w3.bf16 || wgrad_sp_applies(w3) || wgrad_supported(w3)))
      return false;
  }
  return true;
}

// ---- Layouts: where each tensor of a workspace lies (base null: sizes only) ----

struct Carve {
  char *base;
  size_t off = 0;
  explicit Carve(void *b) : base((char *)b) {}
  template <class T>
  T *take(size_t count) {
    T *p = base ? (T *)(base + off) : nullptr;
    off += align_up(count * sizeof(T));
    return p;
  }
};

// Upper bound of the packed-weight scratch any conv_gemm launch of this block needs.
inline size_t wpk_floats(const stgcn_desc_t *d) {
  const int rows = std::max(d->C_out, d->K * d->C_in);  // (stacked H GEMM: K*C_in rows)
  const int red = std::max(d->C_out, d->K * d->C_in);
  // reduction padded to a whole number of chunks for any chunk size <= 32
  size_t n = (size_t)((rows + 63) / 64 * 64) * ((red + 31) / 32 * 32 + 32) * 9;
  // STGCN_F_F32X3: three bf16 planes of the weights (1.5x the fp32 floats)
  if (d->flags & STGCN_F_F32X3) n *= 2;
  // the fused bf16 spatial forward: packed W' + the A image
  if (d->flags & STGCN_F_BF16)
    n = std::max(n, (sp_fwd_bf16_wpk_bytes(d->C_in, d->C_out, d->K, d->V) + 3) / 4);
  // the fused spatial backward: packed W' + its A image
  if (d->flags & STGCN_F_BF16)
    n = std::max(n, (sp_bwd_fused_wpk_bytes(d->C_in, d->C_out, d->K, d->V) + 3) / 4);
  return n;
}

struct BwdLayout {
  double *sg, *sgu, *sdu, *sd, *sdn, *SdZ;
  double *s1, *s2;  // deferred-dx chain: the prev-mode sums of the spatial backward
  unsigned *amax;
  float *dU, *dZ, *G, *H, *slab, *wpk;
  float *Wpk;  // W' = [W_0 | ... | W_{K-1}] (C_out, K*C_in) for the stacked H GEMM
  float *Rg;  // residual projection data-grad (N, C_in, T, V)
  // the folded block: dU summed over clips, per-tap sums Tq, dWc, partials, Wc, bZ
  double *fcs, *ftq, *f64scr, *SdH;
  float *dWc, *fscr;  // the fold GEMMs' operand re-layouts (kernels_fold.hip)
  float *Wc, *bZ;
  // deterministic dA: the spatial backward's per-workgroup partials (dA_cap
  // slots of K V V floats) and the reduction's fp64 scratch
  float *dApart;
  double *dAlvl;
  int64_t dA_cap;
  size_t dbl_bytes, total;
};

// Partial slots the block's dA-producing launches need (0: fp32 atomics stay):
// the folded data gradient's workgroups (spb_epilogue; both stride-2 phases,
// counted at 64-row tiles: an upper bound), or the unfused spatial backward's
// joint kernel -- persistent k_spatial_bwd5 (<= 2048 workgroups) / _bwd6 (two
// slots per workgroup, <= 512), or the flat-row k_spatial_bwd3 (>= 64 rows per
// workgroup). (The fused bf16 spatial backward kernels keep their atomics.)
inline int64_t dA_part_cap(const stgcn_desc_t *d) {
  const int64_t N = d->N, C = d->C_in, T = d->T;
  if (fold_spb(d)) {
    const int FT = conv_ft(d->V);
    const int64_t mt = d->stride == 1 ? (T + FT - 1) / FT
                                      : ((T + 1) / 2 + FT - 1) / FT + (T / 2 + FT - 1) / FT;
    return N * mt * ((C + 63) / 64);
  }
  if (fused_spb(d)) return 0;
  const int64_t bwd3 = C < 16 ? (N * C * T + 63) / 64 : 0;
  return std::max<int64_t>(d->V == 50 ? 512 : 2048, bwd3);
}

inline BwdLayout bwd_layout(const stgcn_desc_t *d, void *ws) {
  Carve c(ws);
  BwdLayout L{};
  const int R = d->C_out, C = d->C_in, K = d->K;
  L.sg = c.take<double>(R);
  L.sgu = c.take<double>(R);
  L.sdu = c.take<double>(R);
  L.sd = c.take<double>(C);
  L.sdn = c.take<double>(C);
  L.SdZ = c.take<double>((size_t)R * d->V);
  L.s1 = c.take<double>(C);
  L.s2 = c.take<double>(C);
  // f16x2: max |dU|, |Wc|, |G| (bna: |dU A|), |x| (bna without a kept bound); zeroed with the sums
  L.amax = c.take<unsigned>(4 * kAmaxWords);
  L.dbl_bytes = c.off;
  if (!residual(d)) {  // clip-chunk sums of dU -> Tq -> sum_{n,t} dZ (kernels_fold.hip)
    L.fcs = c.take<double>((size_t)apply_cols_chunks(d->N) * R * nTo(d));
    L.ftq = c.take<double>((size_t)9 * R * d->V);
    L.f64scr = c.take<double>(fold_sdz_scratch_doubles(R, C, d->V));
  }
  if (fold_w(d)) {
    L.dWc = c.take<float>(fold_dwc_floats(R, C));
    L.fscr = c.take<float>(std::max(fold_bwd_scratch_floats(R, C),
                                    fold_fwd_scratch_floats(R, C, d->V)));
    L.SdH = c.take<double>((size_t)C * d->V);
    L.Wc = c.take<float>((size_t)R * C * 9);
    L.bZ = c.take<float>((size_t)R * d->V);
  }
  L.dU = c.take<float>((size_t)d->N * R * nTo(d));
  L.dZ = c.take<float>((size_t)d->N * R * nT(d));
  L.G = c.take<float>((size_t)d->N * K * C * nT(d));
  L.H = c.take<float>((size_t)d->N * K * C * nT(d));
  WgradParams w1 = make_wgrad_taps(d, nullptr, nullptr, nullptr);
  WgradParams w2 = wgrad_spatial(d, nullptr, nullptr, nullptr);
  size_t slab = std::max((size_t)w1.S * R * R * 9, (size_t)w2.S * R * K * C);
  if (fold_w(d)) {
    WgradParams wf = make_wgrad_taps(d, nullptr, nullptr, nullptr, C);
    slab = std::max(slab, (size_t)wf.S * R * C * 9);
  }
  if (fused_sp(d)) {  // dW' from the kept bf16 G (k_wgrad_gemm_gk)
    WgradParams wg = wgrad_gk(d, nullptr, nullptr, nullptr);
    slab = std::max(slab, (size_t)wg.S * R * K * C);
  }
  if (projection(d)) {
    WgradParams w3 = wgrad_proj(d, nullptr, nullptr, nullptr);
    slab = std::max(slab, (size_t)w3.S * R * C);
    if (d->need_dx) L.Rg = c.take<float>((size_t)d->N * C * nT(d));
  }
  L.slab = c.take<float>(slab);
  L.wpk = c.take<float>(wpk_floats(d));
  L.Wpk = c.take<float>((size_t)R * K * C);
  L.dA_cap = dA_part_cap(d);
  if (L.dA_cap) {
    const size_t kvv = (size_t)K * d->V * d->V;
    L.dApart = c.take<float>((size_t)L.dA_cap * kvv);
    L.dAlvl = c.take<double>((size_t)kDaLvl * kvv);
  }
  L.total = c.off;
  return L;
}

struct FwdLayout {
  double *s1, *q1, *s2, *q2;
  unsigned *amax;  // f16x2: max |G|, |Wc|
  float *G, *Wpk, *biasZ, *wpk;
  float *Rp;  // residual projection output (N, C_out, T_out, V)
  float *Wc, *BT;  // the folded block: composite weights, per-frame bias table
  double *bq;      // ... and its per-tap bias products
  float *fscr;     // ... and its GEMM operand re-layouts
  double *s2part;  // ... and its BN2 statistics per GEMM tile [2][C_out][N * n_mtiles]
  size_t dbl_bytes, total;
};

inline FwdLayout fwd_layout(const stgcn_desc_t *d, void *ws) {
  Carve c(ws);
  FwdLayout L{};
  const int R = d->C_out, C = d->C_in, K = d->K;
  L.s1 = c.take<double>(C);
  L.q1 = c.take<double>(C);
  L.s2 = c.take<double>(R);
  L.q2 = c.take<double>(R);
  L.amax = c.take<unsigned>(2 * kAmaxWords);  // f16x2: max |G|, |Wc|
  L.dbl_bytes = c.off;
  L.G = c.take<float>((size_t)d->N * K * C * nT(d));
  L.Wpk = c.take<float>((size_t)R * K * C);
  L.biasZ = c.take<float>((size_t)R * d->V);
  L.wpk = c.take<float>(wpk_floats(d));
  if (projection(d)) L.Rp = c.take<float>((size_t)d->N * R * nTo(d));
  if (fold_w(d)) {
    L.Wc = c.take<float>((size_t)R * C * 9);
    L.BT = c.take<float>((size_t)R * nTo(d));
    L.bq = c.take<double>((size_t)9 * R * d->V);
    L.fscr = c.take<float>(fold_fwd_scratch_floats(R, C, d->V));
    if (d->training) L.s2part = c.take<double>((size_t)fold_stat_tiles(d) * 2 * R);
  }
  L.total = c.off;
  return L;
}

// A folded block's stgcn_fold_prep buffer (ABI 7); wpk_f / wpk_d: the split-plane
// packs of Wc for the forward and for each launch of the data gradient
// (conv_x3_pack_job reads the weight fields of tconv_fwd / tconv_dgrad)
struct PrepLayout {
  float *bZ, *Wc, *BT, *fscr_f, *fscr_b;
  double *bq, *f64;
  unsigned *amax;  // max |Wc| (kAmaxWords, every slot written)
  char *wpk_f, *wpk_d[2];
  size_t total;
};

inline PrepLayout prep_layout(const stgcn_desc_t *d, const void *base) {
  Carve c(const_cast<void *>(base));
  PrepLayout P{};
  const int R = d->C_out, C = d->C_in, V = d->V;
  P.amax = c.take<unsigned>(kAmaxWords);
  P.bq = c.take<double>((size_t)9 * R * V);
  P.f64 = c.take<double>(fold_sdz_scratch_doubles(R, C, V));
  P.bZ = c.take<float>((size_t)R * V);
  P.Wc = c.take<float>((size_t)R * C * 9);
  P.BT = c.take<float>((size_t)R * nTo(d));
  P.fscr_f = c.take<float>(fold_fwd_scratch_floats(R, C, V));
  P.fscr_b = c.take<float>(fold_bwd_scratch_floats(R, C));
  P.wpk_f = c.take<char>(conv_x3_pack_bytes(
      tconv_fwd(d, C, nullptr, nullptr, nullptr, nullptr), fold_fwd_npl(d)));
  for (int ph = 0; ph < tconv_dgrad_phases(d); ++ph)
    P.wpk_d[ph] = c.take<char>(conv_x3_pack_bytes(
        tconv_dgrad(d, C, ph, nullptr, nullptr, nullptr, nullptr), fold_dgrad_npl(d)));
  P.total = c.off;
  return P;
}

// SpatialConv on its own (stgcn_spatial_fwd / _bwd), planned as a block descriptor
struct SpatialLayout {
  float *ident;  // [4][C_in]: mean 0 | invstd 1 | gamma 1 | beta 0
  double *sd, *sdn, *SdZ;
  float *G, *H, *Wpk, *biasZ, *wpk, *slab;
  size_t total;
};

inline SpatialLayout spatial_layout(const stgcn_desc_t *d, void *ws, bool backward) {
  Carve c(ws);
  SpatialLayout L{};
  const int R = d->C_out, C = d->C_in, K = d->K;
  L.ident = c.take<float>((size_t)4 * C);
  L.G = c.take<float>((size_t)d->N * K * C * nT(d));
  L.Wpk = c.take<float>((size_t)R * K * C);
  L.wpk = c.take<float>(wpk_floats(d));
  if (!backward) {
    L.biasZ = c.take<float>((size_t)R * d->V);
  } else {
    L.sd = c.take<double>(C);
    L.sdn = c.take<double>(C);
    L.SdZ = c.take<double>((size_t)R * d->V);
    L.H = c.take<float>((size_t)d->N * K * C * nT(d));
    WgradParams w = wgrad_spatial(d, nullptr, nullptr, nullptr);
    L.slab = c.take<float>((size_t)w.S * R * K * C);
  }
  L.total = c.off;
  return L;
}

}  // namespace stgcn
