// BatchNorm / ReLU element math of every kernel that forms, or forms again, a
// BatchNorm output. gfx950 only, device only.
//
// A kernel that rebuilds x = ReLU(BN2(U)) from a saved pre-BN2 tensor U
// (STGCN_PLAN_X_FROM_U, the PrevBn chain, the ReLU + BN2 backward, the head
// pooled from U) must get the bits, and the ReLU mask, that bn_relu_fwd_body
// (kernels_bn.hip) got when it first formed x. So the expressions stand here
// once, as plain operators under the build's default contraction. Reshaped (an
// explicit fmaf, a hoisted is * g) they flip the mask of elements near zero.
#pragma once
#include <hip/hip_runtime.h>

#include "internal.h"  // BnRef

namespace stgcn {

// BN(x) with a = invstd * g, and xhat, on per-channel values the kernel holds
__device__ __forceinline__ float bn_pre(float x, float mu, float a, float be) {
  return (x - mu) * a + be;
}
__device__ __forceinline__ float bn_hat(float x, float mu, float is) { return (x - mu) * is; }

// One channel's BatchNorm, loaded in the order mean, invstd, g, b
struct BnAff {
  float mu, is, a, be;
  __device__ __forceinline__ float pre(float x) const { return bn_pre(x, mu, a, be); }
  __device__ __forceinline__ float hat(float x) const { return bn_hat(x, mu, is); }
};
__device__ __forceinline__ BnAff bn_aff(const float *mean, const float *invstd, const float *g,
                                        const float *b, int c) {
  BnAff r = {mean[c], invstd[c]};
  r.a = r.is * g[c], r.be = b[c];
  return r;
}
__device__ __forceinline__ BnAff bn_aff(const BnRef &bn, int c) {
  return bn_aff(bn.mean, bn.invstd, bn.g, bn.b, c);
}

// ReLU keeps NaN, as torch.relu does (stgcn_hip.h Conventions, "Non-finite
// values"): its predicate is !(t <= 0), true for NaN, and y and the backward's
// mask come from that one predicate so that they cannot disagree. On every
// other value it is t > 0, and the bits of y are those of t > 0 ? t : 0.
__device__ __forceinline__ bool relu_on(float t) { return !(t <= 0.f); }

// The element of y = ReLU(BN2(u)): y, the mask m = relu_on(pre) and uhat, as
// bn_relu_fwd_body (kernels_bn.hip) forms the block's output. A kernel that
// rebuilds that output from U writes these lines on bn_pre / bn_hat, or
// bn_relu(pre(u)) where only y is needed.
struct BnReluX {
  float x, uh;
  bool m;
};
__device__ __forceinline__ BnReluX bn_relu_x(const BnAff &p, float u) {
  BnReluX r;
  const float t = p.pre(u);
  r.uh = p.hat(u);
  r.m = relu_on(t);
  r.x = r.m ? t : 0.f;
  return r;
}
__device__ __forceinline__ float bn_relu(float t) { return relu_on(t) ? t : 0.f; }
// The same values from one instruction (v_maximum3_f32: the IEEE 754-2019
// maximum, which keeps NaN and gives +0 for -0), for the sites that need no
// mask: BN1's ReLU of the residual block and the convolutions' ReLU epilogue.
__device__ __forceinline__ float relu_max(float t) { return __builtin_elementwise_maximum(t, 0.f); }

// ReLU + BN2 backward element: g = d on the mask, mg = sum(g) / M, mgu = sum(g uhat) / M
__device__ __forceinline__ float bn2_bwd(const BnAff &p, float u, float d, float mg, float mgu) {
  const float uh = p.hat(u);
  const float gg = relu_on(p.pre(u)) ? d : 0.f;
  return p.a * (gg - mg - uh * mgu);
}

// Deferred dx of the next block (k_chain_coef's five values per channel), y this
// block's output. The null test of the coefficient pointer stays with the kernel.
struct DyCoef {
  float cmdn, cis, cmu, cmd, ca;  // (this order keeps the kernels' register assignment)
  __device__ __forceinline__ void load(const float *coef, int C, int c) {
    ca = coef[c];
    cmd = coef[C + c];
    cmu = coef[2 * C + c];
    cis = coef[3 * C + c];
    cmdn = coef[4 * C + c];
  }
  __device__ __forceinline__ float dy(float d, float y) const {
    return ca * (d - cmd - (y - cmu) * cis * cmdn);
  }
};

}  // namespace stgcn
