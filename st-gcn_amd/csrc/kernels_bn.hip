// BatchNorm / ReLU elementwise kernels of libstgcn_hip.so — gfx950 (MI355X /
// CDNA4) only.
//
// Statistics, normalise + ReLU forward, and the backward reduce / apply passes
// of the block's two BatchNorms, one 256-thread block per (n, c) slice (or a
// few rows of slices), vectorised 1 / 2 / 4 floats wide by the slice's length
// and the pointers' alignment (VecF, slice_vec, STGCN_VEC_LAUNCH). Statistics
// accumulate in fp64. The launchers are declared in internal.h.
//
// Wave size is 64; every block is a multiple of 64 threads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <initializer_list>

#include "device_common.h"
#include "internal.h"

namespace stgcn {

// ---------------------------------------------------------------------------
// BatchNorm kernels. One 256-thread block per (n, c) slice of L = T*V floats.
// ---------------------------------------------------------------------------
// Vector width VEC (1, 2, 4 floats) for the per-(n, c) slice loops: the slice
// base (n*C + c)*L is a multiple of VEC when L is.
template <int N>
struct VecF;
template <>
struct VecF<1> {
  using T = float;
};
template <>
struct VecF<2> {
  using T = float2;
};
template <>
struct VecF<4> {
  using T = float4;
};
template <int N>
__device__ __forceinline__ void vld(const float *p, float (&v)[N]) {
  const typename VecF<N>::T t = *reinterpret_cast<const typename VecF<N>::T *>(p);
  __builtin_memcpy(v, &t, sizeof(t));
}
template <int N>
__device__ __forceinline__ void vst(float *p, const float (&v)[N]) {
  typename VecF<N>::T t;
  __builtin_memcpy(&t, v, sizeof(t));
  *reinterpret_cast<typename VecF<N>::T *>(p) = t;
}

static int slice_vec(int L, std::initializer_list<const void *> ptrs) {
  int vec = L % 4 == 0 ? 4 : (L % 2 == 0 ? 2 : 1);
  for (const void *q : ptrs)  // (null pointers are aligned)
    while (vec > 1 && ((uintptr_t)q & (4 * vec - 1)) != 0) vec >>= 1;
  return vec;
}

#define STGCN_VEC_LAUNCH(kern, vec, grid, ...)                            \
  do {                                                                    \
    if ((vec) == 4)                                                       \
      hipLaunchKernelGGL((kern<4>), grid, dim3(256), 0, s, __VA_ARGS__); \
    else if ((vec) == 2)                                                  \
      hipLaunchKernelGGL((kern<2>), grid, dim3(256), 0, s, __VA_ARGS__); \
    else                                                                  \
      hipLaunchKernelGGL((kern<1>), grid, dim3(256), 0, s, __VA_ARGS__); \
  } while (0)

// sum * invM of a BatchNorm backward's batch-mean terms. Eval mode passes
// invM = 0 (constant running statistics: the terms are absent), and absent
// means 0 whatever the sum holds: NaN * 0 is NaN, and one bad element of dy
// would reach every clip through its channel's sum.
__device__ __forceinline__ float bn_mean_term(double sum, double invM) {
  return invM != 0.0 ? (float)(sum * invM) : 0.f;
}

// (amax, or null: max |x| as float bits, device_common.h block_amax -- the
// fp16 operand bound of the folded block's GEMMs that read x, capi.hip fold_bna)
template <int VEC>
__global__ __launch_bounds__(256) void k_bn_stats(const float *x, int C, int L, double *sum,
                                                  double *sq, unsigned *amax) {
  __shared__ double red[8];
  const int c = blockIdx.x, n = blockIdx.y;
  const float *src = x + ((int64_t)n * C + c) * L;
  double s = 0.0, q = 0.0;
  float m = 0.f;
  for (int i = threadIdx.x * VEC; i < L; i += 256 * VEC) {
    float v[VEC];
    vld<VEC>(src + i, v);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      s += (double)v[j];
      q += (double)v[j] * (double)v[j];
      m = fmaxf(m, amax_abs(v[j]));
    }
  }
  if (amax) block_amax<256>(m, amax);
  block_sum2_atomic<256>(s, q, sum + c, sq + c, red);
}

hipError_t launch_bn_stats(const float *x, int N, int C, int L, double *sum, double *sq,
                           hipStream_t s, unsigned *amax) {
  STGCN_VEC_LAUNCH(k_bn_stats, slice_vec(L, {x}), dim3(C, N), x, C, L, sum, sq, amax);
  return hipGetLastError();
}

// (zw non-null: also zeroes nzw words for the kernels that follow -- the f16x2
// max |x| words of the folded forward -- instead of a memset launch)
__global__ void k_bn_finalize(const double *sum, const double *sq, int C, int64_t M, float eps,
                              float momentum, int training, float *rm, float *rv, float *mean_out,
                              float *invstd_out, unsigned *zw, int nzw) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (zw)
    for (int i = c; i < nzw; i += gridDim.x * blockDim.x) zw[i] = 0u;
  if (c >= C) return;
  if (training) {
    const double mean = sum[c] / (double)M;
    double var = sq[c] / (double)M - mean * mean;
    if (var < 0.0) var = 0.0;
    mean_out[c] = (float)mean;
    invstd_out[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (rm) {
      const double unb = M > 1 ? var * (double)M / (double)(M - 1) : var;
      rm[c] = (float)((1.0 - momentum) * rm[c] + momentum * mean);
      rv[c] = (float)((1.0 - momentum) * rv[c] + momentum * unb);
    }
  } else {
    mean_out[c] = rm[c];
    invstd_out[c] = (float)(1.0 / sqrt((double)rv[c] + (double)eps));
  }
}

// one workgroup per channel: the tile partials summed in a fixed order (strided
// per thread, then a fixed tree), then k_bn_finalize's arithmetic
// (ys non-null: also zeroes the block's y_stats -- 5 C doubles, then nw words --
// for the output pass that follows: no memset launch)
__global__ __launch_bounds__(256) void k_bn_finalize_parts(const double *part, int ntiles, int C,
                                                           int64_t M, float eps, float momentum,
                                                           int training, float *rm, float *rv,
                                                           float *mean_out, float *invstd_out,
                                                           double *ys, int nw) {
  __shared__ double red[2][256];
  const int c = blockIdx.x, tid = threadIdx.x;
  if (ys) {
    if (tid < 5) ys[(int64_t)tid * C + c] = 0.0;
    const int per = (nw + C - 1) / C;
    unsigned *w = reinterpret_cast<unsigned *>(ys + 5 * (int64_t)C);
    for (int i = tid; i < per; i += 256)
      if (c * per + i < nw) w[c * per + i] = 0u;
  }
  double a = 0.0, b = 0.0;
  const double *pa = part + (int64_t)c * ntiles, *pb = pa + (int64_t)C * ntiles;
  for (int t = tid; t < ntiles; t += 256) {  // (contiguous per channel: coalesced)
    a += pa[t];
    b += pb[t];
  }
  red[0][tid] = a;
  red[1][tid] = b;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      red[0][tid] += red[0][tid + h];
      red[1][tid] += red[1][tid + h];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const double mean = red[0][0] / (double)M;
  double var = red[1][0] / (double)M - mean * mean;
  if (var < 0.0) var = 0.0;
  mean_out[c] = (float)mean;
  invstd_out[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (training && rm) {
    const double unb = M > 1 ? var * (double)M / (double)(M - 1) : var;
    rm[c] = (float)((1.0 - momentum) * rm[c] + momentum * mean);
    rv[c] = (float)((1.0 - momentum) * rv[c] + momentum * unb);
  }
}

hipError_t launch_bn_finalize_parts(const double *part, int ntiles, int C, int64_t M, float eps,
                                    float momentum, int training, float *rm, float *rv,
                                    float *mean_out, float *invstd_out, hipStream_t s,
                                    double *ys_zero, int nw) {
  if (!training) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_bn_finalize_parts, dim3(C), dim3(256), 0, s, part, ntiles, C, M, eps,
                     momentum, training, rm, rv, mean_out, invstd_out, ys_zero, nw);
  return hipGetLastError();
}

hipError_t launch_bn_finalize(const double *sum, const double *sq, int C, int64_t M, float eps,
                              float momentum, int training, float *rm, float *rv,
                              float *mean_out, float *invstd_out, hipStream_t s, unsigned *zw,
                              int nzw) {
  hipLaunchKernelGGL(k_bn_finalize, dim3((C + 255) / 256), dim3(256), 0, s, sum, sq, C, M, eps,
                     momentum, training, rm, rv, mean_out, invstd_out, zw, nzw);
  return hipGetLastError();
}

// y = ReLU(BN(U)); optionally (ysum != null) also the per-channel sum and sum
// of squares of y (fp64): the next block's BN1 batch statistics. A block
// covers kBnRows clips of one channel (one block reduction and one set of
// fp64 atomics per kBnRows rows: per-row blocks spent their time there).
// (y null, ABI 8: only the statistics -- the next block forms y itself from U,
// STGCN_PLAN_X_FROM_U -- as k_bn_relu_stats, so traces tell the two apart)
constexpr int kBnRows = 4;
template <int VEC, bool WY>
__device__ __forceinline__ void bn_relu_fwd_body(const float *U, const float *mean,
                                                 const float *invstd, const float *g,
                                                 const float *b, float *y, int N, int C, int L,
                                                 double *ysum, double *ysq, Dropout drop,
                                                 double *yext, unsigned *ymax) {
  __shared__ double red[8];
  drop = dropout_resolve(drop);
  const int c = blockIdx.x, n0 = blockIdx.y * kBnRows, n1 = min(N, n0 + kBnRows);
  const BnAff bn = bn_aff(mean, invstd, g, b, c);
  double s = 0.0, q = 0.0, cnt = 0.0, su = 0.0, xu = 0.0;
  float ym = 0.f;  // max y (y >= 0): the next block's fp16 operand bound
  // (two vectors' loads issued before either's math; the sums stay fp64 per
  // element: the chain sums su / xu feed nearly cancelling BN2 backward terms)
  auto vec = [&](int64_t base, int i, float (&v)[VEC]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const BnReluX e = bn_relu_x(bn, v[j]);
      v[j] = e.x;
      if (drop.thresh) v[j] = dropout_keep(drop, base + i + j) ? v[j] * drop.scale : 0.f;
      s += (double)v[j];
      q += (double)v[j] * (double)v[j];
      ym = fmaxf(ym, amax_abs(v[j]));  // (v >= 0 or NaN)
      if (yext && e.m) {
        cnt += 1.0;
        su += (double)e.uh;
        xu += (double)v[j] * (double)e.uh;
      }
    }
    if constexpr (WY) vst<VEC>(y + base + i, v);
  };
  for (int n = n0; n < n1; ++n) {
    const int64_t base = ((int64_t)n * C + c) * L;
    int i = threadIdx.x * VEC;
    for (; i + 256 * VEC < L; i += 512 * VEC) {
      float v0[VEC], v1[VEC];
      vld<VEC>(U + base + i, v0);
      vld<VEC>(U + base + i + 256 * VEC, v1);
      vec(base, i, v0);
      vec(base, i + 256 * VEC, v1);
    }
    if (i < L) {
      float v0[VEC];
      vld<VEC>(U + base + i, v0);
      vec(base, i, v0);
    }
  }
  if (ysum) block_sum2_atomic<256>(s, q, ysum + c, ysq + c, red);
  if (yext) {
    block_sum2_atomic<256>(cnt, su, yext + c, yext + C + c, red);
    block_sum2_atomic<256>(xu, 0.0, yext + 2 * C + c, nullptr, red);
  }
  if (ymax) block_amax<256>(ym, ymax);
}

template <int VEC>
__global__ __launch_bounds__(256) void k_bn_relu_fwd(const float *U, const float *mean,
                                                     const float *invstd, const float *g,
                                                     const float *b, float *y, int N, int C,
                                                     int L, double *ysum, double *ysq,
                                                     Dropout drop, double *yext,
                                                     unsigned *ymax) {
  bn_relu_fwd_body<VEC, true>(U, mean, invstd, g, b, y, N, C, L, ysum, ysq, drop, yext, ymax);
}

template <int VEC>
__global__ __launch_bounds__(256) void k_bn_relu_stats(const float *U, const float *mean,
                                                       const float *invstd, const float *g,
                                                       const float *b, float *y, int N, int C,
                                                       int L, double *ysum, double *ysq,
                                                       Dropout drop, double *yext,
                                                       unsigned *ymax) {
  bn_relu_fwd_body<VEC, false>(U, mean, invstd, g, b, y, N, C, L, ysum, ysq, drop, yext, ymax);
}

hipError_t launch_bn_relu_fwd(const float *U, const BnRef &bn, float *y, int N, int C, int L,
                              double *ysum, double *ysq, Dropout drop, hipStream_t s,
                              double *yext, unsigned *ymax) {
  if (!y) {
    if (!ysum) return hipErrorInvalidValue;  // (nothing to form)
    STGCN_VEC_LAUNCH(k_bn_relu_stats, slice_vec(L, {U}), dim3(C, (N + kBnRows - 1) / kBnRows), U,
                     bn.mean, bn.invstd, bn.g, bn.b, y, N, C, L, ysum, ysq, drop, yext, ymax);
    return hipGetLastError();
  }
  STGCN_VEC_LAUNCH(k_bn_relu_fwd, slice_vec(L, {U, y}), dim3(C, (N + kBnRows - 1) / kBnRows), U,
                   bn.mean, bn.invstd, bn.g, bn.b, y, N, C, L, ysum, ysq, drop, yext, ymax);
  return hipGetLastError();
}

template <int VEC>
__global__ __launch_bounds__(256) void k_bn_relu_bwd_reduce(const float *dy, const float *U,
                                                            const float *mean,
                                                            const float *invstd, const float *g,
                                                            const float *b, int C, int L,
                                                            double *sg, double *sgu,
                                                            Dropout drop, const float *dync) {
  __shared__ double red[8];
  const int c = blockIdx.x, n = blockIdx.y;
  const int64_t base = ((int64_t)n * C + c) * L;
  const BnAff bn = bn_aff(mean, invstd, g, b, c);
  const float dv = dync ? dync[(int64_t)n * C + c] : 0.f;  // (ABI 10: dy constant per row)
  drop = dropout_resolve(drop);
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x * VEC; i < L; i += 256 * VEC) {
    float u[VEC], d[VEC];
    vld<VEC>(U + base + i, u);
    if (dync) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) d[j] = dv;
    } else {
      vld<VEC>(dy + base + i, d);
    }
    if (drop.thresh) {  // gradient through the fused dropout
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        d[j] = dropout_keep(drop, base + i + j) ? d[j] * drop.scale : 0.f;
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      if (relu_on(bn.pre(u[j]))) {
        s += d[j];
        q += (double)d[j] * (double)bn.hat(u[j]);
      }
  }
  block_sum2_atomic<256>(s, q, sg + c, sgu + c, red);
}

hipError_t launch_bn_relu_bwd_reduce(const Bn2Bwd &q, double *sg, double *sgu, hipStream_t s) {
  STGCN_VEC_LAUNCH(k_bn_relu_bwd_reduce, slice_vec(q.L, {q.dy, q.U}), dim3(q.C, q.N), q.dy, q.U,
                   q.bn.mean, q.bn.invstd, q.bn.g, q.bn.b, q.C, q.L, sg, sgu, q.drop, q.dy_nc);
  return hipGetLastError();
}

// dU stored as bf16 in the fp32 buffer (its readers round it to bf16 anyway). A
// macro: behind a call the address arithmetic of one of its two kernels moves.
#define STGCN_STORE_DU_BF16(dU, base, i, o)                                                  \
  do {                                                                                       \
    __bf16 *ob_ = reinterpret_cast<__bf16 *>(dU) + (base) + (i);                             \
    unsigned short h_[VEC];                                                                  \
    _Pragma("unroll") for (int j_ = 0; j_ < VEC; ++j_)                                       \
        h_[j_] = __builtin_bit_cast(unsigned short, (__bf16)(o)[j_]);                        \
    if constexpr (VEC == 4)                                                                  \
      *reinterpret_cast<uint2 *>(ob_) =                                                      \
          make_uint2(h_[0] | ((unsigned)h_[1] << 16), h_[2] | ((unsigned)h_[3] << 16));      \
    else if constexpr (VEC == 2)                                                             \
      *reinterpret_cast<unsigned *>(ob_) = h_[0] | ((unsigned)h_[1] << 16);                  \
    else                                                                                     \
      *reinterpret_cast<unsigned short *>(ob_) = h_[0];                                      \
  } while (0)

template <int VEC>
__global__ __launch_bounds__(256) void k_bn_relu_bwd_apply(
    const float *dy, const float *U, const float *mean, const float *invstd, const float *g,
    const float *b, const double *sg, const double *sgu, float *dU, double *sdu, int C, int L,
    double invM, Dropout drop, int du_bf16, const float *dy_coef, const float *dync) {
  __shared__ double red[8];
  const int c = blockIdx.x, n = blockIdx.y;
  const int64_t base = ((int64_t)n * C + c) * L;
  const float dv = dync ? dync[(int64_t)n * C + c] : 0.f;  // (ABI 10: dy constant per row)
  drop = dropout_resolve(drop);
  const BnAff bn = bn_aff(mean, invstd, g, b, c);
  const float mg = bn_mean_term(sg[c], invM), mgu = bn_mean_term(sgu[c], invM);
  DyCoef dc = {};
  if (dy_coef) dc.load(dy_coef, C, c);
  double s = 0.0;
  for (int i = threadIdx.x * VEC; i < L; i += 256 * VEC) {
    float u[VEC], d[VEC], o[VEC];
    vld<VEC>(U + base + i, u);
    if (dync) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) d[j] = dv;
    } else {
      vld<VEC>(dy + base + i, d);
    }
    if (dy_coef) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) d[j] = dc.dy(d[j], bn_relu(bn.pre(u[j])));
    }
    if (drop.thresh) {
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        d[j] = dropout_keep(drop, base + i + j) ? d[j] * drop.scale : 0.f;
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      o[j] = bn2_bwd(bn, u[j], d[j], mg, mgu);
      s += o[j];
    }
    if (du_bf16) {
      STGCN_STORE_DU_BF16(dU, base, i, o);
    } else {
      vst<VEC>(dU + base + i, o);
    }
  }
  block_sum2_atomic<256>(s, 0.0, sdu + c, nullptr, red);
}

// 1 / M of the apply passes (eval mode, constant running statistics: no batch-mean terms)
static double bn2_inv_m(const Bn2Bwd &q) { return q.training ? 1.0 / ((double)q.N * q.L) : 0.0; }

hipError_t launch_bn_relu_bwd_apply(const Bn2Bwd &q, hipStream_t s) {
  STGCN_VEC_LAUNCH(k_bn_relu_bwd_apply, slice_vec(q.L, {q.dy, q.U, q.dU}), dim3(q.C, q.N), q.dy,
                   q.U, q.bn.mean, q.bn.invstd, q.bn.g, q.bn.b, q.sg, q.sgu, q.dU, q.sdu, q.C, q.L,
                   bn2_inv_m(q), q.drop, q.du_bf16, q.dy_coef, q.dy_nc);
  return hipGetLastError();
}

// k_bn_relu_bwd_apply with the clip sums of its output (non-residual blocks):
// block = (channel c, 256 * VEC consecutive positions of the (T_out, V) row,
// clip chunk z), thread = VEC positions over the chunk's clips, so
// cs[z][c][pos] = sum_{n in chunk z} dU[n, c, pos] accumulates in registers
// (fp64, no atomics). Those sums give sum_{n,t} dZ by the per-tap algebra of
// kernels_fold.hip (SdZ = sum_q Wt_q^T Tq): the separate pass over dZ is gone.
template <int VEC>
__global__ __launch_bounds__(256) void k_bn_relu_bwd_apply_cols(
    const float *__restrict__ dy, const float *__restrict__ U, const float *mean,
    const float *invstd, const float *g, const float *b, const double *sg, const double *sgu,
    float *__restrict__ dU, double *sdu, int N, int C, int L, double invM, Dropout drop,
    int du_bf16, const float *dy_coef, double *__restrict__ cs, unsigned *amax,
    const float *dync) {
  __shared__ double red[8];
  drop = dropout_resolve(drop);
  float om = 0.f;  // max |dU| (f16x2 operand bound)
  const int c = blockIdx.x;
  const int i = (blockIdx.y * 256 + threadIdx.x) * VEC;
  const int nz = gridDim.z, per = (N + nz - 1) / nz;
  const int n0 = blockIdx.z * per, n1 = min(N, n0 + per);
  const BnAff bn = bn_aff(mean, invstd, g, b, c);
  const float mg = bn_mean_term(sg[c], invM), mgu = bn_mean_term(sgu[c], invM);
  // (this kernel keeps the five loads as scalars: as a DyCoef captured by the
  // lambdas below they come out in other registers)
  float ca = 0.f, cmd = 0.f, cmu = 0.f, cis = 0.f, cmdn = 0.f;
  if (dy_coef) {
    ca = dy_coef[c];
    cmd = dy_coef[C + c];
    cmu = dy_coef[2 * C + c];
    cis = dy_coef[3 * C + c];
    cmdn = dy_coef[4 * C + c];
  }
  double s = 0.0, col[VEC] = {};
  if (i < L) {
    // (two clips' operands in flight ahead of this clip's math and stores:
    // register sets A (even steps) and B (odd steps), loaded two clips ahead)
    float ua[VEC], da[VEC], ub[VEC], db[VEC];
    const int64_t cl = (int64_t)C * L;  // floats per clip
    const int64_t b0 = ((int64_t)n0 * C + c) * L + i;
    // (ABI 10, dync: dy constant over the row -- one value per clip, no dy tensor)
    auto ldy = [&](int64_t off, int nn, float (&dr)[VEC]) __attribute__((always_inline)) {
      if (dync) {
        const float dv = dync[(int64_t)nn * C + c];
#pragma unroll
        for (int j = 0; j < VEC; ++j) dr[j] = dv;
      } else {
        vld<VEC>(dy + off, dr);
      }
    };
    if (n0 < n1) {
      vld<VEC>(U + b0, ua);
      ldy(b0, n0, da);
    }
    if (n0 + 1 < n1) {
      vld<VEC>(U + b0 + cl, ub);
      ldy(b0 + cl, n0 + 1, db);
    }
    auto clip = [&](int n, float (&ur)[VEC], float (&dr)[VEC]) __attribute__((always_inline)) {
      const int64_t base = ((int64_t)n * C + c) * L;
      float u[VEC], d[VEC], o[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        u[j] = ur[j];
        d[j] = dr[j];
      }
      if (n + 2 < n1) {
        vld<VEC>(U + base + 2 * cl + i, ur);
        ldy(base + 2 * cl + i, n + 2, dr);
      }
      if (dy_coef) {
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          d[j] = ca * (d[j] - cmd - (bn_relu(bn.pre(u[j])) - cmu) * cis * cmdn);
      }
      if (drop.thresh) {
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          d[j] = dropout_keep(drop, base + i + j) ? d[j] * drop.scale : 0.f;
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        o[j] = bn2_bwd(bn, u[j], d[j], mg, mgu);
        s += o[j];
        col[j] += o[j];
        om = fmaxf(om, amax_abs(o[j]));
      }
      if (du_bf16) {
        STGCN_STORE_DU_BF16(dU, base, i, o);
      } else {
        vst<VEC>(dU + base + i, o);
      }
    };
    for (int n = n0; n < n1; n += 2) {
      clip(n, ua, da);
      if (n + 1 < n1) clip(n + 1, ub, db);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) cs[((int64_t)blockIdx.z * C + c) * L + i + j] = col[j];
  }
  if (amax) block_amax<256>(om, amax);
  block_sum2_atomic<256>(s, 0.0, sdu + c, nullptr, red);
}

int apply_cols_chunks(int N) { return std::min(N, 4); }

// k_bn_relu_bwd_apply_cols for the folded block without G (capi.hip fold_bna).
// Block = (channel c, a tile of FR = 28 frames, clip chunk z), 256 threads; per
// clip of the chunk:
//   1. thread i < 252 takes joints 2i, 2i + 1 of the tile's 504 positions (fp32
//      pairs, coalesced): dU as k_bn_relu_bwd_apply_cols forms it, stored, its
//      clip-chunk sums in registers, and dU into an LDS row (double-buffered);
//   2. thread i forms dUA at positions e = i, i + 256 (< 504), frame e / V,
//      joint w = e % V:  dUA[n,c,t,w] = sum_v dU[n,c,t,v] A[v][w]  (fp32 fma in v
//      order, its two columns of A in registers), stored as coalesced words:
// the weight gradient's P operand. Also the fp16 operand bounds max |dU|
// (amax) and max |dUA| (amaxa). One barrier per clip.
constexpr int kFrTile = 28;
template <int V>
__global__ __launch_bounds__(256) void k_bn_relu_bwd_apply_fr(
    const float *__restrict__ dy, const float *__restrict__ U, const float *mean,
    const float *invstd, const float *g, const float *b, const double *sg, const double *sgu,
    float *__restrict__ dU, float *__restrict__ dUA, double *sdu, int N, int C, int To,
    double invM, Dropout drop, const float *dy_coef, double *__restrict__ cs, unsigned *amax,
    unsigned *amaxa, const float *A) {
  static_assert(V % 2 == 0, "whole pairs per frame");
  constexpr int NP = kFrTile * V;  // positions of a tile
  static_assert(NP / 2 <= 256 && NP <= 512, "one pair per thread, two outputs per thread");
  __shared__ float ob[2][NP];
  __shared__ double red[8];
  drop = dropout_resolve(drop);
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int f0 = blockIdx.y * kFrTile, nf = min(kFrTile, To - f0);
  const int L = To * V, np = nf * V;
  const int nz = gridDim.z, per = (N + nz - 1) / nz;
  const int n0 = blockIdx.z * per, n1 = min(N, n0 + per);
  const BnAff bn = bn_aff(mean, invstd, g, b, c);
  const float mg = bn_mean_term(sg[c], invM), mgu = bn_mean_term(sgu[c], invM);
  DyCoef dc = {};
  if (dy_coef) dc.load(dy_coef, C, c);
  // this thread's two output positions of dUA and their columns of A
  const int e0 = tid, e1 = tid + 256;
  const int w0 = e0 % V, w1 = e1 % V, fr0 = e0 / V, fr1 = e1 / V;
  float a0[V], a1[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    a0[v] = A[v * V + w0];
    a1[v] = A[v * V + w1];
  }
  const int pp = 2 * tid;  // this thread's pair of phase 1
  const bool pok = pp < np;
  float om = 0.f, oma = 0.f;
  double s = 0.0, col0 = 0.0, col1 = 0.0;
  for (int n = n0; n < n1; ++n) {
    const int64_t base = ((int64_t)n * C + c) * L + (int64_t)f0 * V;
    float *obn = ob[(n - n0) & 1];
    if (pok) {
      const float2 uu = *reinterpret_cast<const float2 *>(U + base + pp);
      const float2 dd = *reinterpret_cast<const float2 *>(dy + base + pp);
      float u[2] = {uu.x, uu.y}, d[2] = {dd.x, dd.y}, o[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (dy_coef) {
          d[j] = dc.dy(d[j], bn_relu(bn.pre(u[j])));
        }
        if (drop.thresh) d[j] = dropout_keep(drop, base + pp + j) ? d[j] * drop.scale : 0.f;
        o[j] = bn2_bwd(bn, u[j], d[j], mg, mgu);
        s += o[j];
        om = fmaxf(om, amax_abs(o[j]));
      }
      col0 += o[0];
      col1 += o[1];
      *reinterpret_cast<float2 *>(dU + base + pp) = make_float2(o[0], o[1]);
      *reinterpret_cast<float2 *>(obn + pp) = make_float2(o[0], o[1]);
    }
    __syncthreads();  // (double buffer: the other row is free since the last barrier)
    if (e0 < np) {
      const float *r = obn + fr0 * V;
      float t = r[0] * a0[0];
#pragma unroll
      for (int v = 1; v < V; ++v) t = fmaf(r[v], a0[v], t);
      dUA[base + e0] = t;
      oma = fmaxf(oma, amax_abs(t));
    }
    if (e1 < np) {
      const float *r = obn + fr1 * V;
      float t = r[0] * a1[0];
#pragma unroll
      for (int v = 1; v < V; ++v) t = fmaf(r[v], a1[v], t);
      dUA[base + e1] = t;
      oma = fmaxf(oma, amax_abs(t));
    }
  }
  if (pok) {
    double *dst = cs + ((int64_t)blockIdx.z * C + c) * L + (int64_t)f0 * V + pp;
    dst[0] = col0;
    dst[1] = col1;
  }
  block_amax<256>(om, amax);
  __syncthreads();  // (block_amax's LDS words are reused by the second call)
  block_amax<256>(oma, amaxa);
  block_sum2_atomic<256>(s, 0.0, sdu + c, nullptr, red);
}

hipError_t launch_bn_relu_bwd_apply_fr(const Bn2Bwd &q, hipStream_t s) {
  if (q.V != 18 || !q.amax || !q.amaxa || !q.A) return hipErrorInvalidValue;
  const int To = q.L / q.V;
  hipLaunchKernelGGL((k_bn_relu_bwd_apply_fr<18>),
                     dim3(q.C, (To + kFrTile - 1) / kFrTile, apply_cols_chunks(q.N)), dim3(256), 0,
                     s, q.dy, q.U, q.bn.mean, q.bn.invstd, q.bn.g, q.bn.b, q.sg, q.sgu, q.dU, q.dUA,
                     q.sdu, q.N, q.C, To, bn2_inv_m(q), q.drop, q.dy_coef, q.cs, q.amax, q.amaxa,
                     q.A);
  return hipGetLastError();
}

hipError_t launch_bn_relu_bwd_apply_cols(const Bn2Bwd &q, hipStream_t s) {
  // (whole-row vectors: every row start VEC-aligned needs L % VEC == 0)
  int vec = slice_vec(q.L, {q.dy, q.U, q.dU});
  const int nz = apply_cols_chunks(q.N);
#define COLS_LAUNCH(VV)                                                                        \
  hipLaunchKernelGGL((k_bn_relu_bwd_apply_cols<VV>),                                           \
                     dim3(q.C, (q.L + 256 * VV - 1) / (256 * VV), nz), dim3(256), 0, s, q.dy,  \
                     q.U, q.bn.mean, q.bn.invstd, q.bn.g, q.bn.b, q.sg, q.sgu, q.dU, q.sdu, q.N, \
                     q.C, q.L, bn2_inv_m(q), q.drop, q.du_bf16, q.dy_coef, q.cs, q.amax, q.dy_nc)
  if (vec == 4)
    COLS_LAUNCH(4);
  else if (vec == 2)
    COLS_LAUNCH(2);
  else
    COLS_LAUNCH(1);
#undef COLS_LAUNCH
  return hipGetLastError();
}

// The deferred-dx chain's per-channel finalize (see internal.h): with
// a = invstd1 g1, md = sd / M, mdn = sdn / M the next-to-be-applied dx is
//   dx = a (dxhat - md - (x - mu1) invstd1 mdn)
// and, x = ReLU(g2 uhat + b2) being the previous block's output (x = 0 off its
// mask m), the previous block's ReLU+BN2 backward sums follow from the prev-mode
// sums s1 = sum m dxhat, s2 = sum m dxhat uhat and that block's forward sums
// (cnt = sum m, su = sum m uhat, sum x, xu = sum x uhat):
//   sum m dx       = a (s1 - md cnt - mdn invstd1 (sum x - mu1 cnt))
//   sum m dx uhat  = a (s2 - md su  - mdn invstd1 (xu    - mu1 su))
__global__ void k_chain_coef(const double *sd, const double *sdn, const float *mean1,
                             const float *invstd1, const float *g1, const double *s1,
                             const double *s2, const double *xst, int C, double invM,
                             float *dg1, float *db1, float *coef, double *psum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double md = sd[c] * invM, mdn = sdn[c] * invM;
  const float af = invstd1[c] * g1[c];
  const double a = (double)af, is = (double)invstd1[c], mu = (double)mean1[c];
  const double sx = xst[c], cnt = xst[2 * C + c], su = xst[3 * C + c], xu = xst[4 * C + c];
  dg1[c] = (float)sdn[c];
  db1[c] = (float)sd[c];
  coef[c] = af;
  coef[C + c] = (float)md;
  coef[2 * C + c] = mean1[c];
  coef[3 * C + c] = invstd1[c];
  coef[4 * C + c] = (float)mdn;
  psum[c] = a * (s1[c] - md * cnt - mdn * is * (sx - mu * cnt));
  psum[C + c] = a * (s2[c] - md * su - mdn * is * (xu - mu * su));
}

hipError_t launch_chain_coef(const double *sd, const double *sdn, const BnRef &bn1,
                             const double *s1, const double *s2, const double *xst, int C,
                             int64_t M, float *dg1, float *db1, float *coef, double *psum,
                             hipStream_t s) {
  hipLaunchKernelGGL(k_chain_coef, dim3((C + 255) / 256), dim3(256), 0, s, sd, sdn, bn1.mean,
                     bn1.invstd, bn1.g, s1, s2, xst, C, 1.0 / (double)M, dg1, db1, coef, psum);
  return hipGetLastError();
}

__global__ void k_bn_grads_out(const double *sg, const double *sgu, const double *sdu, int C,
                               float *dgamma, float *dbeta, float *dbias) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  dgamma[c] = (float)sgu[c];
  dbeta[c] = (float)sg[c];
  if (dbias) dbias[c] = (float)sdu[c];
}

hipError_t launch_bn_grads_out(const double *sg, const double *sgu, const double *sdu, int C,
                               float *dgamma, float *dbeta, float *dbias, hipStream_t s) {
  hipLaunchKernelGGL(k_bn_grads_out, dim3((C + 255) / 256), dim3(256), 0, s, sg, sgu, sdu, C,
                     dgamma, dbeta, dbias);
  return hipGetLastError();
}

// dx = g*invstd * (dxhat - sum(dxhat)/M - xnorm * sum(dxhat*xnorm)/M), in place
// (invM = 0: eval mode, constant running statistics -> dx = g*invstd*dxhat).
// Optionally (pg2 != null) also the previous block's ReLU+BN2 backward sums:
// x = ReLU(g2*uhat + b2) of that block, so its ReLU mask is x > 0 and
// uhat = (x - b2) / g2 there; with dy_prev = dx:
//   psum[c] += sum dx * [x > 0],  psum[C + c] += sum dx * [x > 0] * uhat.
// The division loses precision when |b2| >> |g2| (and is undefined at g2 = 0):
// for such channels (|b2| > 4|g2|, a channel-uniform branch) uhat is read from
// the previous block's saved pre-BN2 tensor pU instead, exactly as that
// block's own reduction computes it: uhat = (U - mean2) * invstd2, mask
// (U - mean2) * invstd2*g2 + b2 > 0.
template <int VEC>
__global__ __launch_bounds__(256) void k_bn1_bwd_apply(float *dx, const float *x,
                                                       const float *mean, const float *invstd,
                                                       const float *g, const double *sd,
                                                       const double *sdn, const float *add,
                                                       int C, int L, double invM,
                                                       const float *pg2, const float *pb2,
                                                       double *psum, const float *pU,
                                                       const float *pmean, const float *pinvstd) {
  __shared__ double red[8];
  const int c = blockIdx.x, n = blockIdx.y;
  const int64_t base = ((int64_t)n * C + c) * L;
  const float mu = mean[c], is = invstd[c], a = is * g[c];
  const float md = bn_mean_term(sd[c], invM), mdn = bn_mean_term(sdn[c], invM);
  const float pg = pg2 ? pg2[c] : 1.f, pb = pg2 ? pb2[c] : 0.f;
  // poorly conditioned reconstruction (or g2 == 0 / non-finite): use U
  const bool from_u = pg2 && pU && !(fabsf(pb) <= 4.f * fabsf(pg));
  const float pmu = from_u ? pmean[c] : 0.f, pis = from_u ? pinvstd[c] : 1.f;
  const BnAff pbn = {pmu, pis, pis * pg, pb};  // the previous block's BN2
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x * VEC; i < L; i += 256 * VEC) {
    float xv[VEC], d[VEC];
    vld<VEC>(x + base + i, xv);
    vld<VEC>(dx + base + i, d);
#pragma unroll
    for (int j = 0; j < VEC; ++j) d[j] = a * (d[j] - md - bn_hat(xv[j], mu, is) * mdn);
    if (add) {
      float r[VEC];
      vld<VEC>(add + base + i, r);
#pragma unroll
      for (int j = 0; j < VEC; ++j) d[j] += r[j];
    }
    vst<VEC>(dx + base + i, d);
    if (from_u) {
      float u[VEC];
      vld<VEC>(pU + base + i, u);
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (relu_on(pbn.pre(u[j]))) {
          s += d[j];
          q += (double)d[j] * (double)pbn.hat(u[j]);
        }
    } else if (pg2) {
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (relu_on(xv[j])) {
          s += d[j];
          q += (double)d[j] * (double)((xv[j] - pb) / pg);
        }
    }
  }
  if (pg2) block_sum2_atomic<256>(s, q, psum + c, psum + C + c, red);
}

hipError_t launch_bn1_bwd_apply(float *dx, const float *x, const BnRef &bn1, const double *sd,
                                const double *sdn, const float *add, int N, int C, int L,
                                int64_t M, int training, const BnRef &pbn2, double *psum,
                                const float *pU, hipStream_t s) {
  STGCN_VEC_LAUNCH(k_bn1_bwd_apply, slice_vec(L, {dx, x, add, pU}), dim3(C, N), dx, x, bn1.mean,
                   bn1.invstd, bn1.g, sd, sdn, add, C, L, training ? 1.0 / (double)M : 0.0, pbn2.g,
                   pbn2.b, psum, pU, pbn2.mean, pbn2.invstd);
  return hipGetLastError();
}

// dout = dy * (y > 0) for the residual block's final ReLU (st_graphconv.py:105),
// with the per-channel sum of dout (the temporal and projection bias grads).
template <int VEC>
__global__ __launch_bounds__(256) void k_relu_bwd(const float *dy, const float *y, float *dout,
                                                  double *sum, int C, int L, float scale) {
  __shared__ double red[8];
  const int c = blockIdx.x, n = blockIdx.y;
  const int64_t base = ((int64_t)n * C + c) * L;
  double s = 0.0;
  for (int i = threadIdx.x * VEC; i < L; i += 256 * VEC) {
    float d[VEC], yv[VEC];
    vld<VEC>(dy + base + i, d);
    vld<VEC>(y + base + i, yv);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      d[j] = relu_on(yv[j]) ? d[j] * scale : 0.f;
      s += d[j];
    }
    vst<VEC>(dout + base + i, d);
  }
  block_sum2_atomic<256>(s, 0.0, sum + c, nullptr, red);
}

hipError_t launch_relu_bwd(const float *dy, const float *y, float *dout, double *sum, int N,
                           int C, int L, float scale, hipStream_t s) {
  STGCN_VEC_LAUNCH(k_relu_bwd, slice_vec(L, {dy, y, dout}), dim3(C, N), dy, y, dout, sum, C, L,
                   scale);
  return hipGetLastError();
}

}  // namespace stgcn
