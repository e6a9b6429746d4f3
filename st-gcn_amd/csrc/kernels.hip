// SpatialConv (graph convolution) kernels of libstgcn_hip.so — gfx950 (MI355X
// / CDNA4) only.
//
// The joint-axis (V) contractions with the dense adjacency A: the forward
// gathers (k_gather_fwd, k_gather3/4 on the VALU with A pinned in LDS,
// k_gather_mfma on the matrix cores), the fused backward kernels
// (k_spatial_bwd3/5/6, k_spatial_dx), the small dA / bias reductions, and the
// dispatch between them (launch_gather_fwd, launch_spatial_dx,
// spatial_dx_prev_supported). BatchNorm statistics accumulate in fp64. The
// fp32 conv GEMMs and weight gradients are in kernels_conv.hip, the BatchNorm
// / ReLU elementwise kernels in kernels_bn.hip.
//
// Wave size is 64; every block is a multiple of 64 threads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "device_common.h"
#include "internal.h"

namespace stgcn {

// ---------------------------------------------------------------------------
// Spatial (graph) kernels.
// ---------------------------------------------------------------------------
__global__ void k_pack_w(const float *W, float *Wpk, int K, int R, int C) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // co*(K*C) + k*C + ci
  const int KC = K * C;
  if (idx >= R * KC) return;
  const int co = idx / KC, rem = idx - co * KC, k = rem / C, ci = rem - k * C;
  Wpk[idx] = W[((int64_t)k * R + co) * C + ci];
}

hipError_t launch_pack_w(const float *W, float *Wpk, int K, int R, int C, hipStream_t s) {
  const int n = R * K * C;
  hipLaunchKernelGGL(k_pack_w, dim3((n + 255) / 256), dim3(256), 0, s, W, Wpk, K, R, C);
  return hipGetLastError();
}

// bias_rv[co][v] = sum_k bW[k*R+co] * sum_w A[k][v][w]   (the 1x1-conv bias
// pushed through the joint contraction: st_graphconv.py:148-150)
__global__ void k_bias_rv(const float *A, const float *bW, float *bias_rv, int K, int R, int V) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= R * V) return;
  const int co = idx / V, v = idx - co * V;
  double s = 0.0;
  for (int k = 0; k < K; ++k) {
    double ra = 0.0;
    for (int w = 0; w < V; ++w) ra += A[((int64_t)k * V + v) * V + w];
    s += (double)bW[k * R + co] * ra;
  }
  bias_rv[idx] = (float)s;
}

hipError_t launch_bias_rv(const float *A, const float *bW, float *bias_rv, int K, int R, int V,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_bias_rv, dim3((R * V + 255) / 256), dim3(256), 0, s, A, bW, bias_rv, K, R,
                     V);
  return hipGetLastError();
}

constexpr int kGatherTC = 32;  // frames per gather block

// G[n][k*C+ci][t][v] = sum_w A[k][v][w] * BN1(x)[n][ci][t][w]
// One block per (n, frame chunk); A pinned in LDS; loop over channels.
__global__ __launch_bounds__(256) void k_gather_fwd(const float *x, const float *mean,
                                                    const float *invstd, const float *g,
                                                    const float *b, const float *A, float *G,
                                                    int C, int T, int V, int K, int relu,
                                                    unsigned *amax) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *As = smem;                 // [K][V][V]
  float gm = 0.f;
  float *xs = smem + K * V * V;     // [TC][V]
  const int n = blockIdx.y, t0 = blockIdx.x * kGatherTC;
  int tc = T - t0;
  if (tc > kGatherTC) tc = kGatherTC;
  for (int i = threadIdx.x; i < K * V * V; i += 256) As[i] = A[i];
  const int L = T * V;
  const int nout = K * tc * V;
  for (int ci = 0; ci < C; ++ci) {
    __syncthreads();
    const float *src = x + ((int64_t)n * C + ci) * L + (int64_t)t0 * V;
    const BnAff bn = bn_aff(mean, invstd, g, b, ci);
    for (int i = threadIdx.x; i < tc * V; i += 256) {
      const float t = bn.pre(src[i]);
      xs[i] = relu ? relu_max(t) : t;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < nout; o += 256) {
      const int k = o / (tc * V);
      const int rem = o - k * tc * V;
      const int t = rem / V, v = rem - t * V;
      const float *ar = As + (k * V + v) * V;
      const float *xr = xs + t * V;
      float s = 0.f;
      for (int w = 0; w < V; ++w) s = fmaf(ar[w], xr[w], s);
      G[(((int64_t)n * K + k) * C + ci) * L + (int64_t)(t0 + t) * V + v] = s;
      gm = fmaxf(gm, amax_abs(s));
    }
  }
  if (amax) block_amax<256>(gm, amax);
}

// Joint-axis (V) kernels: rows padded to VP (multiple of 4) for 16-byte LDS reads.
template <int V>
struct JointCfg {
  static constexpr int VP = (V + 3) & ~3;
};

// ---------------------------------------------------------------------------
// Flat row-parallel joint kernels: one thread per (n, ci, t) row of the whole
// tensor (rows are contiguous in NCTV memory), RB rows per workgroup, no
// per-slice chunk loop. A sits in LDS ([K][V][VP], 16-B broadcast reads).
// ---------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void k_gather3(const float *__restrict__ x,
                                                 const float *__restrict__ mean,
                                                 const float *__restrict__ invstd,
                                                 const float *__restrict__ g,
                                                 const float *__restrict__ b,
                                                 const float *__restrict__ A, float *G, int C,
                                                 int T, int K, int64_t rows, int relu,
                                                 unsigned *amax) {
  constexpr int VP = JointCfg<V>::VP;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *As = smem;  // [K][V][VP]
  const int tid = threadIdx.x;
  for (int i = tid; i < K * V * VP; i += blockDim.x) {
    const int kv = i / VP, w = i - kv * VP;
    As[i] = w < V ? A[kv * V + w] : 0.f;
  }
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * blockDim.x + tid;
  const bool live = r0 < rows;
  const int64_t r = live ? r0 : rows - 1;  // (the last row again: every lane reaches wave_amax)
  float gm = 0.f;
  const int64_t CT = (int64_t)C * T;
  const int64_t n = r / CT;
  const int rem = (int)(r - n * CT);
  const int ci = rem / T, t = rem - ci * T;
  const BnAff bn = bn_aff(mean, invstd, g, b, ci);
  const float *xr = x + r * V;
  float xv[VP];
#pragma unroll
  for (int w = 0; w < VP; ++w) {
    const float t = w < V ? bn.pre(xr[w]) : 0.f;
    xv[w] = relu ? relu_max(t) : t;
  }
  for (int k = 0; k < K; ++k) {
    float *gout = G + ((n * K + k) * C + ci) * (int64_t)T * V + (int64_t)t * V;
    const float *Ak = As + k * V * VP;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      float acc = 0.f;
#pragma unroll
      for (int w4 = 0; w4 < VP; w4 += 4) {
        const float4 q = *reinterpret_cast<const float4 *>(Ak + v * VP + w4);
        acc = fmaf(q.x, xv[w4], acc);
        acc = fmaf(q.y, xv[w4 + 1], acc);
        acc = fmaf(q.z, xv[w4 + 2], acc);
        acc = fmaf(q.w, xv[w4 + 3], acc);
      }
      if (live) gout[v] = acc;
      gm = fmaxf(gm, amax_abs(acc));
    }
  }
  if (amax) block_amax<256>(gm, amax);
}

// k_gather4: k_gather3 with the block's rows moved through LDS: the 256 rows
// of a block are contiguous in x (256*V floats; the host checks that no block
// crosses a clip, so each partition's 256*V outputs are contiguous in G too),
// they arrive by 16-byte LDS-DMA, each thread contracts its row from LDS (A in
// LDS), and the outputs leave through LDS as float4 stores. (A persistent,
// double-buffered variant measured slower: fewer workgroups per CU.)
// pv.bn.mean non-null (ABI 8, STGCN_PLAN_X_FROM_U): x holds the previous block's U
// and the input is ReLU(BN2_prev(U)), formed as k_bn_relu_fwd forms its y.
template <int V>
__global__ __launch_bounds__(256) void k_gather4(const float *__restrict__ x,
                                                 const float *__restrict__ mean,
                                                 const float *__restrict__ invstd,
                                                 const float *__restrict__ g,
                                                 const float *__restrict__ b,
                                                 const float *__restrict__ A, float *G, int C,
                                                 int T, int K, int64_t rows, int relu,
                                                 unsigned *amax, PrevBn pv) {
  constexpr int VP = JointCfg<V>::VP;
  constexpr int BF = 256 * V;  // floats of a block (a multiple of 256: V DMA rounds)
  float gm = 0.f;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float *xs = smem;     // [256][V]
  float *os = xs + BF;  // [256][V]
  float *As = os + BF;  // [K][V][VP]
  const int64_t r0 = (int64_t)blockIdx.x * 256;
  {
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(x + r0 * V, BF);
    for (int i = wave; i < V; i += 4)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, xs + i * 256, 16, (unsigned)(i * 256 + lane * 4) * 4u,
                                               0, 0, 0);
  }
  for (int i = tid; i < K * V * VP; i += 256) {
    const int kv = i / VP, w = i - kv * VP;
    As[i] = w < V ? A[kv * V + w] : 0.f;
  }
  const int64_t CT = (int64_t)C * T;
  const int64_t n0 = r0 / CT, rem0 = r0 - n0 * CT;
  const int ci = (int)((rem0 + tid) / T);
  const float mu = mean[ci], a = invstd[ci] * g[ci], be = b[ci];
  const bool prev = pv.bn.mean != nullptr;
  const float pmu = prev ? pv.bn.mean[ci] : 0.f, pa = prev ? pv.bn.invstd[ci] * pv.bn.g[ci] : 0.f;
  const float pbe = prev ? pv.bn.b[ci] : 0.f;
  __syncthreads();
  float xv[VP];
#pragma unroll
  for (int w = 0; w < VP; ++w) {
    float xx = w < V ? xs[tid * V + w] : 0.f;
    if (prev) xx = bn_relu(bn_pre(xx, pmu, pa, pbe));
    const float t = w < V ? bn_pre(xx, mu, a, be) : 0.f;
    xv[w] = relu ? relu_max(t) : t;
  }
  for (int k = 0; k < K; ++k) {
    const float *Ak = As + k * V * VP;
    if (k > 0) __syncthreads();  // previous partition's stores have read os
#pragma unroll
    for (int v = 0; v < V; ++v) {
      float acc = 0.f;
#pragma unroll
      for (int w4 = 0; w4 < VP; w4 += 4) {
        const float4 q = *reinterpret_cast<const float4 *>(Ak + v * VP + w4);
        acc = fmaf(q.x, xv[w4], acc);
        acc = fmaf(q.y, xv[w4 + 1], acc);
        acc = fmaf(q.z, xv[w4 + 2], acc);
        acc = fmaf(q.w, xv[w4 + 3], acc);
      }
      os[tid * V + v] = acc;
    }
    __syncthreads();
    float *dst = G + ((n0 * K + k) * CT + rem0) * V;
    for (int e = tid; e < BF / 4; e += 256) {
      const float4 q = *reinterpret_cast<const float4 *>(os + e * 4);
      *reinterpret_cast<float4 *>(dst + e * 4) = q;
      gm = fmaxf(gm, fmaxf(fmaxf(amax_abs(q.x), amax_abs(q.y)),
                           fmaxf(amax_abs(q.z), amax_abs(q.w))));
    }
  }
  if (amax) block_amax<256>(gm, amax);
}

// Flat-row spatial backward (the math: see k_spatial_dx). Per block:
// dx rows, BN1 sums reduced per channel segment in LDS (rows are sorted by
// channel), dA over the block's rows on MFMA, wave partials summed in LDS.
template <int V>
__global__ __launch_bounds__(256) void k_spatial_bwd3(
    const float *__restrict__ H, const float *__restrict__ x, const float *__restrict__ mean,
    const float *__restrict__ invstd, const float *__restrict__ g, const float *__restrict__ b,
    const float *__restrict__ A, float *dx, float *dA, double *sd, double *sdn, int C, int T,
    int K, int64_t rows, int write_dx, int relu, float *dA_part) {
  constexpr int VP = JointCfg<V>::VP;
  constexpr int NT = (V + 31) / 32;
  constexpr int MAXSEG = 32;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ double seg_s[MAXSEG], seg_n[MAXSEG];
  const int RB = blockDim.x;
  float *As = smem;                 // [K][V][VP]
  float *Hs = As + K * V * VP;      // [K][RB][V]
  float *XBs = Hs + K * RB * V;     // [RB][VP] BN1(x)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, lo = lane & 31;
  for (int i = tid; i < K * V * VP; i += RB) {
    const int kv = i / VP, w = i - kv * VP;
    As[i] = w < V ? A[kv * V + w] : 0.f;
  }
  if (tid < MAXSEG) seg_s[tid] = seg_n[tid] = 0.0;
  const int64_t r0 = (int64_t)blockIdx.x * RB;
  const int64_t r = r0 + tid;
  const bool live = r < rows;
  const int64_t CT = (int64_t)C * T;
  // channel segment of this row relative to the block's first row
  const int64_t cfirst = (r0 / CT) * C + (int)((r0 % CT) / T);  // global (n*C + ci) of row r0
  int64_t n = 0;
  int ci = 0, t = 0;
  if (live) {
    n = r / CT;
    const int rem = (int)(r - n * CT);
    ci = rem / T;
    t = rem - ci * T;
  }
  const int seg = live ? (int)((n * C + ci) - cfirst) : 0;
  const bool seg_lds = (RB + T - 1) / T + 1 <= MAXSEG;
  __syncthreads();
  float s = 0.f, sn = 0.f;
  if (live) {
    const float mu = mean[ci], is = invstd[ci], a = is * g[ci], be = b[ci];
    const float *xr = x + r * V;
    float xv[VP];
#pragma unroll
    for (int w = 0; w < VP; ++w) xv[w] = w < V ? xr[w] : 0.f;
    float acc[VP];
#pragma unroll
    for (int w = 0; w < VP; ++w) acc[w] = 0.f;
    for (int k = 0; k < K; ++k) {
      const float *hr = H + ((n * K + k) * C + ci) * (int64_t)T * V + (int64_t)t * V;
      const float *Ak = As + k * V * VP;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const float h = hr[v];
        Hs[(k * RB + tid) * V + v] = h;
#pragma unroll
        for (int w4 = 0; w4 < VP; w4 += 4) {
          const float4 q = *reinterpret_cast<const float4 *>(Ak + v * VP + w4);
          acc[w4] = fmaf(h, q.x, acc[w4]);
          acc[w4 + 1] = fmaf(h, q.y, acc[w4 + 1]);
          acc[w4 + 2] = fmaf(h, q.z, acc[w4 + 2]);
          acc[w4 + 3] = fmaf(h, q.w, acc[w4 + 3]);
        }
      }
    }
    float *dxr = dx + r * V;
#pragma unroll
    for (int w = 0; w < V; ++w) {
      const float xn = bn_hat(xv[w], mu, is);
      const float bn = bn_pre(xv[w], mu, a, be);
      if (relu && bn <= 0.f) acc[w] = 0.f;  // ReLU'(BN1(x))
      s += acc[w];
      sn = fmaf(acc[w], xn, sn);
      if (write_dx) dxr[w] = acc[w];
      XBs[tid * VP + w] = relu ? relu_max(bn) : bn;
    }
  } else {
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int v = 0; v < V; ++v) Hs[(k * RB + tid) * V + v] = 0.f;
#pragma unroll
    for (int w = 0; w < V; ++w) XBs[tid * VP + w] = 0.f;
  }
  // BN1 partial sums per channel segment
  if (seg_lds) {
    if (live) {
      atomicAdd(&seg_s[seg], (double)s);
      atomicAdd(&seg_n[seg], (double)sn);
    }
  } else if (live) {
    atomicAdd(sd + ci, (double)s);
    atomicAdd(sdn + ci, (double)sn);
  }
  __syncthreads();
  if (seg_lds && tid < MAXSEG) {
    const int64_t gc = cfirst + tid;  // global (n*C + ci)
    const int64_t rlast = min(r0 + RB, rows) - 1;
    const int64_t glast = (rlast / CT) * C + (int)((rlast % CT) / T);
    if (gc <= glast) {
      const int cc = (int)(gc % C);
      atomicAdd(sd + cc, seg_s[tid]);
      atomicAdd(sdn + cc, seg_n[tid]);
    }
  }
  // dA on MFMA over the block's rows (wave takes row pairs kk = wave, +nw, ...);
  // each wave's tiles go to its own slice [wave][K][DW][DW] (one owner lane per
  // entry: plain stores), summed over the waves in wave order below
  const int nw = RB / 64;
  const int nk = RB / 2;
  const int DW = NT * 32;
  float *dred = XBs + RB * VP + wave * K * DW * DW;
  __syncthreads();
  for (int k = 0; k < K; ++k) {
    floatx16 dacc[NT][NT];
#pragma unroll
    for (int p2 = 0; p2 < NT; ++p2)
#pragma unroll
      for (int q2 = 0; q2 < NT; ++q2)
#pragma unroll
        for (int i = 0; i < 16; ++i) dacc[p2][q2][i] = 0.f;
    const float *hk = Hs + k * RB * V;
    for (int kk = wave; kk < nk; kk += nw) {
      const int rr = 2 * kk + hi;
#pragma unroll
      for (int p2 = 0; p2 < NT; ++p2) {
        const int v = p2 * 32 + lo;
        const float av = v < V ? hk[rr * V + v] : 0.f;
#pragma unroll
        for (int q2 = 0; q2 < NT; ++q2) {
          const int w = q2 * 32 + lo;
          const float bw = w < V ? XBs[rr * VP + w] : 0.f;
          dacc[p2][q2] = mfma32(av, bw, dacc[p2][q2]);
        }
      }
    }
#pragma unroll
    for (int p2 = 0; p2 < NT; ++p2)
#pragma unroll
      for (int q2 = 0; q2 < NT; ++q2)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int v = p2 * 32 + (i & 3) + 8 * (i >> 2) + 4 * hi;
          const int w = q2 * 32 + lo;
          if (v < V && w < V) dred[(k * DW + v) * DW + w] = dacc[p2][q2][i];
        }
  }
  __syncthreads();
  const float *dw0 = XBs + RB * VP;
  for (int i = tid; i < K * V * V; i += RB) {
    const int k = i / (V * V), rem = i - k * V * V, v = rem / V, w = rem - v * V;
    float sum = 0.f;
    for (int wv = 0; wv < nw; ++wv) sum += dw0[((wv * K + k) * DW + v) * DW + w];
    if (dA_part)  // (deterministic: launch_dA_reduce adds the partials in order)
      dA_part[(int64_t)blockIdx.x * K * V * V + i] = sum;
    else
      atomicAdd(dA + i, sum);
  }
}

// Row-pass sums of k_spatial_bwd5 / _bwd6 (float sv[4]: sd, sdn and, in prev
// mode, s1, s2 of PrevBn; ns of them), reduced per channel segment of the
// block: a wave whose rows share one channel reduces once; LDS segment
// accumulators (the kernel's __shared__ segv[4][MAXSEG]) when the block spans
// few channels, else global fp64 atomics. (A macro: the LDS array must stay a
// visible __shared__ object at the atomics, or hipcc mis-selects them.)
#define STGCN_ROWPASS_SUMS(sv, ns, seg, ci)                                   \
  do {                                                                        \
    const int seg0_ = __builtin_amdgcn_readfirstlane(seg);                    \
    if (__builtin_amdgcn_ballot_w64((seg) != seg0_) == 0) {                   \
      for (int i_ = 0; i_ < (ns); ++i_) {                                     \
        const double w_ = wave_sum((double)(sv)[i_]);                         \
        if (lane == 0) {                                                      \
          if (seg_lds)                                                        \
            atomicAdd(&segv[i_][seg0_], w_);                                  \
          else                                                                \
            atomicAdd(gdst[i_] + (ci), w_);                                   \
        }                                                                     \
      }                                                                       \
    } else {                                                                  \
      for (int i_ = 0; i_ < (ns); ++i_) {                                     \
        if (seg_lds)                                                          \
          atomicAdd(&segv[i_][seg], (double)(sv)[i_]);                        \
        else                                                                  \
          atomicAdd(gdst[i_] + (ci), (double)(sv)[i_]);                       \
      }                                                                       \
    }                                                                         \
  } while (0)

// k_spatial_bwd5: the spatial backward with both joint contractions on MFMA.
// Persistent and double-buffered like k_spatial_bwd4 (row blocks of RB rows,
// contiguous in x, dx and per partition in H; H planes and x by 16-byte
// LDS-DMA). Per block:
//   dx[row][w] = sum_k sum_v H_k[row][v] A_k[v][w]   MFMA, A_k resident in VGPRs
//                                                    as the B operand (k = v)
//   BN1 sums per row from the dx tile in LDS, BN1(x) in place (one thread/row)
//   dA_k[v][w] += sum_rows H_k[row][v] BN1(x)[row][w]  MFMA, LDS accumulator
// dx leaves through LDS as float4 stores. With 3 partitions, 8 waves (two per
// SIMD): wave w takes dx row tile w & 3 (if < RB/32) over half w >> 2 of the
// joint reduction (the halves meet in LDS and are summed by the row pass), and
// rows 2(w + 8j) + h of the dA partials; with 1 or 2 partitions 4 waves and
// the whole reduction per wave (measured: 8 waves are slower at V = 18, K = 1,
// 7% faster at V = 25, K = 3). Requires K * ceil(V/2) * ceil(V/32) <= 48 (B-operand
// registers) and the k_spatial_bwd4 host conditions.
constexpr int bwd5_nw(int kmax) { return kmax >= 3 ? 8 : 4; }

template <int V, int RB, int KMAX>
__global__ __launch_bounds__(bwd5_nw(KMAX) * 64) void k_spatial_bwd5(
    const float *__restrict__ H, const float *__restrict__ x, const float *__restrict__ mean,
    const float *__restrict__ invstd, const float *__restrict__ g, const float *__restrict__ b,
    const float *__restrict__ A, float *dx, float *dA, double *sd, double *sdn, int C, int T,
    int K, int64_t rows, int write_dx, int relu, PrevBn prev, float *dA_part) {
  constexpr int VH = (V + 1) / 2;           // MFMA k-steps over v
  constexpr int NW = bwd5_nw(KMAX);         // waves
  constexpr int NH = NW / 4;                // reduction halves of the dx GEMM
  constexpr int VQ = (VH + NH - 1) / NH;    // MFMA k-steps per half
  constexpr int NT = (V + 31) / 32;         // 32-column output tiles over w
  constexpr int DW = NT * 32;
  constexpr int MAXSEG = 32;
  constexpr int PL = (RB * V + 255) / 256 * 256;  // plane pitch: whole 16-byte DMA rounds
  constexpr int NRT = RB / 32;                    // 32-row tiles per block
  constexpr bool DREG = KMAX * NT * NT <= 4;      // dA accumulators resident in VGPRs
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ double segv[4][MAXSEG];  // [sd | sdn | s1 | s2] per channel segment
  const int BUF = (K + 1) * PL;  // one buffer: K H planes + x plane (prev mode: U)
  float *dxs = smem + 2 * BUF;   // [RB][V]: reduction half 0, then dx
  float *dxs2 = dxs + PL;        // [RB][V]: reduction half 1 (NH == 2)
  const bool pv = prev.bn.mean != nullptr;
  const int ns = pv ? 4 : 2;
  double *const gdst[4] = {sd, sdn, prev.s1, prev.s2};
  float *dred = dxs + NH * PL;   // [K][DW][DW]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, lo = lane & 31;
  const int CT = C * T;  // rows per clip (rows < 2^31: host check)
  const int nblocks = (int)(rows / RB);
  const bool seg_lds = (RB + T - 1) / T + 1 <= MAXSEG;

  const int kh = wave >> 2, rtile = wave & 3;  // dx reduction half, row tile
  // B operand of the dx GEMM, this wave's half: Bm[k][j][t] = A_k[v = 2(kh VQ + j) + hi]
  // [w = 32t + lo] (0 outside)
  float Bm[KMAX][VQ][NT];
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
#pragma unroll
    for (int s2 = 0; s2 < VQ; ++s2)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int v = 2 * (kh * VQ + s2) + hi, w = 32 * t + lo;
        Bm[k][s2][t] = (k < K && v < V && w < V) ? A[(k * V + v) * V + w] : 0.f;
      }

  auto stage = [&](int blk, float *buf) {
    const int r0 = blk * RB;
    const int n0 = r0 / CT, rem0 = r0 - n0 * CT;
    constexpr int ND = PL / 256;  // DMA rounds per plane
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(x + (int64_t)r0 * V, (int64_t)RB * V);
    for (int i = wave; i < ND; i += NW)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, buf + K * PL + i * 256, 16,
                                               (unsigned)(i * 256 + lane * 4) * 4u, 0, 0, 0);
    for (int k = 0; k < K; ++k) {
      const __amdgpu_buffer_rsrc_t rh =
          make_rsrc(H + ((int64_t)(n0 * K + k) * CT + rem0) * V, (int64_t)RB * V);
      for (int i = wave; i < ND; i += NW)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rh, buf + k * PL + i * 256, 16,
                                                 (unsigned)(i * 256 + lane * 4) * 4u, 0, 0, 0);
    }
  };

  for (int i = tid; i < K * DW * DW; i += NW * 64) dred[i] = 0.f;
  floatx16 dacc[DREG ? KMAX : 1][NT][NT];
  auto zero_dacc = [&](int kd) {
#pragma unroll
    for (int p2 = 0; p2 < NT; ++p2)
#pragma unroll
      for (int q2 = 0; q2 < NT; ++q2)
#pragma unroll
        for (int i = 0; i < 16; ++i) dacc[kd][p2][q2][i] = 0.f;
  };
#pragma unroll
  for (int kd = 0; kd < (DREG ? KMAX : 1); ++kd) zero_dacc(kd);
  // dacc[kd] -> dred[k] (LDS atomics), then zero
  auto flush_dacc = [&](int k) {
    const int kd = DREG ? k : 0;
#pragma unroll
    for (int p2 = 0; p2 < NT; ++p2)
#pragma unroll
      for (int q2 = 0; q2 < NT; ++q2)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int v = p2 * 32 + (i & 3) + 8 * (i >> 2) + 4 * hi;
          const int w = q2 * 32 + lo;
          if (v < V && w < V) atomicAdd(dred + (k * DW + v) * DW + w, dacc[kd][p2][q2][i]);
        }
    zero_dacc(kd);
  };
  int blk = blockIdx.x;
  if (blk < nblocks) stage(blk, smem);
  for (int it = 0; blk < nblocks; ++it, blk += gridDim.x) {
    float *buf = smem + (it & 1) * BUF;
    float *Hs = buf, *xs = buf + K * PL;
    if (tid < MAXSEG) segv[0][tid] = segv[1][tid] = segv[2][tid] = segv[3][tid] = 0.0;
    __syncthreads();  // block blk staged (vmcnt(0)); previous block fully retired
    if (blk + (int)gridDim.x < nblocks) stage(blk + gridDim.x, smem + ((it + 1) & 1) * BUF);
    const int r0 = blk * RB;
    const int n0 = r0 / CT, rem0 = r0 - n0 * CT;
    const int cfirst = n0 * C + rem0 / T;  // global (n*C + ci) of row r0
    // dx tile rtile (32 rows), reduction half kh, on MFMA (RB = 64: waves 2, 3,
    // 6, 7 idle here)
    if (rtile < NRT) {
      floatx16 acc[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
          const float *hr = Hs + k * PL + (rtile * 32 + lo) * V + hi + 2 * kh * VQ;
#pragma unroll
          for (int s2 = 0; s2 < VQ; ++s2) {
            const float av = (2 * (kh * VQ + s2) + hi < V) ? hr[2 * s2] : 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = mfma32(av, Bm[k][s2][t], acc[t]);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = rtile * 32 + (i & 3) + 8 * (i >> 2) + 4 * hi;
          const int w = 32 * t + lo;
          if (w < V) (kh ? dxs2 : dxs)[row * V + w] = acc[t][i];
        }
    }
    __syncthreads();  // dx tile complete
    // per row (TPR threads each, interleaved joints): BN1 sums, BN1(x) in
    // place; per-channel-segment sums (a wave's rows usually share one
    // channel: then one wave reduction)
    {
      constexpr int TPR = NW * 64 / RB;
      const int rl = tid / TPR, part = tid % TPR;
      const int rem = rem0 + rl;
      const int ci = rem / T;
      const int seg = n0 * C + ci - cfirst;
      const BnAff bn1 = bn_aff(mean, invstd, g, b, ci);
      // prev mode: the staged plane is the previous block's U
      const float pmu = pv ? prev.bn.mean[ci] : 0.f, pis = pv ? prev.bn.invstd[ci] : 1.f;
      const float pa = pv ? pis * prev.bn.g[ci] : 1.f, pb = pv ? prev.bn.b[ci] : 0.f;
      float sv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < (V + TPR - 1) / TPR; ++j) {
        const int w = part + j * TPR;
        if (w < V) {
          float xv = xs[rl * V + w];
          float uh = 0.f;
          bool pm = false;
          if (pv) {
            const float t = bn_pre(xv, pmu, pa, pb);
            uh = bn_hat(xv, pmu, pis);
            pm = relu_on(t);
            xv = pm ? t : 0.f;
          }
          float d = NH == 2 ? dxs[rl * V + w] + dxs2[rl * V + w] : dxs[rl * V + w];
          const float bn = bn1.pre(xv);
          if (relu && bn <= 0.f) d = 0.f;  // ReLU'(BN1(x))
          dxs[rl * V + w] = d;
          sv[0] += d;
          sv[1] = fmaf(d, bn1.hat(xv), sv[1]);
          if (pm) {
            sv[2] += d;
            sv[3] = fmaf(d, uh, sv[3]);
          }
          xs[rl * V + w] = relu ? relu_max(bn) : bn;
        }
      }
      STGCN_ROWPASS_SUMS(sv, ns, seg, ci);
    }
    __syncthreads();  // BN1(x) rows and segment sums complete
    if (seg_lds && tid < MAXSEG) {
      const int gc = cfirst + tid;  // global (n*C + ci)
      const int rlast = r0 + RB - 1;
      const int glast = (rlast / CT) * C + (rlast % CT) / T;
      if (gc <= glast) {
        const int cc = gc % C;
        for (int i = 0; i < ns; ++i) atomicAdd(gdst[i] + cc, segv[i][tid]);
      }
    }
    // dA partials on MFMA: wave takes row pairs kk = wave + 8j; accumulators
    // stay in registers across blocks (DREG) or are flushed per block
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < K) {
        floatx16(&dk)[NT][NT] = dacc[DREG ? k : 0];
        const float *hk = Hs + k * PL;
#pragma unroll
        for (int j = 0; j < RB / (2 * NW); ++j) {
          const int rr = 2 * (wave + NW * j) + hi;
          float av[NT], bw[NT];
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const int c = t * 32 + lo;
            av[t] = c < V ? hk[rr * V + c] : 0.f;
            bw[t] = c < V ? xs[rr * V + c] : 0.f;
          }
#pragma unroll
          for (int p2 = 0; p2 < NT; ++p2)
#pragma unroll
            for (int q2 = 0; q2 < NT; ++q2) dk[p2][q2] = mfma32(av[p2], bw[q2], dk[p2][q2]);
        }
        if (!DREG) flush_dacc(k);
      }
    }
    if (write_dx) {
      float *dst = dx + (int64_t)r0 * V;
      for (int e = tid; e < RB * V / 4; e += NW * 64)
        *reinterpret_cast<float4 *>(dst + e * 4) = *reinterpret_cast<const float4 *>(dxs + e * 4);
    }
  }
  if constexpr (DREG) {
    // the waves' register tiles into the zeroed LDS accumulator one wave after
    // the other (plain adds, one owner lane per entry): a fixed order
    __syncthreads();
    for (int wv = 0; wv < NW; ++wv) {
      if (wave == wv) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < K) {
#pragma unroll
            for (int p2 = 0; p2 < NT; ++p2)
#pragma unroll
              for (int q2 = 0; q2 < NT; ++q2)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                  const int v = p2 * 32 + (i & 3) + 8 * (i >> 2) + 4 * hi;
                  const int w = q2 * 32 + lo;
                  if (v < V && w < V) dred[(k * DW + v) * DW + w] += dacc[k][p2][q2][i];
                }
          }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  for (int i = tid; i < K * V * V; i += NW * 64) {
    const int k = i / (V * V), rm = i - k * V * V, v = rm / V, w = rm - v * V;
    if (dA_part)  // (deterministic: launch_dA_reduce adds the partials in order)
      dA_part[(int64_t)blockIdx.x * K * V * V + i] = dred[(k * DW + v) * DW + w];
    else
      atomicAdd(dA + i, dred[(k * DW + v) * DW + w]);
  }
}

template <int V, int RB>
static size_t bwd5_lds(int K) {
  constexpr int PL = (RB * V + 255) / 256 * 256;
  constexpr int DW = (V + 31) / 32 * 32;
  const int nh = bwd5_nw(K) / 4;
  return sizeof(float) * ((size_t)(2 * (K + 1) + nh) * PL + (size_t)K * DW * DW);
}

// (dry: whether the kernel takes the shape; nothing but b's shape is read)
template <int V, int RB, int KT>
static bool launch_bwd5(const SpatialBwd &b, int64_t rows, bool dry, hipStream_t s) {
  const size_t lds = bwd5_lds<V, RB>(b.K);
  if (lds > 160 * 1024 - 1024 || ((int64_t)b.C * b.T) % RB != 0 || rows >= (int64_t)1 << 31)
    return false;
  const int per_cu = std::max(1, std::min(8, (int)((160 * 1024) / (lds + 1024))));
  const dim3 grid((unsigned)std::min<int64_t>(rows / RB, 256 * per_cu));
  if (b.K != KT) return false;
  if (dry) return true;
  float *part = b.dA_part && (int64_t)grid.x <= b.part_cap ? b.dA_part : nullptr;
  if (part && b.nparts) *b.nparts = grid.x;
  hipLaunchKernelGGL((k_spatial_bwd5<V, RB, KT>), grid, dim3(bwd5_nw(KT) * 64), lds, s, b.in, b.x,
                     b.bn.mean, b.bn.invstd, b.bn.g, b.bn.b, b.A, b.dx, b.dA, b.sd, b.sdn, b.C, b.T,
                     b.K, rows, b.write_dx, b.relu, b.prev, part);
  return true;
}

// k_spatial_bwd6: k_spatial_bwd5 for joint counts above 32 (two 32-column
// output tiles, V = 50: the two-person graph) with up to 3 partitions, where
// bwd5's register-resident B operand (all column tiles) and LDS dA accumulator
// do not fit. RB = 64 rows per block, 8 waves (two per SIMD, so one wave's LDS
// reads and row pass run under the other's MFMAs): dx = 2 row tiles x 2 column
// tiles x 2 halves of the joint reduction (wave = tile + 4 * half, each half
// keeping only its k-steps of its column tile of A_k as the B operand:
// K * 13 VGPRs; the halves meet in LDS, summed by the row pass); the K x 2 x 2
// dA tiles x 2 row halves of the block are dealt to the 8 waves (K each) and
// stay in registers for the whole persistent loop, flushed once by global
// atomics. Staging, BN1 sums and the dx store as in bwd5.
// (dA by the exact 3-way bf16 split of device_common.h, split_bf16x3.)

// BF (STGCN_F_BF16 blocks): H and A to 2^-16 (h + m planes; the dropped terms
// are below 2^-16 of each product), f(BN1(x)) of the dA GEMM to bf16: three
// products for dx and two for dA instead of six each. (H to bf16 alone moved
// the residual V = 50 block's BN1 bias gradient to 4.5x the bf16 reference's
// own error, past the 3x gate.)
template <int V, int KMAX, bool BF>
__global__ __launch_bounds__(512, 1) void k_spatial_bwd6(
    const float *__restrict__ H, const float *__restrict__ x, const float *__restrict__ mean,
    const float *__restrict__ invstd, const float *__restrict__ g, const float *__restrict__ b,
    const float *__restrict__ A, float *dx, float *dA, double *sd, double *sdn, int C, int T,
    int K, int64_t rows, int write_dx, int relu, PrevBn prev, float *dA_part) {
  constexpr int RB = 64, NW = 8;
  static_assert(V > 32 && V <= 64, "two 32-column tiles");
  constexpr int MAXSEG = 32;
  constexpr int PL = (RB * V + 255) / 256 * 256;  // plane pitch: whole 16-byte DMA rounds
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ double segv[4][MAXSEG];  // [sd | sdn | s1 | s2] per channel segment
  const int BUF = (K + 1) * PL;  // one buffer: K H planes + x plane (prev mode: U)
  float *dxs = smem + 2 * BUF;   // [RB][V]: reduction half 0, then dx
  float *dxs2 = dxs + PL;        // [RB][V]: reduction half 1
  const bool pv = prev.bn.mean != nullptr;
  const int ns = pv ? 4 : 2;
  double *const gdst[4] = {sd, sdn, prev.s1, prev.s2};
  // f(BN1(x)) split into 3 bf16 planes, joint-major [w][row] (pitch XTP: 16-byte
  // row groups at an odd 16-byte stride), the dA GEMM's B operand
  constexpr int XTP = RB + 8, XTPL = V * XTP * 2;
  char *XT = reinterpret_cast<char *>(dxs2 + PL);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, lo = lane & 31;
  const int CT = C * T;
  const int nblocks = (int)(rows / RB);
  const bool seg_lds = (RB + T - 1) / T + 1 <= MAXSEG;
  const int rt = wave & 1, ct = (wave >> 1) & 1, kh = wave >> 2;  // this wave's dx tile, half

  // B operand of the dx GEMM (v_mfma_f32_32x32x16_bf16 on exact 3-way splits):
  // column tile ct, joints v = 32 kh + 16 ks + 8 hi + j (ks = 0, 1): this wave's
  // half of the reduction, A_k[v][w = 32ct + lo] split into h / m / l planes
  uint4 Bh[KMAX][2], Bmd[KMAX][2], Bl[KMAX][2];
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int v0 = 32 * kh + 16 * ks + 8 * hi, w = 32 * ct + lo;
      float bv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        bv[j] = (k < K && v0 + j < V && w < V) ? A[(k * V + v0 + j) * V + w] : 0.f;
      split_bf16x3(bv[0], bv[1], Bh[k][ks].x, Bmd[k][ks].x, Bl[k][ks].x);
      split_bf16x3(bv[2], bv[3], Bh[k][ks].y, Bmd[k][ks].y, Bl[k][ks].y);
      split_bf16x3(bv[4], bv[5], Bh[k][ks].z, Bmd[k][ks].z, Bl[k][ks].z);
      split_bf16x3(bv[6], bv[7], Bh[k][ks].w, Bmd[k][ks].w, Bl[k][ks].w);
    }

  auto stage = [&](int blk, float *buf) {
    const int r0 = blk * RB;
    const int n0 = r0 / CT, rem0 = r0 - n0 * CT;
    constexpr int ND = PL / 256;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(x + (int64_t)r0 * V, (int64_t)RB * V);
    for (int i = wave; i < ND; i += NW)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, buf + K * PL + i * 256, 16,
                                               (unsigned)(i * 256 + lane * 4) * 4u, 0, 0, 0);
    for (int k = 0; k < K; ++k) {
      const __amdgpu_buffer_rsrc_t rh =
          make_rsrc(H + ((int64_t)(n0 * K + k) * CT + rem0) * V, (int64_t)RB * V);
      for (int i = wave; i < ND; i += NW)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rh, buf + k * PL + i * 256, 16,
                                                 (unsigned)(i * 256 + lane * 4) * 4u, 0, 0, 0);
    }
  };

  // dA tiles of this wave: j = (wave & 3) + 4i (i < KMAX) -> (k = i, p2 = (j / 2) & 1,
  // q2 = j & 1), over rows kh*32..+31 of each block
  floatx16 dacc[KMAX], dacl[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) dacc[i][e] = dacl[i][e] = 0.f;

  int blk = blockIdx.x;
  if (blk < nblocks) stage(blk, smem);
  for (int it = 0; blk < nblocks; ++it, blk += gridDim.x) {
    float *buf = smem + (it & 1) * BUF;
    float *Hs = buf, *xs = buf + K * PL;
    if (tid < MAXSEG) segv[0][tid] = segv[1][tid] = segv[2][tid] = segv[3][tid] = 0.0;
    __syncthreads();  // block blk staged (vmcnt(0)); previous block fully retired
    if (blk + (int)gridDim.x < nblocks) stage(blk + gridDim.x, smem + ((it + 1) & 1) * BUF);
    const int r0 = blk * RB;
    const int n0 = r0 / CT, rem0 = r0 - n0 * CT;
    const int cfirst = n0 * C + rem0 / T;
    {  // dx tile (rt, ct), reduction half kh: six bf16 products per fp32 product
      floatx16 acc, acl;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = acl[i] = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const int v0 = 32 * kh + 16 * ks + 8 * hi;
            const float *hr = Hs + k * PL + (rt * 32 + lo) * V + v0;
            float av[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) av[j] = v0 + j < V ? hr[j] : 0.f;
            uint4 ah, am, al;
            split_bf16x3(av[0], av[1], ah.x, am.x, al.x);
            split_bf16x3(av[2], av[3], ah.y, am.y, al.y);
            split_bf16x3(av[4], av[5], ah.z, am.z, al.z);
            split_bf16x3(av[6], av[7], ah.w, am.w, al.w);
            acc = mfma_bf16(ah, Bh[k][ks], acc);
            acl = mfma_bf16(ah, Bmd[k][ks], acl);
            acl = mfma_bf16(am, Bh[k][ks], acl);
            if constexpr (!BF) {
              acl = mfma_bf16(ah, Bl[k][ks], acl);
              acl = mfma_bf16(am, Bmd[k][ks], acl);
              acl = mfma_bf16(al, Bh[k][ks], acl);
            }
          }
        }
      }
      acc += acl;
      float *dst = kh ? dxs2 : dxs;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = rt * 32 + (i & 3) + 8 * (i >> 2) + 4 * hi;
        const int w = 32 * ct + lo;
        if (w < V) dst[row * V + w] = acc[i];
      }
    }
    __syncthreads();  // dx tile halves complete
    {  // per row (8 threads each): dx = sum of halves, BN1 sums, BN1(x) in place (see bwd5)
      constexpr int TPR = NW * 64 / RB;
      const int rl = tid / TPR, part = tid % TPR;
      const int rem = rem0 + rl;
      const int ci = rem / T;
      const int seg = n0 * C + ci - cfirst;
      const BnAff bn1 = bn_aff(mean, invstd, g, b, ci);
      const float pmu = pv ? prev.bn.mean[ci] : 0.f, pis = pv ? prev.bn.invstd[ci] : 1.f;
      const float pa = pv ? pis * prev.bn.g[ci] : 1.f, pb = pv ? prev.bn.b[ci] : 0.f;
      float sv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < (V + TPR - 1) / TPR; ++j) {
        const int w = part + j * TPR;
        if (w < V) {
          float xv = xs[rl * V + w];
          float uh = 0.f;
          bool pm = false;
          if (pv) {  // prev mode: the staged plane is the previous block's U (see bwd5)
            const float t = bn_pre(xv, pmu, pa, pb);
            uh = bn_hat(xv, pmu, pis);
            pm = relu_on(t);
            xv = pm ? t : 0.f;
          }
          float d = dxs[rl * V + w] + dxs2[rl * V + w];
          const float bn = bn1.pre(xv);
          if (relu && bn <= 0.f) d = 0.f;
          dxs[rl * V + w] = d;
          sv[0] += d;
          sv[1] = fmaf(d, bn1.hat(xv), sv[1]);
          if (pm) {
            sv[2] += d;
            sv[3] = fmaf(d, uh, sv[3]);
          }
          const float f = relu ? relu_max(bn) : bn;
          const __bf16 fh = (__bf16)f;
          __bf16 *xt = reinterpret_cast<__bf16 *>(XT) + w * XTP + rl;
          xt[0] = fh;
          if constexpr (!BF) {
            const float r1 = f - (float)fh;
            const __bf16 fm = (__bf16)r1;
            xt[XTPL / 2] = fm;
            xt[XTPL] = (__bf16)(r1 - (float)fm);
          }
        }
      }
      STGCN_ROWPASS_SUMS(sv, ns, seg, ci);
    }
    __syncthreads();  // BN1(x) rows, dx and segment sums complete
    if (seg_lds && tid < MAXSEG) {
      const int gc = cfirst + tid;
      const int rlast = r0 + RB - 1;
      const int glast = (rlast / CT) * C + (rlast % CT) / T;
      if (gc <= glast) {
        const int cc = gc % C;
        for (int i = 0; i < ns; ++i) atomicAdd(gdst[i] + cc, segv[i][tid]);
      }
    }
    // dA tiles: dA_k[v in p2][w in q2] += sum_rows H_k[row][v] f(BN1(x))[row][w],
    // rows kh*32..+31 as two 16-row k-steps of v_mfma_f32_32x32x16_bf16 on the
    // exact 3-way splits: six products, h*h apart from the five cross terms
    {
      const int p2 = (wave >> 1) & 1, q2 = wave & 1;
      const int cv = p2 * 32 + lo, cw = q2 * 32 + lo;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int rb = kh * 32 + ks * 16 + 8 * hi;  // this lane's 8 rows
        uint4 bh = {0, 0, 0, 0}, bm = bh, bl = bh;
        if (cw < V) {
          const char *xt = XT + (cw * XTP + rb) * 2;
          bh = *reinterpret_cast<const uint4 *>(xt);
          if constexpr (!BF) {
            bm = *reinterpret_cast<const uint4 *>(xt + XTPL);
            bl = *reinterpret_cast<const uint4 *>(xt + 2 * XTPL);
          }
        }
#pragma unroll
        for (int i = 0; i < KMAX; ++i) {
          if (i < K) {
            const float *hk = Hs + i * PL + rb * V + cv;
            float av[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) av[e] = cv < V ? hk[e * V] : 0.f;
            uint4 ah, am, al;
            split_bf16x3(av[0], av[1], ah.x, am.x, al.x);
            split_bf16x3(av[2], av[3], ah.y, am.y, al.y);
            split_bf16x3(av[4], av[5], ah.z, am.z, al.z);
            split_bf16x3(av[6], av[7], ah.w, am.w, al.w);
            dacc[i] = mfma_bf16(ah, bh, dacc[i]);
            dacl[i] = mfma_bf16(am, bh, dacl[i]);
            if constexpr (!BF) {
              dacl[i] = mfma_bf16(ah, bm, dacl[i]);
              dacl[i] = mfma_bf16(ah, bl, dacl[i]);
              dacl[i] = mfma_bf16(am, bm, dacl[i]);
              dacl[i] = mfma_bf16(al, bh, dacl[i]);
            }
          }
        }
      }
    }
    if (write_dx) {
      float *dst = dx + (int64_t)r0 * V;
      for (int e = tid; e < RB * V / 4; e += NW * 64)
        *reinterpret_cast<float4 *>(dst + e * 4) = *reinterpret_cast<const float4 *>(dxs + e * 4);
    }
  }
#pragma unroll
  for (int i = 0; i < KMAX; ++i) {
    const int j = (wave & 3) + 4 * i;
    const int k = j >> 2, p2 = (j >> 1) & 1, q2 = j & 1;
    if (k < K) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int v = p2 * 32 + (e & 3) + 8 * (e >> 2) + 4 * hi;
        const int w = q2 * 32 + lo;
        if (v < V && w < V) {
          // (deterministic: one slot per row half -- waves w, w + 4 hold the same
          // entries -- added in order by launch_dA_reduce)
          if (dA_part)
            dA_part[((int64_t)blockIdx.x * 2 + (wave >> 2)) * K * V * V + (k * V + v) * V + w] =
                dacc[i][e] + dacl[i][e];
          else
            atomicAdd(dA + (k * V + v) * V + w, dacc[i][e] + dacl[i][e]);
        }
      }
    }
  }
}

template <int V, int KT, bool BF>
static bool launch_bwd6(const SpatialBwd &b, int64_t rows, bool dry, hipStream_t s) {
  constexpr int RB = 64;
  constexpr int PL = (RB * V + 255) / 256 * 256;
  const size_t lds =
      sizeof(float) * ((size_t)(2 * (b.K + 1) + 2) * PL) + 3 * (size_t)V * (RB + 8) * 2;
  if (b.K != KT || lds > 160 * 1024 - 1024 || ((int64_t)b.C * b.T) % RB != 0 ||
      rows >= (int64_t)1 << 31)
    return false;
  if (dry) return true;
  const dim3 grid((unsigned)std::min<int64_t>(rows / RB, 256));
  float *part = b.dA_part && 2 * (int64_t)grid.x <= b.part_cap ? b.dA_part : nullptr;
  if (part && b.nparts) *b.nparts = 2 * (int64_t)grid.x;
  hipLaunchKernelGGL((k_spatial_bwd6<V, KT, BF>), grid, dim3(512), lds, s, b.in, b.x, b.bn.mean,
                     b.bn.invstd, b.bn.g, b.bn.b, b.A, b.dx, b.dA, b.sd, b.sdn, b.C, b.T, b.K, rows,
                     b.write_dx, b.relu, b.prev, part);
  return true;
}

// k_gather_mfma: G_k = f(BN1(x)) A_k^T on the fp32 matrix cores (joint counts
// 25 and 50 with 3 partitions, where k_gather4's one-row-per-thread VALU
// contraction is the slow part). Persistent, x row blocks double-buffered by
// LDS-DMA; block = RB = 128 / NT rows = 4 MFMA tiles (32 rows x one 32-joint
// column tile), one per wave. A-operand: f(BN1(x))[row][w] computed once per
// block from the staged rows (per-lane row constants); B-operand: the wave's
// column tile of A_k^T (B[w][v] = A_k[v][w]) resident in VGPRs. The K output
// tiles leave through LDS as float4 stores (each partition's block of G is
// contiguous).
template <int V, int KMAX>
__global__ __launch_bounds__(256, 2) void k_gather_mfma(
    const float *__restrict__ x, const float *__restrict__ mean, const float *__restrict__ invstd,
    const float *__restrict__ g, const float *__restrict__ b, const float *__restrict__ A,
    float *G, int C, int T, int K, int64_t rows, int relu) {
  constexpr int NT = (V + 31) / 32;
  constexpr int RB = 128 / NT;
  constexpr int NRT = RB / 32;
  constexpr int VH = (V + 1) / 2;
  constexpr int PL = (RB * V + 255) / 256 * 256;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *obuf = smem + 2 * PL;  // [K][PL]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, lo = lane & 31;
  const int CT = C * T;
  const int nblocks = (int)(rows / RB);
  const int rt = wave % NRT, ct = wave / NRT;
  float Bm[KMAX][VH];
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
#pragma unroll
    for (int s2 = 0; s2 < VH; ++s2) {
      const int w = 2 * s2 + hi, v = 32 * ct + lo;
      Bm[k][s2] = (k < K && v < V && w < V) ? A[(k * V + v) * V + w] : 0.f;
    }
  auto stage = [&](int blk, float *buf) {
    constexpr int ND = PL / 256;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(x + (int64_t)blk * RB * V, (int64_t)RB * V);
    for (int i = wave; i < ND; i += 4)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, buf + i * 256, 16,
                                               (unsigned)(i * 256 + lane * 4) * 4u, 0, 0, 0);
  };
  int blk = blockIdx.x;
  if (blk < nblocks) stage(blk, smem);
  for (int it = 0; blk < nblocks; ++it, blk += gridDim.x) {
    const float *xs = smem + (it & 1) * PL;
    __syncthreads();  // block staged; previous block's stores done with obuf
    if (blk + (int)gridDim.x < nblocks) stage(blk + gridDim.x, smem + ((it + 1) & 1) * PL);
    const int r0 = blk * RB;
    const int n0 = r0 / CT, rem0 = r0 - n0 * CT;
    const int row = rt * 32 + lo;
    const int ci = (rem0 + row) / T;
    const BnAff bn = bn_aff(mean, invstd, g, b, ci);
    float fv[VH];
#pragma unroll
    for (int s2 = 0; s2 < VH; ++s2) {
      const int w = 2 * s2 + hi;
      const float t = w < V ? bn.pre(xs[row * V + w]) : 0.f;
      fv[s2] = w < V ? (relu ? relu_max(t) : t) : 0.f;
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < K) {
        floatx16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < VH; ++s2) acc = mfma32(fv[s2], Bm[k][s2], acc);
        float *ok = obuf + k * PL;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int r = rt * 32 + (i & 3) + 8 * (i >> 2) + 4 * hi;
          const int v = 32 * ct + lo;
          if (v < V) ok[r * V + v] = acc[i];
        }
      }
    }
    __syncthreads();  // output tiles complete
    for (int k = 0; k < K; ++k) {
      float *dst = G + ((int64_t)(n0 * K + k) * CT + rem0) * V;
      const float *src = obuf + k * PL;
      for (int e = tid; e < RB * V / 4; e += 256)
        *reinterpret_cast<float4 *>(dst + e * 4) = *reinterpret_cast<const float4 *>(src + e * 4);
    }
  }
}

template <int V, int KT>
static bool launch_gather_mfma_k(const SpatialFwd &f, int64_t rows, hipStream_t s) {
  constexpr int NT = (V + 31) / 32;
  constexpr int RB = 128 / NT;
  constexpr int PL = (RB * V + 255) / 256 * 256;
  if (f.K != KT || ((int64_t)f.C * f.T) % RB != 0 || (RB * V) % 4 != 0 ||
      rows >= (int64_t)1 << 31)
    return false;
  const size_t lds = sizeof(float) * (size_t)(2 + f.K) * PL;
  const int per_cu = std::max(1, std::min(2, (int)((160 * 1024) / (lds + 512))));
  const dim3 grid((unsigned)std::min<int64_t>(rows / RB, 256 * per_cu));
  hipLaunchKernelGGL((k_gather_mfma<V, KT>), grid, dim3(256), lds, s, f.x, f.bn.mean, f.bn.invstd,
                     f.bn.g, f.bn.b, f.A, f.G, f.C, f.T, f.K, rows, f.relu);
  return true;
}
template <int V>
static bool launch_gather_mfma(const SpatialFwd &f, int64_t rows, hipStream_t s) {
  return launch_gather_mfma_k<V, 2>(f, rows, s) || launch_gather_mfma_k<V, 3>(f, rows, s);
}

static int bwd3_rows(int V, int K) {
  // rows per block: 256 when the per-row LDS footprint is small, else 64
  const int VP = (V + 3) & ~3;
  return (K * V + VP) * 4 * 256 <= 48 * 1024 ? 256 : 64;
}

static bool joint_fast(int V) { return V == 18 || V == 25 || V == 50; }

bool gather_prev_supported(int C, int T, int V) {
  return joint_fast(V) && ((int64_t)C * T) % 256 == 0 &&
         sizeof(float) * ((size_t)2 * 256 * V + (size_t)V * ((V + 3) & ~3)) <= 160 * 1024;
}

hipError_t launch_gather_fwd(const SpatialFwd &f, hipStream_t s) {
  const int C = f.C, T = f.T, V = f.V, K = f.K;
  const bool pv = f.prev.bn.mean != nullptr;
  const bool al16 = ((uintptr_t)f.x & 15) == 0 && ((uintptr_t)f.G & 15) == 0;
  const int64_t rows = (int64_t)f.N * C * T;
  if (pv && (K != 1 || !gather_prev_supported(C, T, V) || !al16))
    return hipErrorInvalidValue;  // (x from U: k_gather4 only; checked by the caller first)
  // partitioned graphs: contraction on MFMA
  if (!pv && !f.amax && K > 1 && (V == 25 || V == 50) && al16 &&
      (V == 25 ? launch_gather_mfma<25>(f, rows, s) : launch_gather_mfma<50>(f, rows, s)))
    return hipGetLastError();
  const size_t lds4 = sizeof(float) * ((size_t)2 * 256 * V + (size_t)K * V * ((V + 3) & ~3));
  if (joint_fast(V) && ((int64_t)C * T) % 256 == 0 && al16 && lds4 <= 160 * 1024) {
    dispatch_v(V, [&](auto v) {
      hipLaunchKernelGGL(k_gather4<decltype(v)::value>, dim3((unsigned)(rows / 256)), dim3(256),
                         lds4, s, f.x, f.bn.mean, f.bn.invstd, f.bn.g, f.bn.b, f.A, f.G, C, T, K,
                         rows, f.relu, f.amax, f.prev);
    });
    return hipGetLastError();
  }
  if (joint_fast(V)) {
    const size_t lds3 = sizeof(float) * (size_t)K * V * ((V + 3) & ~3);
    dispatch_v(V, [&](auto v) {
      hipLaunchKernelGGL(k_gather3<decltype(v)::value>, dim3((unsigned)((rows + 255) / 256)),
                         dim3(256), lds3, s, f.x, f.bn.mean, f.bn.invstd, f.bn.g, f.bn.b, f.A, f.G,
                         C, T, K, rows, f.relu, f.amax);
    });
    return hipGetLastError();
  }
  const size_t lds = sizeof(float) * ((size_t)K * V * V + kGatherTC * V);
  hipLaunchKernelGGL(k_gather_fwd, dim3((T + kGatherTC - 1) / kGatherTC, f.N), dim3(256), lds, s,
                     f.x, f.bn.mean, f.bn.invstd, f.bn.g, f.bn.b, f.A, f.G, C, T, V, K, f.relu,
                     f.amax);
  return hipGetLastError();
}

// out[c][v] += sum_t X[n][c][t][v]   (fp64), one block per (c, n)
__global__ __launch_bounds__(256) void k_sum_nt(const float *X, int C, int T, int V,
                                                double *out) {
  __shared__ double part[256];
  const int c = blockIdx.x, n = blockIdx.y;
  const float *src = X + ((int64_t)n * C + c) * T * V;
  const int tpb = 256 / V;  // frame lanes per joint
  const int tid = threadIdx.x;
  double s = 0.0;
  if (tid < tpb * V) {
    const int v = tid % V, tt = tid / V;
    for (int t = tt; t < T; t += tpb) s += src[t * V + v];
  }
  part[tid] = s;
  __syncthreads();
  if (tid < V) {
    double acc = 0.0;
    for (int tt = 0; tt < tpb; ++tt) acc += part[tt * V + tid];
    atomicAdd(out + c * V + tid, acc);
  }
}

// k_sum_nt with float4 loads: 4*A consecutive floats per pass, A = the
// largest multiple of the float4 period of V (V / gcd(4, V)) <= 256, so each
// thread's 4 lanes keep fixed joints across passes; the per-thread fp64
// partials are then folded per joint through LDS. A row (n, c) that does not
// start on a 16-byte boundary (T * V odd or 2 mod 4) is read from the aligned
// address below its start: its elements sit `shift` floats into the float4
// stream, lanes outside [0, T*V) are masked, and the fold maps stream position
// q to joint (q - shift) mod V.
__global__ __launch_bounds__(256) void k_sum_nt4(const float *X, int C, int T, int V,
                                                 double *out) {
  __shared__ double part[1024];
  const int c = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const int L = T * V;
  const int per = V / (V % 4 == 0 ? 4 : (V % 2 == 0 ? 2 : 1));  // float4 period
  const int A = 256 / per * per;                                 // active threads
  const int64_t start = ((int64_t)n * C + c) * L;
  const int shift = (int)(start & 3);
  const float4 *src = reinterpret_cast<const float4 *>(X + (start - shift));
  const int nf = (L + shift + 3) / 4;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (tid < A) {
    for (int f = tid; f < nf; f += A) {
      const float4 q = src[f];
      const int p0 = 4 * f - shift;  // row position of lane 0
      if (p0 >= 0 && p0 + 3 < L) {
        a0 += q.x;
        a1 += q.y;
        a2 += q.z;
        a3 += q.w;
      } else {
        if (p0 >= 0 && p0 < L) a0 += q.x;
        if (p0 + 1 >= 0 && p0 + 1 < L) a1 += q.y;
        if (p0 + 2 >= 0 && p0 + 2 < L) a2 += q.z;
        if (p0 + 3 >= 0 && p0 + 3 < L) a3 += q.w;
      }
    }
  }
  part[4 * tid] = a0;
  part[4 * tid + 1] = a1;
  part[4 * tid + 2] = a2;
  part[4 * tid + 3] = a3;
  __syncthreads();
  if (tid < V) {
    double acc = 0.0;
    // stream position q holds joint (q - shift) mod V; 4*A is a multiple of V
    for (int q = (tid + shift) % V; q < 4 * A; q += V) acc += part[q];
    atomicAdd(out + c * V + tid, acc);
  }
}

hipError_t launch_sum_nt(const float *X, int N, int C, int T, int V, double *out, hipStream_t s) {
  // (rows of any alignment: the float4 kernel reads from the 16-byte boundary
  // below a row's start; X 16-byte aligned and a whole number of float4 in
  // total, so no read passes the tensor's end)
  if (((uintptr_t)X & 15) == 0 && ((int64_t)N * C * T * V) % 4 == 0 && V <= 256) {
    hipLaunchKernelGGL(k_sum_nt4, dim3(C, N), dim3(256), 0, s, X, C, T, V, out);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_sum_nt, dim3(C, N), dim3(256), 0, s, X, C, T, V, out);
  return hipGetLastError();
}

// dbW[k*R+co] = sum_v SdZ[co][v] * rowsum(A_k)[v]
// dA[k][v][w]  = sum_co bW[k*R+co] * SdZ[co][v]      (bias part of dA; all w)
// One block per partition k; V <= 90 (K*V*V <= 8192, checked by the C-ABI).
__global__ __launch_bounds__(256) void k_spatial_small(const double *SdZ, const float *A,
                                                       const float *bW, int K, int R, int V,
                                                       float *dbW, float *dA) {
  __shared__ double rs[128], part[256];
  const int k = blockIdx.x, tid = threadIdx.x;
  for (int v = tid; v < V; v += 256) {
    double ra = 0.0;
    for (int w = 0; w < V; ++w) ra += A[((int64_t)k * V + v) * V + w];
    rs[v] = ra;
  }
  __syncthreads();
  for (int co = tid; co < R; co += 256) {
    double acc = 0.0;
    for (int v = 0; v < V; ++v) acc += SdZ[co * V + v] * rs[v];
    dbW[k * R + co] = (float)acc;
  }
  // bias part of dA: thread (v, j) sums co = j, j + P, ... (P = 256 / V parts)
  const int P = 256 / V;
  const int v = tid % V, j = tid / V;
  double acc = 0.0;
  if (j < P)
    for (int co = j; co < R; co += P) acc += (double)bW[k * R + co] * SdZ[co * V + v];
  part[tid] = acc;
  __syncthreads();
  if (tid < V) {
    double t = 0.0;
    for (int jj = 0; jj < P; ++jj) t += part[jj * V + tid];
    rs[tid] = t;  // rowsums no longer needed
  }
  __syncthreads();
  for (int i = tid; i < V * V; i += 256) dA[(int64_t)k * V * V + i] = (float)rs[i / V];
}

hipError_t launch_spatial_small(const double *SdZ, const float *A, const float *bW, int K, int R,
                                int V, float *dbW, float *dA, hipStream_t s) {
  if (V > 128) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_spatial_small, dim3(K), dim3(256), 0, s, SdZ, A, bW, K, R, V, dbW, dA);
  return hipGetLastError();
}

constexpr int kDxTC = 16;  // frames per spatial-dx block

// Per (n, frame chunk), looping over input channels ci:
//   dxhat[t][w] = sum_k sum_v H[k*C+ci][t][v] * A[k][v][w]     (-> dx buffer)
//   dA[k][v][w] += sum_t H[k*C+ci][t][v] * BN1(x)[ci][t][w]     (LDS accumulator)
//   sd[ci] += sum dxhat, sdn[ci] += sum dxhat * xnorm          (BN1 backward)
__global__ __launch_bounds__(256) void k_spatial_dx(const float *H, const float *x,
                                                    const float *mean, const float *invstd,
                                                    const float *g, const float *b,
                                                    const float *A, float *dx, float *dA,
                                                    double *sd, double *sdn, int C, int T, int V,
                                                    int K, int write_dx, int relu) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ double red[8];
  const int KVV = K * V * V;
  float *As = smem;             // [K][V][V]
  float *dAs = As + KVV;        // [K][V][V] block-local dA
  float *xb = dAs + KVV;        // [TC][V] BN1 output
  float *Hs = xb + kDxTC * V;   // [K][TC][V]
  const int n = blockIdx.y, t0 = blockIdx.x * kDxTC;
  int tc = T - t0;
  if (tc > kDxTC) tc = kDxTC;
  const int tid = threadIdx.x;
  for (int i = tid; i < KVV; i += 256) {
    As[i] = A[i];
    dAs[i] = 0.f;
  }
  const int L = T * V;
  for (int ci = 0; ci < C; ++ci) {
    __syncthreads();
    const int64_t xo = ((int64_t)n * C + ci) * L + (int64_t)t0 * V;
    const BnAff bn = bn_aff(mean, invstd, g, b, ci);
    for (int i = tid; i < tc * V; i += 256) {
      const float t = bn.pre(x[xo + i]);
      xb[i] = relu ? relu_max(t) : t;
    }
    for (int i = tid; i < K * tc * V; i += 256) {
      const int k = i / (tc * V), rem = i - k * tc * V;
      Hs[k * kDxTC * V + rem] = H[(((int64_t)n * K + k) * C + ci) * L + (int64_t)t0 * V + rem];
    }
    __syncthreads();
    // dxhat and BN1 partial sums
    double s = 0.0, sn = 0.0;
    for (int o = tid; o < tc * V; o += 256) {
      const int t = o / V, w = o - t * V;
      float acc = 0.f;
      for (int k = 0; k < K; ++k) {
        const float *hr = Hs + (k * kDxTC + t) * V;
        const float *ac = As + k * V * V + w;
        for (int v = 0; v < V; ++v) acc = fmaf(hr[v], ac[v * V], acc);
      }
      const float xn = bn.hat(x[xo + o]);
      if (relu && bn.pre(x[xo + o]) <= 0.f) acc = 0.f;  // ReLU'(BN1(x))
      if (write_dx) dx[xo + o] = acc;
      s += acc;
      sn += (double)acc * xn;
    }
    // dA partials: each thread owns entries e = tid + 256*j
    for (int e = tid; e < KVV; e += 256) {
      const int k = e / (V * V), rem = e - k * V * V;
      const int v = rem / V, w = rem - v * V;
      float acc = dAs[e];
      for (int t = 0; t < tc; ++t) acc = fmaf(Hs[(k * kDxTC + t) * V + v], xb[t * V + w], acc);
      dAs[e] = acc;
    }
    block_sum2_atomic<256>(s, sn, sd + ci, sdn + ci, red);
  }
  for (int e = tid; e < KVV; e += 256) atomicAdd(dA + e, dAs[e]);
}

// the six k_spatial_bwd5 forms of a joint count: rows per block, partitions K
// (1 uniform, 2 distance, 3 spatial labelling)
template <int V>
static bool launch_bwd5_v(const SpatialBwd &b, int64_t rows, bool dry, hipStream_t s) {
  return launch_bwd5<V, 128, 1>(b, rows, dry, s) || launch_bwd5<V, 64, 1>(b, rows, dry, s) ||
         launch_bwd5<V, 128, 2>(b, rows, dry, s) || launch_bwd5<V, 64, 2>(b, rows, dry, s) ||
         launch_bwd5<V, 128, 3>(b, rows, dry, s) || launch_bwd5<V, 64, 3>(b, rows, dry, s);
}
template <bool BF>
static bool launch_bwd6_k(const SpatialBwd &b, int64_t rows, bool dry, hipStream_t s) {
  return launch_bwd6<50, 1, BF>(b, rows, dry, s) || launch_bwd6<50, 2, BF>(b, rows, dry, s) ||
         launch_bwd6<50, 3, BF>(b, rows, dry, s);
}

// the bwd5 / bwd6 launch; dry: only whether one of them takes this shape, given
// 16-byte aligned tensors (no pointer of b is read)
static bool launch_bwd56(const SpatialBwd &b, bool dry, hipStream_t s) {
  const int V = b.V, K = b.K;
  const int64_t rows = (int64_t)b.N * b.C * b.T;
  const bool aligned = (rows * V) % 4 == 0 &&
                       (dry || (((uintptr_t)b.x & 15) == 0 && ((uintptr_t)b.in & 15) == 0 &&
                                ((uintptr_t)b.dx & 15) == 0));
  if (!aligned || K > 3) return false;
  // (V = 50: K * 25 * 2 > 48 for every K, so it goes to bwd6)
  if ((V == 18 || V == 25) && K * ((V + 1) / 2) * ((V + 31) / 32) <= 48)
    return V == 18 ? launch_bwd5_v<18>(b, rows, dry, s) : launch_bwd5_v<25>(b, rows, dry, s);
  // two-person graph (bf16 blocks: the two-plane k_spatial_bwd6, fp32 paths: its exact-split form)
  if (V == 50)
    return b.bf16ops ? launch_bwd6_k<true>(b, rows, dry, s) : launch_bwd6_k<false>(b, rows, dry, s);
  return false;
}

bool spatial_dx_prev_supported(int N, int C, int T, int V, int K) {
  SpatialBwd b;
  b.N = N, b.C = C, b.T = T, b.V = V, b.K = K;
  return launch_bwd56(b, true, nullptr);
}

hipError_t launch_spatial_dx(const SpatialBwd &b, hipStream_t s) {
  const int N = b.N, C = b.C, T = b.T, V = b.V, K = b.K;
  if (b.nparts) *b.nparts = 0;
  if (launch_bwd56(b, false, s)) return hipGetLastError();
  if (b.prev.bn.mean) return hipErrorInvalidValue;  // (callers check spatial_dx_prev_supported)
  if (joint_fast(V) && K <= 3) {
    const int VP = (V + 3) & ~3;
    const int RB = bwd3_rows(V, K);
    const int64_t rows = (int64_t)N * C * T;
    const int DW3 = (V + 31) / 32 * 32;
    const size_t lds3 = sizeof(float) * ((size_t)K * V * VP + (size_t)K * RB * V + (size_t)RB * VP +
                                         (size_t)(RB / 64) * K * DW3 * DW3);
    const dim3 grid3((unsigned)((rows + RB - 1) / RB));
    // (per-workgroup dA partials where the caller's buffer holds them all)
    float *part = b.dA_part && (int64_t)grid3.x <= b.part_cap ? b.dA_part : nullptr;
    if (part && b.nparts) *b.nparts = grid3.x;
    dispatch_v(V, [&](auto v) {
      hipLaunchKernelGGL(k_spatial_bwd3<decltype(v)::value>, grid3, dim3(RB), lds3, s, b.in, b.x,
                         b.bn.mean, b.bn.invstd, b.bn.g, b.bn.b, b.A, b.dx, b.dA, b.sd, b.sdn, C, T,
                         K, rows, b.write_dx, b.relu, part);
    });
    return hipGetLastError();
  }
  if (K * V * V > 8192) return hipErrorInvalidValue;
  const size_t lds = sizeof(float) * (2 * (size_t)K * V * V + kDxTC * V + (size_t)K * kDxTC * V);
  hipLaunchKernelGGL(k_spatial_dx, dim3((T + kDxTC - 1) / kDxTC, N), dim3(256), lds, s, b.in, b.x,
                     b.bn.mean, b.bn.invstd, b.bn.g, b.bn.b, b.A, b.dx, b.dA, b.sd, b.sdn, C, T, V,
                     K, b.write_dx, b.relu);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Deterministic dA (the spatial backward's per-workgroup partials, dA_part):
// pass 1 sums the partials of chunk y in a fixed order (four interleaved fp64
// chains per entry, combined in order) into lvl[y][e]; pass 2 adds
// sum_y lvl[y][e] (in y order, fp64) to dA[e]. Replaces the fp32 atomics whose
// arrival order made dA differ from run to run at the 1e-3 level on this
// heavily cancelling gradient.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dA_reduce1(const float *__restrict__ part, int64_t nparts,
                                                    int n, int64_t chunk, double *lvl) {
  __shared__ double sm[4][64];
  const int t = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + t;
  const int64_t p0 = (int64_t)blockIdx.y * chunk, p1 = min(nparts, p0 + chunk);
  double s = 0.0;
  if (e < n) {
    int64_t q = p0 + g;
    for (; q + 12 < p1; q += 16) {  // (four loads in flight)
      const float a0 = part[q * n + e], a1 = part[(q + 4) * n + e];
      const float a2 = part[(q + 8) * n + e], a3 = part[(q + 12) * n + e];
      s += a0;
      s += a1;
      s += a2;
      s += a3;
    }
    for (; q < p1; q += 4) s += part[q * n + e];
  }
  sm[g][t] = s;
  __syncthreads();
  if (g == 0 && e < n) lvl[(int64_t)blockIdx.y * n + e] = ((sm[0][t] + sm[1][t]) + sm[2][t]) + sm[3][t];
}

__global__ __launch_bounds__(256) void k_dA_reduce2(const double *__restrict__ lvl, int ny, int n,
                                                    float *dA) {
  // (four groups of 64 lanes, each over every fourth level with all its loads
  // in flight, combined in group order)
  __shared__ double sm[4][64];
  const int t = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + t;
  double s = 0.0;
  if (e < n) {
#pragma unroll
    for (int i = 0; i < kDaLvl / 4; ++i) {
      const int y = g + 4 * i;
      if (y < ny) s += lvl[(int64_t)y * n + e];
    }
  }
  sm[g][t] = s;
  __syncthreads();
  if (g == 0 && e < n)
    dA[e] = (float)((double)dA[e] + (((sm[0][t] + sm[1][t]) + sm[2][t]) + sm[3][t]));
}

hipError_t launch_dA_reduce(const float *part, int64_t nparts, int n, double *lvl, float *dA,
                            hipStream_t s) {
  if (nparts <= 0) return hipSuccess;
  if (!part || !lvl || !dA || n <= 0) return hipErrorInvalidValue;
  const int ny = (int)std::min<int64_t>(kDaLvl, nparts);
  const int64_t chunk = (nparts + ny - 1) / ny;
  const int nb = (n + 63) / 64;
  hipLaunchKernelGGL(k_dA_reduce1, dim3(nb, ny), dim3(256), 0, s, part, nparts, n, chunk, lvl);
  hipLaunchKernelGGL(k_dA_reduce2, dim3(nb), dim3(256), 0, s, lvl, ny, n, dA);
  return hipGetLastError();
}

}  // namespace stgcn
