// Training-step ops around the block stack: the
// classification head (global average pool over (T, V) + Linear + cross
// entropy, lightning_model.py:105-107, :202) in its training and evaluation
// forms, and the dropout step token, gfx950 only. Launch-bound, not FLOP-bound:
// the head is 5 small kernels instead of torch's ~12. (The optimizer step of the
// same layer is optim.hip.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/stgcn_hip.h"
#include "device_common.h"
#include "host_common.h"

namespace {

using stgcn::check_aligned;
using stgcn::fail;
using stgcn::NamedPtr;
using stgcn::wave_sumf;

// The dropout step token (stgcn_seed_next), in k_adam_tick's style (optim.hip)
__global__ void k_seed_next(uint64_t *counter, uint64_t *token) {
  *counter += 1;
  *token = *counter;
}

// ---------------------------------------------------------------------------
// Head. y: (N, C, L) block output (L = T*V), W: (classes, C), b: (classes),
// labels: int64 (N). pooled (N, C), logits (N, classes), lossv (N) per-clip
// losses, loss (1) = mean.
// ---------------------------------------------------------------------------
// pooled[n][c] = mean_l y[n][c][l]: one wave per (n, c) row, 4 rows per block
__global__ __launch_bounds__(256) void k_head_pool(const float *y, float *pooled, int64_t rows,
                                                   int L) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float *src = y + row * L;
  float s = 0.f;
  for (int l = lane; l < L; l += 64) s += src[l];
  s = wave_sumf(s);
  if (lane == 0) pooled[row] = s / (float)L;
}

// ABI 9: the same mean over y = ReLU(BN2(U)) formed on load from the last
// block's pre-BN2 tensor U (its y is never written): the element arithmetic of
// k_bn_relu_fwd (kernels_bn.hip bn_relu_fwd_body), the summation order of
// k_head_pool, so pooled is bit-identical to pooling the written y
__global__ __launch_bounds__(256) void k_head_pool_u(const float *U, const float *mean,
                                                     const float *invstd, const float *g,
                                                     const float *b, float *pooled, int64_t rows,
                                                     int C, int L) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int c = (int)(row % C);
  const stgcn::BnAff bn = stgcn::bn_aff(mean, invstd, g, b, c);
  const float *src = U + row * L;
  float s = 0.f;
  for (int l = lane; l < L; l += 64) s += stgcn::bn_relu(bn.pre(src[l]));
  s = wave_sumf(s);
  if (lane == 0) pooled[row] = s / (float)L;
}

// The logits row of clip blockIdx.x and its log-sum-exp (k_head_row). sh:
// [C] pooled row, [classes] logits (kept for the caller), [8] reduction. Every
// thread returns the row maximum mx and the sum tot of exp(logit - mx).
__device__ __forceinline__ void head_fc_lse(const float *pooled, const float *W,
                                            const float *bias, float *logits, int C,
                                            int classes, float *sh, float &mx, float &tot) {
  float *pr = sh, *lg = sh + C, *red = lg + classes;
  const int n = blockIdx.x, tid = threadIdx.x;
  for (int c = tid; c < C; c += 256) pr[c] = pooled[(int64_t)n * C + c];
  __syncthreads();
  for (int j = tid; j < classes; j += 256) {
    const float *w = W + (int64_t)j * C;
    float a = 0.f;
    for (int c = 0; c < C; ++c) a = fmaf(pr[c], w[c], a);
    a += bias[j];
    lg[j] = a;
    logits[(int64_t)n * classes + j] = a;
  }
  __syncthreads();
  mx = -INFINITY;
  for (int j = tid; j < classes; j += 256) mx = fmaxf(mx, lg[j]);
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float se = 0.f;
  for (int j = tid; j < classes; j += 256) se += expf(lg[j] - mx);
  se = wave_sumf(se);
  if ((tid & 63) == 0) red[4 + (tid >> 6)] = se;
  __syncthreads();
  tot = (red[4] + red[5]) + (red[6] + red[7]);
}

// (value, index) maximum with ties going to the lowest index
__device__ __forceinline__ void argmax_take(float &bv, int &bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

// One block per clip, every form of the head: logits = pooled W^T + b and the
// per-clip loss with F.cross_entropy's weight= and label_smoothing= (stgcn_hip.h,
// stgcn_head_eval_loss). With z the logits row, lse its log-sum-exp and nll =
// lse - z[y]:
//   lossv = (1 - eps) * w[y] * nll + (eps / J) * sum_j w[j] * (lse - z[j])
// cw null: w = 1. om = 1 - eps and epsJ = eps / J are formed on the host in
// double. With eps = 0 the sum is not formed and om = 1, and without weights
// w[y] = 1, so lossv is nll itself (a product by 1 is exact): the training head,
// the evaluation head and the evaluation head with default options give the same
// bits. The sum over j is per thread in index order, then the wave, then the four
// waves in a fixed tree.
// TRAIN (stgcn_head_fwd: cw null, om 1, epsJ 0): a label outside [0, classes)
// gives NaN and no smoothing sum is compiled; otherwise such a label is cross
// entropy's ignore_index: loss 0, the label indexes nothing.
// PRED (the evaluation head, validation_step / test_step,
// lightning_model.py:213-253): pred = the lowest index attaining the maximum
// logit, reduced as (value, index) pairs over the lanes of each wave, then over
// the four waves.
template <bool PRED, bool TRAIN>
__global__ __launch_bounds__(256) void k_head_row(const float *pooled, const float *W,
                                                  const float *bias, const float *cw,
                                                  const int64_t *labels, float *logits,
                                                  float *lossv, int32_t *pred, int C,
                                                  int classes, float om, float epsJ) {
  extern __shared__ float sh[];  // [C] pooled row, [classes] logits, [8] reduction
  float mx, tot;
  head_fc_lse(pooled, W, bias, logits, C, classes, sh, mx, tot);
  if constexpr (PRED || !TRAIN)
    __syncthreads();  // (every thread has read the reduction words: reused below)
  const float *lg = sh + C;
  float *av = sh + C + classes;  // [4] value, [4] index per wave
  const int n = blockIdx.x, tid = threadIdx.x;
  const float lse = logf(tot) + mx;
  const bool smooth = !TRAIN && epsJ > 0.f;  // (uniform over the launch)
  float sm = 0.f;
  if (smooth) {
    for (int j = tid; j < classes; j += 256) sm += (cw ? cw[j] : 1.f) * (lse - lg[j]);
    sm = wave_sumf(sm);
    if ((tid & 63) == 0) av[tid >> 6] = sm;
    __syncthreads();
    sm = (av[0] + av[1]) + (av[2] + av[3]);
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t y = labels[n];
    float l = TRAIN ? NAN : 0.f;
    if (y >= 0 && y < classes) {
      l = om * (cw ? cw[y] : 1.f) * (lse - lg[y]);
      if (smooth) l = fmaf(epsJ, sm, l);
    }
    lossv[n] = l;
  }
  if constexpr (PRED) {
    int *ai = reinterpret_cast<int *>(av + 4);
    float bv = -INFINITY;
    int bi = INT32_MAX;
    for (int j = tid; j < classes; j += 256) argmax_take(bv, bi, lg[j], j);
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      argmax_take(bv, bi, ov, oi);
    }
    if ((tid & 63) == 0) {
      av[tid >> 6] = bv;
      ai[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; ++w) argmax_take(bv, bi, av[w], ai[w]);
      pred[n] = bi < classes ? bi : 0;  // (no logit compares: every one NaN)
    }
  }
}

// The batch pass of the evaluation head, ONE workgroup: loss = the sum of lossv
// over the clips with a valid label over D (k_head_loss_mean's fixed-order fp64
// sum, so the same bits when every label is valid and cw is null; 0 when D == 0)
// and, metrics non-null, the epoch's words and confusion matrix. D = the sum of
// w[label] over the valid clips in fp64 in clip order, their count when cw is
// null (the same double as summing ones), written to denom[0] as a float when
// denom is non-null. Wave w takes clips w, w + 4, ..: its lanes count the logits
// that rank before the label's (top-k hit: fewer than topk of them). Counts are
// integers, the sums one fp64 add per word from thread 0, the matrix integer
// atomics: the result does not depend on order.
__global__ __launch_bounds__(256) void k_head_batch(const float *logits, const int64_t *labels,
                                                    const float *lossv, const int32_t *pred,
                                                    const float *cw, float *loss, float *denom,
                                                    void *metrics, int N, int classes,
                                                    int topk) {
  __shared__ int cnt[4][4];  // per wave: valid, invalid, correct, top-k hits
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long *conf =
      metrics ? reinterpret_cast<unsigned long long *>(metrics) + 8 : nullptr;
  int valid = 0, invalid = 0, correct = 0, hits = 0;
  for (int n = wave; n < N; n += 4) {
    const int64_t y = labels[n];  // (wave-uniform)
    if (y < 0 || y >= classes) {
      ++invalid;
      continue;
    }
    ++valid;
    const int p = pred[n];
    correct += p == (int)y ? 1 : 0;
    if (!metrics) continue;
    const float *lg = logits + (int64_t)n * classes;
    const float ly = lg[y];
    int before = 0;
    for (int j = lane; j < classes; j += 64) {
      const float v = lg[j];
      before += (v > ly || (v == ly && j < (int)y)) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    hits += before < topk ? 1 : 0;
    if (lane == 0) atomicAdd(conf + (size_t)y * classes + p, 1ull);
  }
  if (lane == 0) {
    cnt[wave][0] = valid;
    cnt[wave][1] = invalid;
    cnt[wave][2] = correct;
    cnt[wave][3] = hits;
  }
  __syncthreads();
  if (tid != 0) return;
  int64_t tot[4];
  for (int i = 0; i < 4; ++i)
    tot[i] = (int64_t)cnt[0][i] + cnt[1][i] + cnt[2][i] + cnt[3][i];
  double s = 0.0, D = (double)tot[0];
  for (int n = 0; n < N; ++n) {
    const int64_t y = labels[n];
    if (y >= 0 && y < classes) s += lossv[n];
  }
  if (cw) {
    D = 0.0;
    for (int n = 0; n < N; ++n) {
      const int64_t y = labels[n];
      if (y >= 0 && y < classes) D += (double)cw[y];
    }
  }
  const double mean = D > 0.0 ? s / D : 0.0;
  loss[0] = (float)mean;
  if (denom) denom[0] = (float)D;
  if (!metrics) return;
  int64_t *mi = reinterpret_cast<int64_t *>(metrics);
  double *md = reinterpret_cast<double *>(metrics);
  mi[0] += 1;
  mi[1] += tot[0];
  mi[2] += tot[2];
  mi[3] += tot[3];
  mi[4] += tot[1];
  md[5] += s;
  md[6] += mean;
  md[7] += tot[0] > 0 ? (double)tot[2] / (double)tot[0] : 0.0;
}

// loss = mean_n lossv[n] (fixed order: deterministic)
__global__ void k_head_loss_mean(const float *lossv, float *loss, int N) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int n = 0; n < N; ++n) s += lossv[n];
    loss[0] = (float)(s / N);
  }
}

// dlogits[n][j] = (softmax_j - [j == y_n]) * dloss / N; dpooled[n][c] = sum_j dlogits W[j][c]
__global__ __launch_bounds__(256) void k_head_bwd_rows(const float *logits, const float *W,
                                                       const int64_t *labels, const float *dloss,
                                                       float *dlogits, float *dpooled, int N,
                                                       int C, int classes) {
  extern __shared__ float sh[];  // [classes] dlogits, [8]
  float *dl = sh, *red = sh + classes;
  const int n = blockIdx.x, tid = threadIdx.x;
  const float *lg = logits + (int64_t)n * classes;
  float mx = -INFINITY;
  for (int j = tid; j < classes; j += 256) mx = fmaxf(mx, lg[j]);
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float se = 0.f;
  for (int j = tid; j < classes; j += 256) se += expf(lg[j] - mx);
  se = wave_sumf(se);
  if ((tid & 63) == 0) red[4 + (tid >> 6)] = se;
  __syncthreads();
  const float tot = (red[4] + red[5]) + (red[6] + red[7]);
  const float scale = dloss[0] / (float)N;
  const int64_t y = labels[n];
  for (int j = tid; j < classes; j += 256) {
    const float d = (expf(lg[j] - mx) / tot - (j == y ? 1.f : 0.f)) * scale;
    dl[j] = d;
    dlogits[(int64_t)n * classes + j] = d;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float a = 0.f;
    for (int j = 0; j < classes; ++j) a = fmaf(dl[j], W[(int64_t)j * C + c], a);
    dpooled[(int64_t)n * C + c] = a;
  }
}

// dW[j][c] = sum_n dlogits[n][j] pooled[n][c]; db[j] = sum_n dlogits[n][j]
__global__ __launch_bounds__(256) void k_head_wgrad(const float *dlogits, const float *pooled,
                                                    float *dW, float *db, int N, int C,
                                                    int classes) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)classes * (C + 1)) return;
  const int j = (int)(idx / (C + 1)), c = (int)(idx % (C + 1));
  float a = 0.f;
  if (c < C) {
    for (int n = 0; n < N; ++n) a = fmaf(dlogits[(int64_t)n * classes + j], pooled[(int64_t)n * C + c], a);
    dW[(int64_t)j * C + c] = a;
  } else {
    for (int n = 0; n < N; ++n) a += dlogits[(int64_t)n * classes + j];
    db[j] = a;
  }
}

// dy[n][c][l] = dpooled[n][c] / L (the avg-pool backward), float4 stores when L % 4 == 0
__global__ __launch_bounds__(256) void k_head_bcast(const float *dpooled, float *dy, int64_t rows,
                                                    int L) {
  const int64_t row = blockIdx.x;
  if (row >= rows) return;
  const float v = dpooled[row] / (float)L;
  float *dst = dy + row * L;
  for (int l = threadIdx.x; l < L; l += 256) dst[l] = v;
}

// the per-row value k_head_bcast writes at every position (same arithmetic)
__global__ __launch_bounds__(256) void k_head_dync(const float *dpooled, float *dy_nc, int64_t rows,
                                                   int L) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row < rows) dy_nc[row] = dpooled[row] / (float)L;
}

// The source of a head's pool: the last block's output y (N, C, L) as written,
// or (u) its pre-BN2 tensor U with stats2 = [mean2 | invstd2] and the BN2 affine
struct HeadSrc {
  const float *x, *stats2, *g2, *b2;
  bool u;
};

void launch_pool(const HeadSrc &src, float *pooled, int N, int C, int L, hipStream_t s) {
  const int64_t rows = (int64_t)N * C;
  const dim3 grid((unsigned)((rows + 3) / 4));
  const stgcn::BnRef bn = stgcn::bn_ref(src.stats2, C, src.g2, src.b2);
  if (src.u)
    hipLaunchKernelGGL(k_head_pool_u, grid, dim3(256), 0, s, src.x, bn.mean, bn.invstd, bn.g, bn.b,
                       pooled, rows, C, L);
  else
    hipLaunchKernelGGL(k_head_pool, grid, dim3(256), 0, s, src.x, pooled, rows, L);
}

size_t head_row_lds(int C, int classes) { return (size_t)(C + classes + 8) * sizeof(float); }

// stgcn_head_fwd / _fwd_u
int head_fwd(const stgcn_head_desc_t *d, const HeadSrc &src, const float *W, const float *bias,
             const int64_t *labels, float *pooled, float *logits, float *lossv, float *loss,
             void *stream) {
  if (!d || d->N <= 0 || d->C <= 0 || d->L <= 0 || d->classes <= 0)
    return fail(STGCN_E_INVALID, "head: bad descriptor");
  if (!src.x || (src.u && (!src.stats2 || !src.g2 || !src.b2)) || !W || !bias || !labels ||
      !pooled || !logits || !lossv || !loss)
    return fail(STGCN_E_INVALID, "head: null tensor argument");
  if (int rc = check_aligned({NamedPtr{src.x, src.u ? "U" : "y"}, NamedPtr{src.stats2, "stats2"},
                              NamedPtr{src.g2, "g2"}, NamedPtr{src.b2, "b2"}, NP(W), NP(bias),
                              NP(pooled), NP(logits), NP(lossv), NP(loss)},
                             4))
    return rc;
  if (int rc = check_aligned({NP(labels)}, 8)) return rc;
  if (head_row_lds(d->C, d->classes) > 64 * 1024)
    return fail(STGCN_E_UNSUPPORTED, "head: C + classes too large");
  hipStream_t s = (hipStream_t)stream;
  launch_pool(src, pooled, d->N, d->C, d->L, s);
  hipLaunchKernelGGL((k_head_row<false, true>), dim3(d->N), dim3(256),
                     head_row_lds(d->C, d->classes), s, pooled, W, bias, nullptr, labels, logits,
                     lossv, nullptr, d->C, d->classes, 1.f, 0.f);
  hipLaunchKernelGGL(k_head_loss_mean, dim3(1), dim3(64), 0, s, lossv, loss, d->N);
  HIP_TRY(hipGetLastError());
  return STGCN_OK;
}

// (classes of a metrics block: the head's own LDS limit at C = 1)
bool eval_classes_ok(int classes) { return classes > 0 && head_row_lds(1, classes) <= 64 * 1024; }

// The launches of every evaluation head after its checks: the pool, logits,
// losses and predictions, then the batch pass. cw / denom null, om 1, epsJ 0:
// stgcn_head_eval.
int head_eval_launch(int N, int C, int L, int classes, int topk, const HeadSrc &src,
                     const float *W, const float *bias, const float *cw, float om, float epsJ,
                     const int64_t *labels, float *pooled, float *logits, float *lossv,
                     float *denom, float *loss, int32_t *pred, void *metrics, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  launch_pool(src, pooled, N, C, L, s);
  hipLaunchKernelGGL((k_head_row<true, false>), dim3(N), dim3(256), head_row_lds(C, classes), s,
                     pooled, W, bias, cw, labels, logits, lossv, pred, C, classes, om, epsJ);
  hipLaunchKernelGGL(k_head_batch, dim3(1), dim3(256), 0, s, logits, labels, lossv, pred, cw,
                     loss, denom, metrics, N, classes, topk);
  HIP_TRY(hipGetLastError());
  return STGCN_OK;
}

// stgcn_head_eval / _eval_u
int head_eval(const stgcn_eval_desc_t *d, const HeadSrc &src, const float *W, const float *bias,
              const int64_t *labels, float *pooled, float *logits, float *lossv, float *loss,
              int32_t *pred, void *metrics, void *stream) {
  if (!d || d->N <= 0 || d->C <= 0 || d->L <= 0 || d->classes <= 0)
    return fail(STGCN_E_INVALID, "head: bad descriptor");
  if (d->topk < 1 || d->topk > d->classes)
    return fail(STGCN_E_INVALID, "head: topk outside [1, classes]");
  if (!src.x || !W || !bias || !labels || !pooled || !logits || !lossv || !loss || !pred)
    return fail(STGCN_E_INVALID, "head: null tensor argument");
  if (int rc = check_aligned({NamedPtr{src.x, "y / U"}, NP(W), NP(bias), NP(pooled), NP(logits),
                              NP(lossv), NP(loss), NP(pred)},
                             4))
    return rc;
  if (int rc = check_aligned({NP(labels)}, 8)) return rc;
  if (src.u && (!src.stats2 || !src.g2 || !src.b2))
    return fail(STGCN_E_INVALID, "head: null tensor argument");
  if (int rc = check_aligned({NamedPtr{src.stats2, "stats2"}, NamedPtr{src.g2, "g2"},
                              NamedPtr{src.b2, "b2"}},
                             4))
    return rc;
  if (int rc = check_aligned({NP(metrics)}, 8)) return rc;
  if (head_row_lds(d->C, d->classes) > 64 * 1024)
    return fail(STGCN_E_UNSUPPORTED, "head: C + classes too large");
  return head_eval_launch(d->N, d->C, d->L, d->classes, d->topk, src, W, bias, nullptr, 1.f, 0.f,
                          labels, pooled, logits, lossv, nullptr, loss, pred, metrics, stream);
}

// STGCN_FEATURE_HEAD_LOSS ----------------------------------------------------
// (everything stgcn_loss_check refuses but the LDS limit, which the entry points
// apply after their argument checks, as stgcn_head_eval does)
int loss_desc_check(const stgcn_loss_desc_t *d) {
  if (!d) return fail(STGCN_E_INVALID, "loss: null descriptor");
  if (d->N <= 0 || d->C <= 0 || d->L <= 0 || d->classes <= 0)
    return fail(STGCN_E_INVALID, "loss: bad descriptor (N, C, L, classes must be positive)");
  if (d->topk < 1 || d->topk > d->classes)
    return fail(STGCN_E_INVALID, "loss: topk outside [1, classes]");
  if (d->flags & ~STGCN_LOSS_WEIGHT) return fail(STGCN_E_INVALID, "loss: unknown flags");
  if (!std::isfinite(d->label_smoothing) || d->label_smoothing < 0.0 ||
      d->label_smoothing > 1.0)
    return fail(STGCN_E_INVALID, "loss: label_smoothing outside [0, 1]");
  return STGCN_OK;
}
int loss_desc_fits(const stgcn_loss_desc_t *d) {
  if ((size_t)((int64_t)d->C + d->classes + 8) * sizeof(float) > 64 * 1024)
    return fail(STGCN_E_UNSUPPORTED, "loss: C + classes too large");
  return STGCN_OK;
}

// stgcn_head_eval_loss / _eval_loss_u
int head_eval_loss(const stgcn_loss_desc_t *d, const HeadSrc &src, const float *W,
                   const float *bias, const float *class_weight, const int64_t *labels,
                   float *pooled, float *logits, float *lossv, float *denom, float *loss,
                   int32_t *pred, void *metrics, void *stream) {
  if (int rc = loss_desc_check(d)) return rc;
  if (!src.x || !W || !bias || !labels || !pooled || !logits || !lossv || !denom || !loss ||
      !pred)
    return fail(STGCN_E_INVALID, "loss: null tensor argument");
  if ((d->flags & STGCN_LOSS_WEIGHT) && !class_weight)
    return fail(STGCN_E_INVALID, "loss: STGCN_LOSS_WEIGHT without class_weight");
  if (!(d->flags & STGCN_LOSS_WEIGHT) && class_weight)
    return fail(STGCN_E_INVALID, "loss: class_weight without STGCN_LOSS_WEIGHT");
  if (int rc = check_aligned({NamedPtr{src.x, "y / U"}, NP(W), NP(bias), NP(class_weight),
                              NP(pooled), NP(logits), NP(lossv), NP(denom), NP(loss), NP(pred)},
                             4))
    return rc;
  if (int rc = check_aligned({NP(labels), NP(metrics)}, 8)) return rc;
  if (src.u && (!src.stats2 || !src.g2 || !src.b2))
    return fail(STGCN_E_INVALID, "loss: null tensor argument");
  if (int rc = check_aligned({NamedPtr{src.stats2, "stats2"}, NamedPtr{src.g2, "g2"},
                              NamedPtr{src.b2, "b2"}},
                             4))
    return rc;
  if (int rc = loss_desc_fits(d)) return rc;
  const double eps = d->label_smoothing;
  return head_eval_launch(d->N, d->C, d->L, d->classes, d->topk, src, W, bias, class_weight,
                          (float)(1.0 - eps), (float)(eps / d->classes), labels, pooled, logits,
                          lossv, denom, loss, pred, metrics, stream);
}

// stgcn_head_bwd / _bwd_nc: dy the (N, C, L) gradient, or (nc) its per-row value
int head_bwd(const stgcn_head_desc_t *d, const float *pooled, const float *logits, const float *W,
             const int64_t *labels, const float *dloss, float *dlogits, float *dpooled,
             float *dy, bool nc, float *dW, float *dbias, void *stream) {
  if (!d || d->N <= 0 || d->C <= 0 || d->L <= 0 || d->classes <= 0)
    return fail(STGCN_E_INVALID, "head: bad descriptor");
  if (!pooled || !logits || !W || !labels || !dloss || !dlogits || !dpooled || !dy || !dW ||
      !dbias)
    return fail(STGCN_E_INVALID, "head: null tensor argument");
  if (int rc = check_aligned({NP(pooled), NP(logits), NP(W), NP(dloss), NP(dlogits), NP(dpooled),
                              NamedPtr{dy, nc ? "dy_nc" : "dy"}, NP(dW), NP(dbias)},
                             4))
    return rc;
  if (int rc = check_aligned({NP(labels)}, 8)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)d->N * d->C;
  hipLaunchKernelGGL(k_head_bwd_rows, dim3(d->N), dim3(256),
                     (size_t)(d->classes + 8) * sizeof(float), s, logits, W, labels, dloss,
                     dlogits, dpooled, d->N, d->C, d->classes);
  const int64_t nw = (int64_t)d->classes * (d->C + 1);
  hipLaunchKernelGGL(k_head_wgrad, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, dlogits,
                     pooled, dW, dbias, d->N, d->C, d->classes);
  if (nc)
    hipLaunchKernelGGL(k_head_dync, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s,
                       dpooled, dy, rows, d->L);
  else
    hipLaunchKernelGGL(k_head_bcast, dim3((unsigned)rows), dim3(256), 0, s, dpooled, dy, rows,
                       d->L);
  HIP_TRY(hipGetLastError());
  return STGCN_OK;
}

}  // namespace

extern "C" {

int stgcn_seed_next(uint64_t *counter, uint64_t *token, void *stream) {
  if (!counter) return fail(STGCN_E_INVALID, "seed_next: counter is null");
  if (!token) return fail(STGCN_E_INVALID, "seed_next: token is null");
  if (int rc = check_aligned({NP(counter), NP(token)}, 8)) return rc;
  hipLaunchKernelGGL(k_seed_next, dim3(1), dim3(1), 0, (hipStream_t)stream, counter, token);
  HIP_TRY(hipGetLastError());
  return STGCN_OK;
}

int stgcn_features(void) {
  return STGCN_FEATURE_EVAL_CHAIN | STGCN_FEATURE_EVAL_HEAD | STGCN_FEATURE_STEP_STATE |
         STGCN_FEATURE_INPUT_STAGE | STGCN_FEATURE_OPTIMIZERS | STGCN_FEATURE_HEAD_LOSS |
         STGCN_FEATURE_INPUT_MOVE | STGCN_FEATURE_BWD_OVERLAP | STGCN_FEATURE_INPUT_STREAMS;
}

int stgcn_head_fwd(const stgcn_head_desc_t *d, const float *y, const float *W, const float *bias,
                   const int64_t *labels, float *pooled, float *logits, float *lossv, float *loss,
                   void *stream) {
  return head_fwd(d, {y, nullptr, nullptr, nullptr, false}, W, bias, labels, pooled, logits,
                  lossv, loss, stream);
}

int stgcn_head_fwd_u(const stgcn_head_desc_t *d, const float *U, const float *stats2,
                     const float *g2, const float *b2, const float *W, const float *bias,
                     const int64_t *labels, float *pooled, float *logits, float *lossv,
                     float *loss, void *stream) {
  return head_fwd(d, {U, stats2, g2, b2, true}, W, bias, labels, pooled, logits, lossv, loss,
                  stream);
}

size_t stgcn_eval_metrics_bytes(int classes) {
  if (!eval_classes_ok(classes)) return 0;
  return 8 * sizeof(int64_t) + (size_t)classes * classes * sizeof(int64_t);
}

int stgcn_eval_metrics_reset(void *metrics, int classes, void *stream) {
  const size_t nbytes = stgcn_eval_metrics_bytes(classes);
  if (!metrics || !nbytes) return fail(STGCN_E_INVALID, "eval metrics: null block or bad classes");
  if (int rc = check_aligned({NP(metrics)}, 8)) return rc;
  HIP_TRY(hipMemsetAsync(metrics, 0, nbytes, (hipStream_t)stream));
  return STGCN_OK;
}

int stgcn_head_eval(const stgcn_eval_desc_t *d, const float *y, const float *W, const float *bias,
                    const int64_t *labels, float *pooled, float *logits, float *lossv,
                    float *loss, int32_t *pred, void *metrics, void *stream) {
  return head_eval(d, {y, nullptr, nullptr, nullptr, false}, W, bias, labels, pooled, logits,
                   lossv, loss, pred, metrics, stream);
}

int stgcn_head_eval_u(const stgcn_eval_desc_t *d, const float *U, const float *stats2,
                      const float *g2, const float *b2, const float *W, const float *bias,
                      const int64_t *labels, float *pooled, float *logits, float *lossv,
                      float *loss, int32_t *pred, void *metrics, void *stream) {
  return head_eval(d, {U, stats2, g2, b2, true}, W, bias, labels, pooled, logits, lossv, loss,
                   pred, metrics, stream);
}

int stgcn_loss_check(const stgcn_loss_desc_t *d) {
  if (int rc = loss_desc_check(d)) return rc;
  return loss_desc_fits(d);
}

int stgcn_head_eval_loss(const stgcn_loss_desc_t *d, const float *y, const float *W,
                         const float *bias, const float *class_weight, const int64_t *labels,
                         float *pooled, float *logits, float *lossv, float *denom, float *loss,
                         int32_t *pred, void *metrics, void *stream) {
  return head_eval_loss(d, {y, nullptr, nullptr, nullptr, false}, W, bias, class_weight, labels,
                        pooled, logits, lossv, denom, loss, pred, metrics, stream);
}

int stgcn_head_eval_loss_u(const stgcn_loss_desc_t *d, const float *U, const float *stats2,
                           const float *g2, const float *b2, const float *W, const float *bias,
                           const float *class_weight, const int64_t *labels, float *pooled,
                           float *logits, float *lossv, float *denom, float *loss, int32_t *pred,
                           void *metrics, void *stream) {
  return head_eval_loss(d, {U, stats2, g2, b2, true}, W, bias, class_weight, labels, pooled,
                        logits, lossv, denom, loss, pred, metrics, stream);
}

int stgcn_head_bwd(const stgcn_head_desc_t *d, const float *pooled, const float *logits,
                   const float *W, const int64_t *labels, const float *dloss, float *dlogits,
                   float *dpooled, float *dy, float *dW, float *dbias, void *stream) {
  return head_bwd(d, pooled, logits, W, labels, dloss, dlogits, dpooled, dy, false, dW, dbias,
                  stream);
}

int stgcn_head_bwd_nc(const stgcn_head_desc_t *d, const float *pooled, const float *logits,
                      const float *W, const int64_t *labels, const float *dloss, float *dlogits,
                      float *dpooled, float *dy_nc, float *dW, float *dbias, void *stream) {
  return head_bwd(d, pooled, logits, W, labels, dloss, dlogits, dpooled, dy_nc, true, dW, dbias,
                  stream);
}

}  // extern "C"
