// Training-step ops around the block stack: the
// classification head (global average pool over (T, V) + Linear + cross
// entropy, lightning_model.py:105-107, :202) and a multi-tensor Adam step
// (lightning_model.py:196-197, torch.optim.Adam semantics), gfx950 only.
// Both are launch-bound, not FLOP-bound: the head is 5 small kernels instead
// of torch's ~12, Adam is ONE launch over every parameter tensor.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <string>

#include "../../include/stgcn_hip.h"
#include "device_common.h"

namespace stgcn {
void set_last_error(const std::string &msg);  // capi.hip (stgcn_last_error)
}

namespace {

using stgcn::wave_sumf;

int fail(int code, const std::string &m) {
  stgcn::set_last_error(m);
  return code;
}

// The alignment contract of stgcn_hip.h (Conventions) for the head and Adam:
// every kernel below reads and writes one element at a time, so a pointer needs
// its element's own alignment only (4 bytes fp32 / int32, 8 bytes int64 labels,
// the metrics block and the Adam table). Null pointers pass.
struct NamedPtr {
  const void *p;
  const char *name;
};
int check_aligned(std::initializer_list<NamedPtr> ptrs, unsigned align) {
  for (const NamedPtr &q : ptrs)
    if (((uintptr_t)q.p & (align - 1)) != 0)
      return fail(STGCN_E_INVALID,
                  std::string(q.name) + ": must be " + std::to_string(align) + "-byte aligned");
  return STGCN_OK;
}
#define NP(v) NamedPtr{v, #v}

#define HIP_TRY2(expr)                                                                     \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(STGCN_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));        \
  } while (0)

// ---------------------------------------------------------------------------
// Adam. Per element, in fp32, in torch's order (optim/adam.py _multi_tensor_adam /
// _single_tensor_adam, weight_decay folded into the gradient as in torch):
//   g  = grad + wd * p
//   m  = lerp(m, g, 1 - beta1)          (m + w (g - m) for w < 0.5)
//   v  = v * beta2;  v = v + ((1 - beta2) * g) * g
//   p  = p + (-lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))
// with bc1 = 1 - beta1^step, bc2 = 1 - beta2^step computed in double on the
// host and rounded to float like torch's scalar arguments.
// ---------------------------------------------------------------------------
constexpr int kAdamChunk = 2048;  // elements per block (256 threads x 8)

struct AdamScalars {
  float lerp_w, beta2, one_minus_beta2, neg_step_size, bc2_sqrt, eps, wd;
};

// the element loop of every launch form (one function: the same instructions)
// COEF (k_adam_dev2 with a grad_coef): g = grad * coef ahead of the weight decay
template <bool COEF = false>
__device__ __forceinline__ void adam_block(const stgcn_adam_tensor_t *tab,
                                           const int64_t *chunk_start, int ntensors,
                                           const AdamScalars &s, float coef = 1.f) {
#pragma clang fp contract(off)
  // tensor of this block: the last t with chunk_start[t] <= blockIdx.x
  const int64_t b = blockIdx.x;
  int lo = 0, hi = ntensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk_start[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const stgcn_adam_tensor_t t = tab[lo];
  const int64_t base = (b - chunk_start[lo]) * kAdamChunk;
  for (int i = threadIdx.x; i < kAdamChunk; i += 256) {
    const int64_t e = base + i;
    if (e >= t.numel) break;
    // (every operation rounded on its own -- no fma contraction, whose choices
    // differed between the two kernels -- as torch's unfused CPU loop rounds)
    float p = t.param[e];
    float g = t.grad[e];
    if constexpr (COEF) g = g * coef;
    if (s.wd != 0.f) g = g + s.wd * p;
    float m = t.exp_avg[e];
    m = m + s.lerp_w * (g - m);
    float v = t.exp_avg_sq[e] * s.beta2;
    v = v + (s.one_minus_beta2 * g) * g;
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    p = p + s.neg_step_size * (m / denom);
    t.exp_avg[e] = m;
    t.exp_avg_sq[e] = v;
    t.param[e] = p;
  }
}

__global__ __launch_bounds__(256) void k_adam(const stgcn_adam_tensor_t *tab,
                                              const int64_t *chunk_start, int ntensors,
                                              AdamScalars s) {
  adam_block(tab, chunk_start, ntensors, s);
}

// The device-step form (stgcn_adam_step_dev, ABI 11): k_adam_tick advances the
// step count, then every block forms the scalars from it exactly as
// stgcn_adam_step does on the host (double, rounded to float) -- thread 0 into
// LDS -- and runs k_adam's element loop.
__global__ void k_adam_tick(float *step) { *step = *step + 1.f; }

__global__ __launch_bounds__(256) void k_adam_dev(const stgcn_adam_tensor_t *tab,
                                                  const int64_t *chunk_start, int ntensors,
                                                  const float *step, double lr, double beta1,
                                                  double beta2, double eps, double wd) {
  __shared__ AdamScalars sh;
  if (threadIdx.x == 0) {
    const double t = (double)*step;
    const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
    AdamScalars sc;
    sc.lerp_w = (float)(1.0 - beta1);
    sc.beta2 = (float)beta2;
    sc.one_minus_beta2 = (float)(1.0 - beta2);
    sc.neg_step_size = (float)(-(lr / bc1));
    sc.bc2_sqrt = (float)sqrt(bc2);
    sc.eps = (float)eps;
    sc.wd = (float)wd;
    sh = sc;
  }
  __syncthreads();
  const AdamScalars s = sh;
  adam_block(tab, chunk_start, ntensors, s);
}

// stgcn_adam_step_dev2 (STGCN_FEATURE_STEP_STATE): k_adam_dev with the learning
// rate, and optionally a gradient scale, read from device memory, so a captured
// step follows a scheduler and a clip coefficient without a re-capture.
__global__ __launch_bounds__(256) void k_adam_dev2(const stgcn_adam_tensor_t *tab,
                                                   const int64_t *chunk_start, int ntensors,
                                                   const float *step, const float *lr_dev,
                                                   const float *grad_coef, double beta1,
                                                   double beta2, double eps, double wd) {
  __shared__ AdamScalars sh;
  __shared__ float sh_coef;
  if (threadIdx.x == 0) {
    const double t = (double)*step;
    const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
    AdamScalars sc;
    sc.lerp_w = (float)(1.0 - beta1);
    sc.beta2 = (float)beta2;
    sc.one_minus_beta2 = (float)(1.0 - beta2);
    sc.neg_step_size = (float)(-((double)*lr_dev / bc1));
    sc.bc2_sqrt = (float)sqrt(bc2);
    sc.eps = (float)eps;
    sc.wd = (float)wd;
    sh = sc;
    sh_coef = grad_coef ? *grad_coef : 1.f;
  }
  __syncthreads();
  const AdamScalars s = sh;
  if (grad_coef)
    adam_block<true>(tab, chunk_start, ntensors, s, sh_coef);
  else
    adam_block(tab, chunk_start, ntensors, s);
}

// The dropout step token (stgcn_seed_next), in k_adam_tick's style
__global__ void k_seed_next(uint64_t *counter, uint64_t *token) {
  *counter += 1;
  *token = *counter;
}

// Gradient norm over an Adam table (stgcn_grad_norm). k_grad_sq: block b = chunk
// b of the table (adam_block's chunking), its sum of grad^2 in fp64 -- per
// thread in element order, then the block in a fixed tree -- stored to
// partials[b]. k_grad_norm: one workgroup adds the partials (thread i takes
// i, i + 256, ... in order; the same tree) and writes the norm and the clip
// coefficient. Plain stores only: the result does not depend on scheduling.
__device__ __forceinline__ double block_sum_fixed(double v, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void k_grad_sq(const stgcn_adam_tensor_t *tab,
                                                 const int64_t *chunk_start, int ntensors,
                                                 double *partials) {
  __shared__ double red[4];
  const int64_t b = blockIdx.x;
  int lo = 0, hi = ntensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk_start[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const float *grad = tab[lo].grad;
  const int64_t numel = tab[lo].numel;
  const int64_t base = (b - chunk_start[lo]) * kAdamChunk;
  double s = 0.0;
  for (int i = threadIdx.x; i < kAdamChunk; i += 256) {
    const int64_t e = base + i;
    if (e >= numel) break;
    const double g = (double)grad[e];
    s += g * g;
  }
  s = block_sum_fixed(s, red);
  if (threadIdx.x == 0) partials[b] = s;
}

__global__ __launch_bounds__(256) void k_grad_norm(const double *partials, int64_t n,
                                                   float max_norm, float *norm_out,
                                                   float *coef_out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) s += partials[i];
  s = block_sum_fixed(s, red);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s);
    *norm_out = norm;
    *coef_out = fminf(1.f, max_norm / (norm + 1e-6f));
  }
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
  const float mu = mean[c], a = invstd[c] * g[c], be = b[c];
  const float *src = U + row * L;
  float s = 0.f;
  for (int l = lane; l < L; l += 64) {
    const float t = (src[l] - mu) * a + be;
    s += t > 0.f ? t : 0.f;
  }
  s = wave_sumf(s);
  if (lane == 0) pooled[row] = s / (float)L;
}

// The logits row of clip blockIdx.x and its log-sum-exp, shared by k_head_fc_ce
// and k_head_eval_row (one function: the same instructions, so the evaluation
// head's logits and losses are bit-identical to the training head's). sh:
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

// one block per clip: logits = pooled W^T + b, per-clip CE loss (log-sum-exp)
__global__ __launch_bounds__(256) void k_head_fc_ce(const float *pooled, const float *W,
                                                    const float *bias, const int64_t *labels,
                                                    float *logits, float *lossv, int C,
                                                    int classes) {
  extern __shared__ float sh[];  // [C] pooled row, [classes] logits, [8] reduction
  float mx, tot;
  head_fc_lse(pooled, W, bias, logits, C, classes, sh, mx, tot);
  if (threadIdx.x == 0) {
    const float *lg = sh + C;
    const int n = blockIdx.x;
    const int64_t y = labels[n];
    lossv[n] = (y >= 0 && y < classes) ? (logf(tot) + mx) - lg[y] : NAN;  // bad label: NaN
  }
}

// ---------------------------------------------------------------------------
// Evaluation head (validation_step / test_step, lightning_model.py:213-253, and
// compute_conf_mat :123-133): the same logits and per-clip loss, the predicted
// class and the metrics of an epoch kept on the device.
// ---------------------------------------------------------------------------
// (value, index) maximum with ties going to the lowest index
__device__ __forceinline__ void argmax_take(float &bv, int &bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

// one block per clip: k_head_fc_ce's logits and loss (a label outside
// [0, classes) is cross entropy's ignore_index: loss 0, the label indexes
// nothing) and pred = the lowest index attaining the maximum logit, reduced as
// (value, index) pairs over the lanes of each wave, then over the four waves
__global__ __launch_bounds__(256) void k_head_eval_row(const float *pooled, const float *W,
                                                       const float *bias, const int64_t *labels,
                                                       float *logits, float *lossv, int32_t *pred,
                                                       int C, int classes) {
  extern __shared__ float sh[];  // [C] pooled row, [classes] logits, [8] reduction
  float mx, tot;
  head_fc_lse(pooled, W, bias, logits, C, classes, sh, mx, tot);
  __syncthreads();  // (every thread has read the reduction words: the argmax reuses them)
  const float *lg = sh + C;
  float *av = sh + C + classes;  // [4] value, [4] index per wave
  int *ai = reinterpret_cast<int *>(av + 4);
  const int n = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    const int64_t y = labels[n];
    lossv[n] = (y >= 0 && y < classes) ? (logf(tot) + mx) - lg[y] : 0.f;
  }
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

// STGCN_FEATURE_HEAD_LOSS: k_head_eval_row with F.cross_entropy's weight= and
// label_smoothing= (stgcn_hip.h, stgcn_head_eval_loss). With nll = lse - z[y]:
//   lossv = (1 - eps) * w[y] * nll + (eps / J) * sum_j w[j] * (lse - z[j])
// cw null: w = 1. om = 1 - eps and epsJ = eps / J are formed on the host in
// double. With eps = 0 the sum is not formed and om = 1, and without weights
// w[y] = 1, so lossv is nll itself: k_head_eval_row's bits. The sum over j is
// per thread in index order, then the wave, then the four waves in a fixed tree.
__global__ __launch_bounds__(256) void k_head_loss_row(const float *pooled, const float *W,
                                                       const float *bias, const float *cw,
                                                       const int64_t *labels, float *logits,
                                                       float *lossv, int32_t *pred, int C,
                                                       int classes, float om, float epsJ) {
  extern __shared__ float sh[];  // [C] pooled row, [classes] logits, [8] reduction
  float mx, tot;
  head_fc_lse(pooled, W, bias, logits, C, classes, sh, mx, tot);
  __syncthreads();  // (every thread has read the reduction words: reused below)
  const float *lg = sh + C;
  float *av = sh + C + classes;  // [4] value, [4] index per wave
  int *ai = reinterpret_cast<int *>(av + 4);
  const int n = blockIdx.x, tid = threadIdx.x;
  const float lse = logf(tot) + mx;
  float sm = 0.f;
  if (epsJ > 0.f) {  // (uniform over the launch)
    for (int j = tid; j < classes; j += 256) sm += (cw ? cw[j] : 1.f) * (lse - lg[j]);
    sm = wave_sumf(sm);
    if ((tid & 63) == 0) av[tid >> 6] = sm;
    __syncthreads();
    sm = (av[0] + av[1]) + (av[2] + av[3]);
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t y = labels[n];
    float l = 0.f;
    if (y >= 0 && y < classes) {
      l = om * (cw ? cw[y] : 1.f) * (lse - lg[y]);
      if (epsJ > 0.f) l = fmaf(epsJ, sm, l);
    }
    lossv[n] = l;
  }
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

// The batch pass, ONE workgroup: loss = the mean of lossv over the clips with a
// valid label (k_head_loss_mean's fixed-order fp64 sum, so the same bits when
// every label is valid; 0 without a valid clip) and, metrics non-null, the
// epoch's words and confusion matrix. Wave w takes clips w, w + 4, ..: its
// lanes count the logits that rank before the label's (top-k hit: fewer than
// topk of them). Counts are integers, the sums one fp64 add per word from
// thread 0, the matrix integer atomics: the result does not depend on order.
// cw (STGCN_FEATURE_HEAD_LOSS, k_head_loss_batch): the denominator is D = the
// sum of w[label] over the valid clips, in fp64 in clip order, instead of their
// count (the same double when cw is null), written to denom[0] as a float; loss
// = 0 when D == 0.
__device__ __forceinline__ void head_eval_batch_body(const float *logits, const int64_t *labels,
                                                     const float *lossv, const int32_t *pred,
                                                     float *loss, void *metrics, int N,
                                                     int classes, int topk, const float *cw,
                                                     float *denom) {
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

__global__ __launch_bounds__(256) void k_head_eval_batch(const float *logits,
                                                         const int64_t *labels,
                                                         const float *lossv,
                                                         const int32_t *pred, float *loss,
                                                         void *metrics, int N, int classes,
                                                         int topk) {
  head_eval_batch_body(logits, labels, lossv, pred, loss, metrics, N, classes, topk, nullptr,
                       nullptr);
}

__global__ __launch_bounds__(256) void k_head_loss_batch(const float *logits,
                                                         const int64_t *labels,
                                                         const float *lossv,
                                                         const int32_t *pred, const float *cw,
                                                         float *loss, float *denom,
                                                         void *metrics, int N, int classes,
                                                         int topk) {
  head_eval_batch_body(logits, labels, lossv, pred, loss, metrics, N, classes, topk, cw, denom);
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

}  // namespace

extern "C" {

size_t stgcn_adam_table_bytes(int ntensors) {
  if (ntensors <= 0) return 0;
  return (size_t)ntensors * sizeof(stgcn_adam_tensor_t) + (size_t)(ntensors + 1) * sizeof(int64_t);
}

int stgcn_adam_build_table(const stgcn_adam_tensor_t *tensors, int ntensors, void *host_table,
                           size_t table_bytes, int64_t *total_chunks) {
  if (!tensors || ntensors <= 0 || !host_table || !total_chunks)
    return fail(STGCN_E_INVALID, "adam: null argument or no tensors");
  if (table_bytes < stgcn_adam_table_bytes(ntensors))
    return fail(STGCN_E_INVALID, "adam: table buffer too small");
  auto *tab = reinterpret_cast<stgcn_adam_tensor_t *>(host_table);
  auto *cs = reinterpret_cast<int64_t *>(reinterpret_cast<char *>(host_table) +
                                         (size_t)ntensors * sizeof(stgcn_adam_tensor_t));
  int64_t chunks = 0;
  for (int i = 0; i < ntensors; ++i) {
    const stgcn_adam_tensor_t &t = tensors[i];
    if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq || t.numel <= 0)
      return fail(STGCN_E_INVALID,
                  "adam: tensor " + std::to_string(i) + " has a null pointer or numel <= 0");
    if ((((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg |
          (uintptr_t)t.exp_avg_sq) & 3) != 0)
      return fail(STGCN_E_INVALID,
                  "adam: tensor " + std::to_string(i) + ": param / grad / exp_avg / exp_avg_sq "
                  "must be 4-byte aligned");
    tab[i] = t;
    cs[i] = chunks;
    chunks += (t.numel + kAdamChunk - 1) / kAdamChunk;
  }
  cs[ntensors] = chunks;
  if (chunks > INT32_MAX) return fail(STGCN_E_UNSUPPORTED, "adam: too many elements");
  *total_chunks = chunks;
  return STGCN_OK;
}

int stgcn_adam_step(const void *dev_table, int ntensors, int64_t total_chunks, double lr,
                    double beta1, double beta2, double eps, double weight_decay, int64_t step,
                    void *stream) {
  if (!dev_table || ntensors <= 0 || total_chunks <= 0 || step <= 0)
    return fail(STGCN_E_INVALID, "adam: bad table / chunk count / step");
  if (int rc = check_aligned({NP(dev_table)}, 8)) return rc;
  // scalars as torch forms them: Python doubles, rounded to float at the kernel
  const double bc1 = 1.0 - std::pow(beta1, (double)step);
  const double bc2 = 1.0 - std::pow(beta2, (double)step);
  AdamScalars sc;
  sc.lerp_w = (float)(1.0 - beta1);
  sc.beta2 = (float)beta2;
  sc.one_minus_beta2 = (float)(1.0 - beta2);
  sc.neg_step_size = (float)(-(lr / bc1));
  sc.bc2_sqrt = (float)std::sqrt(bc2);
  sc.eps = (float)eps;
  sc.wd = (float)weight_decay;
  const auto *tab = reinterpret_cast<const stgcn_adam_tensor_t *>(dev_table);
  const auto *cs = reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(dev_table) +
                                                     (size_t)ntensors * sizeof(stgcn_adam_tensor_t));
  hipLaunchKernelGGL(k_adam, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tab,
                     cs, ntensors, sc);
  HIP_TRY2(hipGetLastError());
  return STGCN_OK;
}

int stgcn_adam_step_dev(const void *dev_table, int ntensors, int64_t total_chunks, double lr,
                        double beta1, double beta2, double eps, double weight_decay, float *step,
                        void *stream) {
  if (!dev_table || ntensors <= 0 || total_chunks <= 0 || !step)
    return fail(STGCN_E_INVALID, "adam: bad table / chunk count / step pointer");
  if (int rc = check_aligned({NP(dev_table)}, 8)) return rc;
  if (int rc = check_aligned({NP(step)}, 4)) return rc;
  const auto *tab = reinterpret_cast<const stgcn_adam_tensor_t *>(dev_table);
  const auto *cs = reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(dev_table) +
                                                     (size_t)ntensors * sizeof(stgcn_adam_tensor_t));
  hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, (hipStream_t)stream, step);
  hipLaunchKernelGGL(k_adam_dev, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream,
                     tab, cs, ntensors, step, lr, beta1, beta2, eps, weight_decay);
  HIP_TRY2(hipGetLastError());
  return STGCN_OK;
}

int stgcn_adam_step_dev2(const void *dev_table, int ntensors, int64_t total_chunks,
                         const float *lr_dev, const float *grad_coef, double beta1, double beta2,
                         double eps, double weight_decay, float *step, void *stream) {
  if (!dev_table || ntensors <= 0 || total_chunks <= 0 || !step)
    return fail(STGCN_E_INVALID, "adam: bad table / chunk count / step pointer");
  if (!lr_dev) return fail(STGCN_E_INVALID, "adam: lr_dev is null");
  if (int rc = check_aligned({NP(dev_table)}, 8)) return rc;
  if (int rc = check_aligned({NP(step), NP(lr_dev), NP(grad_coef)}, 4)) return rc;
  const auto *tab = reinterpret_cast<const stgcn_adam_tensor_t *>(dev_table);
  const auto *cs = reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(dev_table) +
                                                     (size_t)ntensors * sizeof(stgcn_adam_tensor_t));
  hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, (hipStream_t)stream, step);
  hipLaunchKernelGGL(k_adam_dev2, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream,
                     tab, cs, ntensors, step, lr_dev, grad_coef, beta1, beta2, eps, weight_decay);
  HIP_TRY2(hipGetLastError());
  return STGCN_OK;
}

size_t stgcn_grad_norm_bytes(int64_t total_chunks) {
  return total_chunks > 0 ? (size_t)total_chunks * sizeof(double) : 0;
}

int stgcn_grad_norm(const void *dev_table, int ntensors, int64_t total_chunks, double max_norm,
                    double *partials, float *norm_out, float *coef_out, void *stream) {
  if (!dev_table || ntensors <= 0 || total_chunks <= 0 || total_chunks > INT32_MAX)
    return fail(STGCN_E_INVALID, "grad_norm: bad table / chunk count");
  if (!partials) return fail(STGCN_E_INVALID, "grad_norm: partials is null");
  if (!norm_out) return fail(STGCN_E_INVALID, "grad_norm: norm_out is null");
  if (!coef_out) return fail(STGCN_E_INVALID, "grad_norm: coef_out is null");
  if (!(max_norm > 0.0)) return fail(STGCN_E_INVALID, "grad_norm: max_norm must be positive");
  if (int rc = check_aligned({NP(dev_table), NP(partials)}, 8)) return rc;
  if (int rc = check_aligned({NP(norm_out), NP(coef_out)}, 4)) return rc;
  const auto *tab = reinterpret_cast<const stgcn_adam_tensor_t *>(dev_table);
  const auto *cs = reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(dev_table) +
                                                     (size_t)ntensors * sizeof(stgcn_adam_tensor_t));
  hipLaunchKernelGGL(k_grad_sq, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream,
                     tab, cs, ntensors, partials);
  hipLaunchKernelGGL(k_grad_norm, dim3(1), dim3(256), 0, (hipStream_t)stream, partials,
                     total_chunks, (float)max_norm, norm_out, coef_out);
  HIP_TRY2(hipGetLastError());
  return STGCN_OK;
}

int stgcn_seed_next(uint64_t *counter, uint64_t *token, void *stream) {
  if (!counter) return fail(STGCN_E_INVALID, "seed_next: counter is null");
  if (!token) return fail(STGCN_E_INVALID, "seed_next: token is null");
  if (int rc = check_aligned({NP(counter), NP(token)}, 8)) return rc;
  hipLaunchKernelGGL(k_seed_next, dim3(1), dim3(1), 0, (hipStream_t)stream, counter, token);
  HIP_TRY2(hipGetLastError());
  return STGCN_OK;
}

int stgcn_head_fwd(const stgcn_head_desc_t *d, const float *y, const float *W, const float *bias,
                   const int64_t *labels, float *pooled, float *logits, float *lossv, float *loss,
                   void *stream) {
  if (!d || d->N <= 0 || d->C <= 0 || d->L <= 0 || d->classes <= 0)
    return fail(STGCN_E_INVALID, "head: bad descriptor");
  if (!y || !W || !bias || !labels || !pooled || !logits || !lossv || !loss)
    return fail(STGCN_E_INVALID, "head: null tensor argument");
  if (int rc = check_aligned({NP(y), NP(W), NP(bias), NP(pooled), NP(logits), NP(lossv), NP(loss)}, 4))
    return rc;
  if (int rc = check_aligned({NP(labels)}, 8)) return rc;
  if ((size_t)(d->C + d->classes + 8) * sizeof(float) > 64 * 1024)
    return fail(STGCN_E_UNSUPPORTED, "head: C + classes too large");
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)d->N * d->C;
  hipLaunchKernelGGL(k_head_pool, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, y, pooled,
                     rows, d->L);
  hipLaunchKernelGGL(k_head_fc_ce, dim3(d->N), dim3(256),
                     (size_t)(d->C + d->classes + 8) * sizeof(float), s, pooled, W, bias, labels,
                     logits, lossv, d->C, d->classes);
  hipLaunchKernelGGL(k_head_loss_mean, dim3(1), dim3(64), 0, s, lossv, loss, d->N);
  HIP_TRY2(hipGetLastError());
  return STGCN_OK;
}

int stgcn_head_fwd_u(const stgcn_head_desc_t *d, const float *U, const float *stats2,
                     const float *g2, const float *b2, const float *W, const float *bias,
                     const int64_t *labels, float *pooled, float *logits, float *lossv,
                     float *loss, void *stream) {
  if (!d || d->N <= 0 || d->C <= 0 || d->L <= 0 || d->classes <= 0)
    return fail(STGCN_E_INVALID, "head: bad descriptor");
  if (!U || !stats2 || !g2 || !b2 || !W || !bias || !labels || !pooled || !logits || !lossv ||
      !loss)
    return fail(STGCN_E_INVALID, "head: null tensor argument");
  if (int rc = check_aligned({NP(U), NP(stats2), NP(g2), NP(b2), NP(W), NP(bias), NP(pooled),
                              NP(logits), NP(lossv), NP(loss)},
                             4))
    return rc;
  if (int rc = check_aligned({NP(labels)}, 8)) return rc;
  if ((size_t)(d->C + d->classes + 8) * sizeof(float) > 64 * 1024)
    return fail(STGCN_E_UNSUPPORTED, "head: C + classes too large");
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)d->N * d->C;
  hipLaunchKernelGGL(k_head_pool_u, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, U, stats2,
                     stats2 + d->C, g2, b2, pooled, rows, d->C, d->L);
  hipLaunchKernelGGL(k_head_fc_ce, dim3(d->N), dim3(256),
                     (size_t)(d->C + d->classes + 8) * sizeof(float), s, pooled, W, bias, labels,
                     logits, lossv, d->C, d->classes);
  hipLaunchKernelGGL(k_head_loss_mean, dim3(1), dim3(64), 0, s, lossv, loss, d->N);
  HIP_TRY2(hipGetLastError());
  return STGCN_OK;
}

int stgcn_features(void) {
  return STGCN_FEATURE_EVAL_CHAIN | STGCN_FEATURE_EVAL_HEAD | STGCN_FEATURE_STEP_STATE |
         STGCN_FEATURE_INPUT_STAGE | STGCN_FEATURE_OPTIMIZERS | STGCN_FEATURE_HEAD_LOSS;
}

// (classes of a metrics block: the head's own LDS limit at C = 1)
static bool eval_classes_ok(int classes) {
  return classes > 0 && (size_t)(1 + classes + 8) * sizeof(float) <= 64 * 1024;
}

size_t stgcn_eval_metrics_bytes(int classes) {
  if (!eval_classes_ok(classes)) return 0;
  return 8 * sizeof(int64_t) + (size_t)classes * classes * sizeof(int64_t);
}

int stgcn_eval_metrics_reset(void *metrics, int classes, void *stream) {
  const size_t nbytes = stgcn_eval_metrics_bytes(classes);
  if (!metrics || !nbytes) return fail(STGCN_E_INVALID, "eval metrics: null block or bad classes");
  if (int rc = check_aligned({NP(metrics)}, 8)) return rc;
  HIP_TRY2(hipMemsetAsync(metrics, 0, nbytes, (hipStream_t)stream));
  return STGCN_OK;
}

// the checks of both forms of the evaluation head (src: y or U)
static int head_eval_check(const stgcn_eval_desc_t *d, const void *src, const float *W,
                           const float *bias, const int64_t *labels, const float *pooled,
                           const float *logits, const float *lossv, const float *loss,
                           const int32_t *pred) {
  if (!d || d->N <= 0 || d->C <= 0 || d->L <= 0 || d->classes <= 0)
    return fail(STGCN_E_INVALID, "head: bad descriptor");
  if (d->topk < 1 || d->topk > d->classes)
    return fail(STGCN_E_INVALID, "head: topk outside [1, classes]");
  if (!src || !W || !bias || !labels || !pooled || !logits || !lossv || !loss || !pred)
    return fail(STGCN_E_INVALID, "head: null tensor argument");
  if (int rc = check_aligned({NamedPtr{src, "y / U"}, NP(W), NP(bias), NP(pooled), NP(logits),
                              NP(lossv), NP(loss), NP(pred)},
                             4))
    return rc;
  if (int rc = check_aligned({NP(labels)}, 8)) return rc;
  return STGCN_OK;
}
// (after every argument check of either form)
static int head_eval_fits(const stgcn_eval_desc_t *d) {
  if ((size_t)(d->C + d->classes + 8) * sizeof(float) > 64 * 1024)
    return fail(STGCN_E_UNSUPPORTED, "head: C + classes too large");
  return STGCN_OK;
}

// logits, losses and predictions from pooled, then the batch pass
static int head_eval_tail(const stgcn_eval_desc_t *d, const float *W, const float *bias,
                          const int64_t *labels, float *pooled, float *logits, float *lossv,
                          float *loss, int32_t *pred, void *metrics, hipStream_t s) {
  hipLaunchKernelGGL(k_head_eval_row, dim3(d->N), dim3(256),
                     (size_t)(d->C + d->classes + 8) * sizeof(float), s, pooled, W, bias, labels,
                     logits, lossv, pred, d->C, d->classes);
  hipLaunchKernelGGL(k_head_eval_batch, dim3(1), dim3(256), 0, s, logits, labels, lossv, pred,
                     loss, metrics, d->N, d->classes, d->topk);
  HIP_TRY2(hipGetLastError());
  return STGCN_OK;
}

int stgcn_head_eval(const stgcn_eval_desc_t *d, const float *y, const float *W, const float *bias,
                    const int64_t *labels, float *pooled, float *logits, float *lossv,
                    float *loss, int32_t *pred, void *metrics, void *stream) {
  int rc = head_eval_check(d, y, W, bias, labels, pooled, logits, lossv, loss, pred);
  if (rc) return rc;
  if ((rc = check_aligned({NP(metrics)}, 8))) return rc;
  if ((rc = head_eval_fits(d))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)d->N * d->C;
  hipLaunchKernelGGL(k_head_pool, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, y, pooled,
                     rows, d->L);
  return head_eval_tail(d, W, bias, labels, pooled, logits, lossv, loss, pred, metrics, s);
}

int stgcn_head_eval_u(const stgcn_eval_desc_t *d, const float *U, const float *stats2,
                      const float *g2, const float *b2, const float *W, const float *bias,
                      const int64_t *labels, float *pooled, float *logits, float *lossv,
                      float *loss, int32_t *pred, void *metrics, void *stream) {
  int rc = head_eval_check(d, U, W, bias, labels, pooled, logits, lossv, loss, pred);
  if (rc) return rc;
  if (!stats2 || !g2 || !b2) return fail(STGCN_E_INVALID, "head: null tensor argument");
  if ((rc = check_aligned({NP(stats2), NP(g2), NP(b2)}, 4))) return rc;
  if ((rc = check_aligned({NP(metrics)}, 8))) return rc;
  if ((rc = head_eval_fits(d))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)d->N * d->C;
  hipLaunchKernelGGL(k_head_pool_u, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, U, stats2,
                     stats2 + d->C, g2, b2, pooled, rows, d->C, d->L);
  return head_eval_tail(d, W, bias, labels, pooled, logits, lossv, loss, pred, metrics, s);
}

// STGCN_FEATURE_HEAD_LOSS ----------------------------------------------------
// (everything stgcn_loss_check refuses but the LDS limit, which the entry points
// apply after their argument checks, as stgcn_head_eval does)
static int loss_desc_check(const stgcn_loss_desc_t *d) {
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
static int loss_desc_fits(const stgcn_loss_desc_t *d) {
  if ((size_t)((int64_t)d->C + d->classes + 8) * sizeof(float) > 64 * 1024)
    return fail(STGCN_E_UNSUPPORTED, "loss: C + classes too large");
  return STGCN_OK;
}

int stgcn_loss_check(const stgcn_loss_desc_t *d) {
  if (int rc = loss_desc_check(d)) return rc;
  return loss_desc_fits(d);
}

// the argument checks of both forms (src: y or U)
static int head_eval_loss_check(const stgcn_loss_desc_t *d, const void *src, const float *W,
                                const float *bias, const float *class_weight,
                                const int64_t *labels, const float *pooled, const float *logits,
                                const float *lossv, const float *denom, const float *loss,
                                const int32_t *pred, const void *metrics) {
  if (int rc = loss_desc_check(d)) return rc;
  if (!src || !W || !bias || !labels || !pooled || !logits || !lossv || !denom || !loss || !pred)
    return fail(STGCN_E_INVALID, "loss: null tensor argument");
  if ((d->flags & STGCN_LOSS_WEIGHT) && !class_weight)
    return fail(STGCN_E_INVALID, "loss: STGCN_LOSS_WEIGHT without class_weight");
  if (!(d->flags & STGCN_LOSS_WEIGHT) && class_weight)
    return fail(STGCN_E_INVALID, "loss: class_weight without STGCN_LOSS_WEIGHT");
  if (int rc = check_aligned({NamedPtr{src, "y / U"}, NP(W), NP(bias), NP(class_weight),
                              NP(pooled), NP(logits), NP(lossv), NP(denom), NP(loss), NP(pred)},
                             4))
    return rc;
  if (int rc = check_aligned({NP(labels), NP(metrics)}, 8)) return rc;
  return STGCN_OK;
}

static int head_eval_loss_tail(const stgcn_loss_desc_t *d, const float *W, const float *bias,
                               const float *class_weight, const int64_t *labels, float *pooled,
                               float *logits, float *lossv, float *denom, float *loss,
                               int32_t *pred, void *metrics, hipStream_t s) {
  const double eps = d->label_smoothing;
  hipLaunchKernelGGL(k_head_loss_row, dim3(d->N), dim3(256),
                     (size_t)(d->C + d->classes + 8) * sizeof(float), s, pooled, W, bias,
                     class_weight, labels, logits, lossv, pred, d->C, d->classes,
                     (float)(1.0 - eps), (float)(eps / d->classes));
  hipLaunchKernelGGL(k_head_loss_batch, dim3(1), dim3(256), 0, s, logits, labels, lossv, pred,
                     class_weight, loss, denom, metrics, d->N, d->classes, d->topk);
  HIP_TRY2(hipGetLastError());
  return STGCN_OK;
}

int stgcn_head_eval_loss(const stgcn_loss_desc_t *d, const float *y, const float *W,
                         const float *bias, const float *class_weight, const int64_t *labels,
                         float *pooled, float *logits, float *lossv, float *denom, float *loss,
                         int32_t *pred, void *metrics, void *stream) {
  int rc = head_eval_loss_check(d, y, W, bias, class_weight, labels, pooled, logits, lossv, denom,
                                loss, pred, metrics);
  if (rc) return rc;
  if ((rc = loss_desc_fits(d))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)d->N * d->C;
  hipLaunchKernelGGL(k_head_pool, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, y, pooled,
                     rows, d->L);
  return head_eval_loss_tail(d, W, bias, class_weight, labels, pooled, logits, lossv, denom, loss,
                             pred, metrics, s);
}

int stgcn_head_eval_loss_u(const stgcn_loss_desc_t *d, const float *U, const float *stats2,
                           const float *g2, const float *b2, const float *W, const float *bias,
                           const float *class_weight, const int64_t *labels, float *pooled,
                           float *logits, float *lossv, float *denom, float *loss, int32_t *pred,
                           void *metrics, void *stream) {
  int rc = head_eval_loss_check(d, U, W, bias, class_weight, labels, pooled, logits, lossv, denom,
                                loss, pred, metrics);
  if (rc) return rc;
  if (!stats2 || !g2 || !b2) return fail(STGCN_E_INVALID, "loss: null tensor argument");
  if ((rc = check_aligned({NP(stats2), NP(g2), NP(b2)}, 4))) return rc;
  if ((rc = loss_desc_fits(d))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)d->N * d->C;
  hipLaunchKernelGGL(k_head_pool_u, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, U, stats2,
                     stats2 + d->C, g2, b2, pooled, rows, d->C, d->L);
  return head_eval_loss_tail(d, W, bias, class_weight, labels, pooled, logits, lossv, denom, loss,
                             pred, metrics, s);
}

int stgcn_head_bwd(const stgcn_head_desc_t *d, const float *pooled, const float *logits,
                   const float *W, const int64_t *labels, const float *dloss, float *dlogits,
                   float *dpooled, float *dy, float *dW, float *dbias, void *stream) {
  if (!d || d->N <= 0 || d->C <= 0 || d->L <= 0 || d->classes <= 0)
    return fail(STGCN_E_INVALID, "head: bad descriptor");
  if (!pooled || !logits || !W || !labels || !dloss || !dlogits || !dpooled || !dy || !dW ||
      !dbias)
    return fail(STGCN_E_INVALID, "head: null tensor argument");
  if (int rc = check_aligned({NP(pooled), NP(logits), NP(W), NP(dloss), NP(dlogits), NP(dpooled),
                              NP(dy), NP(dW), NP(dbias)},
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
  hipLaunchKernelGGL(k_head_bcast, dim3((unsigned)rows), dim3(256), 0, s, dpooled, dy, rows,
                     d->L);
  HIP_TRY2(hipGetLastError());
  return STGCN_OK;
}

int stgcn_head_bwd_nc(const stgcn_head_desc_t *d, const float *pooled, const float *logits,
                      const float *W, const int64_t *labels, const float *dloss, float *dlogits,
                      float *dpooled, float *dy_nc, float *dW, float *dbias, void *stream) {
  if (!d || d->N <= 0 || d->C <= 0 || d->L <= 0 || d->classes <= 0)
    return fail(STGCN_E_INVALID, "head: bad descriptor");
  if (!pooled || !logits || !W || !labels || !dloss || !dlogits || !dpooled || !dy_nc || !dW ||
      !dbias)
    return fail(STGCN_E_INVALID, "head: null tensor argument");
  if (int rc = check_aligned({NP(pooled), NP(logits), NP(W), NP(dloss), NP(dlogits), NP(dpooled),
                              NP(dy_nc), NP(dW), NP(dbias)},
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
  hipLaunchKernelGGL(k_head_dync, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, dpooled,
                     dy_nc, rows, d->L);
  HIP_TRY2(hipGetLastError());
  return STGCN_OK;
}

}  // extern "C"
