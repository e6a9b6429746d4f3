// The optimizer step of the training-step layer, gfx950 only: multi-tensor Adam
// (torch.optim.Adam, lightning_model.py:196-197) with decoupled weight decay
// (torch.optim.AdamW) and AMSGrad, and the gradient norm of clip_grad_norm_.
// ONE launch over every tensor of a table: 2048 elements per 256-thread block, a
// binary search of the chunk prefix sums for the block's tensor. stgcn_adam_step
// / _dev / _dev2 (tables of stgcn_adam_tensor_t) and stgcn_opt_step (tables of
// stgcn_opt_tensor_t) launch the same kernel template. The arithmetic is stated
// in include/stgcn_hip.h and DESIGN.md §1.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <type_traits>

#include "../../include/stgcn_hip.h"
#include "host_common.h"

namespace {

using stgcn::check_aligned;
using stgcn::fail;
using stgcn::NamedPtr;

constexpr int kChunk = 2048;  // elements per block (256 threads x 8)

// tensor of this block: the last t with chunk_start[t] <= blockIdx.x
__device__ __forceinline__ int block_tensor(const int64_t *chunk_start, int ntensors) {
  const int64_t b = blockIdx.x;
  int lo = 0, hi = ntensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk_start[mid] <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// A table (host or device copy): ntensors entries, then ntensors + 1 chunk
// prefix sums
template <typename T>
size_t table_bytes(int ntensors) {
  if (ntensors <= 0) return 0;
  return (size_t)ntensors * sizeof(T) + (size_t)(ntensors + 1) * sizeof(int64_t);
}
template <typename T>
const int64_t *chunk_starts(const void *table, int ntensors) {
  return reinterpret_cast<const int64_t *>(reinterpret_cast<const T *>(table) + ntensors);
}

// The pointers of one table entry, whichever its type
struct Entry {
  float *param;
  const float *grad;
  float *m, *v, *vmax;  // exp_avg, exp_avg_sq, max_exp_avg_sq (AMSGrad)
  int64_t numel;
};
__device__ __forceinline__ Entry entry(const stgcn_adam_tensor_t &t) {
  return {t.param, t.grad, t.exp_avg, t.exp_avg_sq, nullptr, t.numel};
}
__device__ __forceinline__ Entry entry(const stgcn_opt_tensor_t &t) {
  return {t.param, t.grad, t.s0, t.s1, t.s2, t.numel};
}

// ---------------------------------------------------------------------------
// Adam. Per element, in fp32, in torch's order (optim/adam.py _multi_tensor_adam /
// _single_tensor_adam), every operation rounded on its own:
//   g  = grad * coef                    (COEF: the clip coefficient)
//   g  = g + wd * p                     (wd != 0, not decoupled)
//   p  = p * decay                      (decoupled: 1 - lr * wd; else 1: exact)
//   m  = lerp(m, g, 1 - beta1)          (m + w (g - m) for w < 0.5)
//   v  = v * beta2;  v = v + ((1 - beta2) * g) * g
//   vd = vmax = max(vmax, v)            (AMS; else vd = v)
//   p  = p + (-lr / bc1) * (m / (sqrt(vd) / sqrt(bc2) + eps))
// with bc1 = 1 - beta1^step, bc2 = 1 - beta2^step. The scalars are formed from
// doubles and rounded to float like torch's scalar arguments, on the host for a
// host step count and a by-value lr, else by thread 0 of every block (the same
// expressions).
// ---------------------------------------------------------------------------
struct AdamScalars {
  float lerp_w, beta2, one_minus_beta2, neg_step_size, bc2_sqrt, eps, wd, decay;
};

__host__ __device__ inline AdamScalars adam_scalars(double t, double lr, double beta1,
                                                    double beta2, double eps, double wd,
                                                    bool decoupled) {
#pragma clang fp contract(off)  // (1 - lr * wd as Python forms it, on both sides)
  const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
  AdamScalars sc;
  sc.lerp_w = (float)(1.0 - beta1);
  sc.beta2 = (float)beta2;
  sc.one_minus_beta2 = (float)(1.0 - beta2);
  sc.neg_step_size = (float)(-(lr / bc1));
  sc.bc2_sqrt = (float)sqrt(bc2);
  sc.eps = (float)eps;
  sc.wd = decoupled ? 0.f : (float)wd;
  sc.decay = decoupled && wd != 0.0 ? (float)(1.0 - lr * wd) : 1.f;
  return sc;
}

// One step in any launch form (launch_adam fills host)
struct AdamArgs {
  AdamScalars host;  // used when neither step_dev nor lr_dev is given
  double lr, beta1, beta2, eps, wd, step;
  float *step_dev;             // the device step count, advanced by the call, or null
  const float *lr_dev, *coef;  // device words read when the kernel runs, or null
  int decoupled;
};

__global__ void k_adam_tick(float *step) { *step = *step + 1.f; }

// T: stgcn_adam_tensor_t or stgcn_opt_tensor_t (the table's entry type)
template <typename T, bool AMS, bool COEF>
__global__ __launch_bounds__(256) void k_adam(const T *tab, const int64_t *chunk_start,
                                              int ntensors, AdamArgs a) {
#pragma clang fp contract(off)
  __shared__ AdamScalars sh;
  __shared__ float sh_coef;
  if (threadIdx.x == 0) {
    if (a.step_dev || a.lr_dev)
      sh = adam_scalars(a.step_dev ? (double)*a.step_dev : a.step,
                        a.lr_dev ? (double)*a.lr_dev : a.lr, a.beta1, a.beta2, a.eps, a.wd,
                        a.decoupled != 0);
    else
      sh = a.host;
    sh_coef = COEF ? *a.coef : 1.f;
  }
  __syncthreads();
  const AdamScalars s = sh;
  const float coef = sh_coef;
  const int ti = block_tensor(chunk_start, ntensors);
  const Entry t = entry(tab[ti]);
  const int64_t base = ((int64_t)blockIdx.x - chunk_start[ti]) * kChunk;
  for (int i = threadIdx.x; i < kChunk; i += 256) {
    const int64_t e = base + i;
    if (e >= t.numel) break;
    // (no fma contraction: as torch's unfused CPU loop rounds)
    float p = t.param[e];
    float g = t.grad[e];
    if constexpr (COEF) g = g * coef;
    if (s.wd != 0.f) g = g + s.wd * p;
    p = p * s.decay;  // (1 without decoupled decay: exact)
    float m = t.m[e];
    m = m + s.lerp_w * (g - m);
    float v = t.v[e] * s.beta2;
    v = v + (s.one_minus_beta2 * g) * g;
    float vd = v;
    if constexpr (AMS) {
      const float vm = t.vmax[e];
      vd = (v > vm || v != v) ? v : vm;  // torch.maximum: a NaN on either side stays
      t.vmax[e] = vd;
    }
    const float denom = sqrtf(vd) / s.bc2_sqrt + s.eps;
    p = p + s.neg_step_size * (m / denom);
    t.m[e] = m;
    t.v[e] = v;
    t.param[e] = p;
  }
}

template <typename T, bool AMS>
void launch_adam_kernel(unsigned grid, hipStream_t s, const void *dev_table, int ntensors,
                        const AdamArgs &a) {
  const T *tab = reinterpret_cast<const T *>(dev_table);
  const int64_t *cs = chunk_starts<T>(dev_table, ntensors);
  if (a.coef)
    hipLaunchKernelGGL((k_adam<T, AMS, true>), dim3(grid), dim3(256), 0, s, tab, cs, ntensors, a);
  else
    hipLaunchKernelGGL((k_adam<T, AMS, false>), dim3(grid), dim3(256), 0, s, tab, cs, ntensors, a);
}

// The launches of every Adam entry point, after its own argument checks: the
// tick of a device step count, then the element kernel. The caller reads
// hipGetLastError().
template <typename T>
void launch_adam(const void *dev_table, int ntensors, int64_t total_chunks, bool amsgrad,
                 AdamArgs a, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  a.host = AdamScalars{};
  if (!a.step_dev && !a.lr_dev)
    a.host = adam_scalars(a.step, a.lr, a.beta1, a.beta2, a.eps, a.wd, a.decoupled != 0);
  if (a.step_dev) hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, s, a.step_dev);
  const unsigned grid = (unsigned)total_chunks;
  if constexpr (std::is_same_v<T, stgcn_opt_tensor_t>) {  // (an Adam entry has no vmax slot)
    if (amsgrad) return launch_adam_kernel<T, true>(grid, s, dev_table, ntensors, a);
  }
  launch_adam_kernel<T, false>(grid, s, dev_table, ntensors, a);
}

// the arguments of the legacy entry points (stgcn_adam_step / _dev / _dev2)
AdamArgs legacy_args(double lr, double beta1, double beta2, double eps, double wd) {
  AdamArgs a{};
  a.lr = lr;
  a.beta1 = beta1;
  a.beta2 = beta2;
  a.eps = eps;
  a.wd = wd;
  return a;
}

// A host table from the caller's entries: prep(i, entry) checks (and may amend)
// each one; then the chunk prefix sums. who: the prefix of the error texts.
template <typename T, typename Prep>
int fill_table(const char *who, const T *tensors, int ntensors, void *host_table,
               int64_t *total_chunks, Prep prep) {
  T *tab = reinterpret_cast<T *>(host_table);
  int64_t *cs = const_cast<int64_t *>(chunk_starts<T>(host_table, ntensors));
  int64_t chunks = 0;
  for (int i = 0; i < ntensors; ++i) {
    T t = tensors[i];
    if (int rc = prep(i, t)) return rc;
    tab[i] = t;
    cs[i] = chunks;
    chunks += (t.numel + kChunk - 1) / kChunk;
  }
  cs[ntensors] = chunks;
  if (chunks > INT32_MAX)
    return fail(STGCN_E_UNSUPPORTED, std::string(who) + ": too many elements");
  *total_chunks = chunks;
  return STGCN_OK;
}

// Gradient norm over an Adam table (stgcn_grad_norm). k_grad_sq: block b = chunk
// b of the table (k_adam's chunking), its sum of grad^2 in fp64 -- per
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
  const int ti = block_tensor(chunk_start, ntensors);
  const float *grad = tab[ti].grad;
  const int64_t numel = tab[ti].numel;
  const int64_t base = (b - chunk_start[ti]) * kChunk;
  double s = 0.0;
  for (int i = threadIdx.x; i < kChunk; i += 256) {
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
    const float c = max_norm / (norm + 1e-6f);
    *coef_out = c > 1.f ? 1.f : c;  // clamp(max = 1): a NaN norm gives a NaN coefficient
  }
}

}  // namespace

extern "C" {

size_t stgcn_adam_table_bytes(int ntensors) { return table_bytes<stgcn_adam_tensor_t>(ntensors); }

int stgcn_adam_build_table(const stgcn_adam_tensor_t *tensors, int ntensors, void *host_table,
                           size_t table_bytes, int64_t *total_chunks) {
  if (!tensors || ntensors <= 0 || !host_table || !total_chunks)
    return fail(STGCN_E_INVALID, "adam: null argument or no tensors");
  if (table_bytes < stgcn_adam_table_bytes(ntensors))
    return fail(STGCN_E_INVALID, "adam: table buffer too small");
  return fill_table("adam", tensors, ntensors, host_table, total_chunks,
                    [](int i, stgcn_adam_tensor_t &t) {
    if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq || t.numel <= 0)
      return fail(STGCN_E_INVALID,
                  "adam: tensor " + std::to_string(i) + " has a null pointer or numel <= 0");
    if ((((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg |
          (uintptr_t)t.exp_avg_sq) & 3) != 0)
      return fail(STGCN_E_INVALID,
                  "adam: tensor " + std::to_string(i) + ": param / grad / exp_avg / exp_avg_sq "
                  "must be 4-byte aligned");
    return (int)STGCN_OK;
  });
}

int stgcn_adam_step(const void *dev_table, int ntensors, int64_t total_chunks, double lr,
                    double beta1, double beta2, double eps, double weight_decay, int64_t step,
                    void *stream) {
  if (!dev_table || ntensors <= 0 || total_chunks <= 0 || step <= 0)
    return fail(STGCN_E_INVALID, "adam: bad table / chunk count / step");
  if (int rc = check_aligned({NP(dev_table)}, 8)) return rc;
  AdamArgs a = legacy_args(lr, beta1, beta2, eps, weight_decay);
  a.step = (double)step;
  launch_adam<stgcn_adam_tensor_t>(dev_table, ntensors, total_chunks, false, a, stream);
  HIP_TRY(hipGetLastError());
  return STGCN_OK;
}

int stgcn_adam_step_dev(const void *dev_table, int ntensors, int64_t total_chunks, double lr,
                        double beta1, double beta2, double eps, double weight_decay, float *step,
                        void *stream) {
  if (!dev_table || ntensors <= 0 || total_chunks <= 0 || !step)
    return fail(STGCN_E_INVALID, "adam: bad table / chunk count / step pointer");
  if (int rc = check_aligned({NP(dev_table)}, 8)) return rc;
  if (int rc = check_aligned({NP(step)}, 4)) return rc;
  AdamArgs a = legacy_args(lr, beta1, beta2, eps, weight_decay);
  a.step_dev = step;
  launch_adam<stgcn_adam_tensor_t>(dev_table, ntensors, total_chunks, false, a, stream);
  HIP_TRY(hipGetLastError());
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
  AdamArgs a = legacy_args(0.0, beta1, beta2, eps, weight_decay);
  a.step_dev = step;
  a.lr_dev = lr_dev;
  a.coef = grad_coef;
  launch_adam<stgcn_adam_tensor_t>(dev_table, ntensors, total_chunks, false, a, stream);
  HIP_TRY(hipGetLastError());
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
  hipLaunchKernelGGL(k_grad_sq, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream,
                     tab, chunk_starts<stgcn_adam_tensor_t>(dev_table, ntensors), ntensors,
                     partials);
  hipLaunchKernelGGL(k_grad_norm, dim3(1), dim3(256), 0, (hipStream_t)stream, partials,
                     total_chunks, (float)max_norm, norm_out, coef_out);
  HIP_TRY(hipGetLastError());
  return STGCN_OK;
}

int stgcn_opt_check(const stgcn_opt_desc_t *d) {
  if (!d) return fail(STGCN_E_INVALID, "opt: null descriptor");
  if (d->algo != STGCN_OPT_ADAM)
    return fail(STGCN_E_INVALID, "opt: unknown algo " + std::to_string(d->algo));
  const int known = STGCN_OPT_DECOUPLED_WD | STGCN_OPT_AMSGRAD;
  if (d->flags & ~known)
    return fail(STGCN_E_INVALID, "opt: unknown flags " + std::to_string(d->flags & ~known));
  // (!(x >= 0) also refuses a NaN)
  if (!d->lr_dev && !(d->lr >= 0.0)) return fail(STGCN_E_INVALID, "opt: lr must be >= 0");
  if (!(d->weight_decay >= 0.0)) return fail(STGCN_E_INVALID, "opt: weight_decay must be >= 0");
  if (!(d->beta1 >= 0.0 && d->beta1 < 1.0))
    return fail(STGCN_E_INVALID, "opt: beta1 must be in [0, 1)");
  if (!(d->beta2 >= 0.0 && d->beta2 < 1.0))
    return fail(STGCN_E_INVALID, "opt: beta2 must be in [0, 1)");
  if (!(d->eps >= 0.0)) return fail(STGCN_E_INVALID, "opt: eps must be >= 0");
  if (!d->step_dev && d->step < 1)
    return fail(STGCN_E_INVALID, "opt: step must be >= 1 (or step_dev given)");
  return check_aligned({NamedPtr{d->lr_dev, "lr_dev"}, NamedPtr{d->grad_coef, "grad_coef"},
                        NamedPtr{d->step_dev, "step_dev"}},
                       4);
}

size_t stgcn_opt_table_bytes(int ntensors) { return table_bytes<stgcn_opt_tensor_t>(ntensors); }

int stgcn_opt_build_table(const stgcn_opt_desc_t *d, const stgcn_opt_tensor_t *tensors,
                          int ntensors, void *host_table, size_t table_bytes,
                          int64_t *total_chunks) {
  if (int rc = stgcn_opt_check(d)) return rc;
  if (!tensors || ntensors <= 0 || !host_table || !total_chunks)
    return fail(STGCN_E_INVALID, "opt: null argument or no tensors");
  if (table_bytes < stgcn_opt_table_bytes(ntensors))
    return fail(STGCN_E_INVALID, "opt: table buffer too small");
  const bool need[3] = {true, true, (d->flags & STGCN_OPT_AMSGRAD) != 0};
  return fill_table("opt", tensors, ntensors, host_table, total_chunks,
                    [&need](int i, stgcn_opt_tensor_t &t) {
    const std::string who = "opt: tensor " + std::to_string(i);
    if (!t.param || !t.grad) return fail(STGCN_E_INVALID, who + ": param or grad is null");
    if (t.numel <= 0) return fail(STGCN_E_INVALID, who + ": numel <= 0");
    if (t.flags != 0) return fail(STGCN_E_INVALID, who + ": unknown tensor flags");
    const float *slots[3] = {t.s0, t.s1, t.s2};
    for (int k = 0; k < 3; ++k)
      if (need[k] && !slots[k])
        return fail(STGCN_E_INVALID, who + ": state slot s" + std::to_string(k) +
                                         " is null, and the algorithm needs it");
    if ((((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.s0 | (uintptr_t)t.s1 |
          (uintptr_t)t.s2) & 3) != 0)
      return fail(STGCN_E_INVALID, who + ": param / grad / s0 / s1 / s2 must be 4-byte aligned");
    t.reserved = 0;
    return (int)STGCN_OK;
  });
}

int stgcn_opt_step(const stgcn_opt_desc_t *d, const void *dev_table, int ntensors,
                   int64_t total_chunks, void *stream) {
  if (int rc = stgcn_opt_check(d)) return rc;
  if (!dev_table || ntensors <= 0 || total_chunks <= 0 || total_chunks > INT32_MAX)
    return fail(STGCN_E_INVALID, "opt: bad table / tensor count / chunk count");
  if (int rc = check_aligned({NP(dev_table)}, 8)) return rc;
  AdamArgs a{};
  a.lr = d->lr;
  a.beta1 = d->beta1;
  a.beta2 = d->beta2;
  a.eps = d->eps;
  a.wd = d->weight_decay;
  a.step = (double)d->step;
  a.step_dev = d->step_dev;
  a.lr_dev = d->lr_dev;
  a.coef = d->grad_coef;
  a.decoupled = (d->flags & STGCN_OPT_DECOUPLED_WD) != 0;
  launch_adam<stgcn_opt_tensor_t>(dev_table, ntensors, total_chunks,
                                  (d->flags & STGCN_OPT_AMSGRAD) != 0, a, stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(STGCN_E_HIP, std::string("opt: ") + hipGetErrorString(e));
  return STGCN_OK;
}

}  // extern "C"
