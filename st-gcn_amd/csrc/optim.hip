// STGCN_FEATURE_OPTIMIZERS (stgcn_opt_*): the Adam family with decoupled weight
// decay (torch.optim.AdamW) and AMSGrad, gfx950 only. One launch per table with
// train_ops.hip's chunking (k_adam: 2048 elements per 256-thread block, a binary
// search of the chunk prefix sums for the block's tensor). The
// arithmetic is stated in include/stgcn_hip.h and DESIGN.md §1; stgcn_adam_step
// and its kernels (train_ops.hip) are not touched by anything here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/stgcn_hip.h"

namespace stgcn {
void set_last_error(const std::string &msg);  // capi.hip (stgcn_last_error)
}

namespace {

int fail(int code, const std::string &m) {
  stgcn::set_last_error(m);
  return code;
}

int check_word(const void *p, const char *name, unsigned align) {
  if (((uintptr_t)p & (align - 1)) != 0)
    return fail(STGCN_E_INVALID,
                std::string(name) + ": must be " + std::to_string(align) + "-byte aligned");
  return STGCN_OK;
}

constexpr int kChunk = 2048;  // elements per block (256 threads x 8), as kAdamChunk

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

// ---------------------------------------------------------------------------
// Adam family: adam_block's arithmetic (train_ops.hip) with the decoupled decay
// ahead of the moment updates and the AMSGrad maximum. The scalars are formed
// from doubles and rounded to float, on the host for a host step count and a
// by-value lr, else by thread 0 of every block (the same expressions).
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

struct AdamArgs {
  AdamScalars host;  // used when neither step_dev nor lr_dev is given
  double lr, beta1, beta2, eps, wd, step;
  const float *step_dev, *lr_dev, *coef;
  int decoupled;
};

__global__ void k_opt_tick(float *step) { *step = *step + 1.f; }

template <bool AMS, bool COEF>
__global__ __launch_bounds__(256) void k_opt_adam(const stgcn_opt_tensor_t *tab,
                                                  const int64_t *chunk_start, int ntensors,
                                                  AdamArgs a) {
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
  const stgcn_opt_tensor_t t = tab[ti];
  const int64_t base = ((int64_t)blockIdx.x - chunk_start[ti]) * kChunk;
  for (int i = threadIdx.x; i < kChunk; i += 256) {
    const int64_t e = base + i;
    if (e >= t.numel) break;
    // (every operation rounded on its own, as in adam_block)
    float p = t.param[e];
    float g = t.grad[e];
    if constexpr (COEF) g = g * coef;
    if (s.wd != 0.f) g = g + s.wd * p;
    p = p * s.decay;  // (1 without decoupled decay: exact)
    float m = t.s0[e];
    m = m + s.lerp_w * (g - m);
    float v = t.s1[e] * s.beta2;
    v = v + (s.one_minus_beta2 * g) * g;
    float vd = v;
    if constexpr (AMS) {
      vd = fmaxf(t.s2[e], v);
      t.s2[e] = vd;
    }
    const float denom = sqrtf(vd) / s.bc2_sqrt + s.eps;
    p = p + s.neg_step_size * (m / denom);
    t.s0[e] = m;
    t.s1[e] = v;
    t.param[e] = p;
  }
}

const int64_t *chunk_starts(const void *dev_table, int ntensors) {
  return reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(dev_table) +
                                           (size_t)ntensors * sizeof(stgcn_opt_tensor_t));
}

int check_table_args(const void *dev_table, int ntensors, int64_t total_chunks) {
  if (!dev_table || ntensors <= 0 || total_chunks <= 0 || total_chunks > INT32_MAX)
    return fail(STGCN_E_INVALID, "opt: bad table / tensor count / chunk count");
  return check_word(dev_table, "dev_table", 8);
}

template <bool AMS>
void launch_adam(bool coef, unsigned grid, hipStream_t s, const stgcn_opt_tensor_t *tab,
                 const int64_t *cs, int ntensors, const AdamArgs &a) {
  if (coef)
    hipLaunchKernelGGL((k_opt_adam<AMS, true>), dim3(grid), dim3(256), 0, s, tab, cs, ntensors,
                       a);
  else
    hipLaunchKernelGGL((k_opt_adam<AMS, false>), dim3(grid), dim3(256), 0, s, tab, cs, ntensors,
                       a);
}

}  // namespace

extern "C" {

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
  if (int rc = check_word(d->lr_dev, "lr_dev", 4)) return rc;
  if (int rc = check_word(d->grad_coef, "grad_coef", 4)) return rc;
  if (int rc = check_word(d->step_dev, "step_dev", 4)) return rc;
  return STGCN_OK;
}

size_t stgcn_opt_table_bytes(int ntensors) {
  if (ntensors <= 0) return 0;
  return (size_t)ntensors * sizeof(stgcn_opt_tensor_t) + (size_t)(ntensors + 1) * sizeof(int64_t);
}

int stgcn_opt_build_table(const stgcn_opt_desc_t *d, const stgcn_opt_tensor_t *tensors,
                          int ntensors, void *host_table, size_t table_bytes,
                          int64_t *total_chunks) {
  if (int rc = stgcn_opt_check(d)) return rc;
  if (!tensors || ntensors <= 0 || !host_table || !total_chunks)
    return fail(STGCN_E_INVALID, "opt: null argument or no tensors");
  if (table_bytes < stgcn_opt_table_bytes(ntensors))
    return fail(STGCN_E_INVALID, "opt: table buffer too small");
  const bool need[3] = {true, true, (d->flags & STGCN_OPT_AMSGRAD) != 0};
  auto *tab = reinterpret_cast<stgcn_opt_tensor_t *>(host_table);
  auto *cs = reinterpret_cast<int64_t *>(reinterpret_cast<char *>(host_table) +
                                         (size_t)ntensors * sizeof(stgcn_opt_tensor_t));
  int64_t chunks = 0;
  for (int i = 0; i < ntensors; ++i) {
    const stgcn_opt_tensor_t &t = tensors[i];
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
    tab[i] = t;
    tab[i].reserved = 0;
    cs[i] = chunks;
    chunks += (t.numel + kChunk - 1) / kChunk;
  }
  cs[ntensors] = chunks;
  if (chunks > INT32_MAX) return fail(STGCN_E_UNSUPPORTED, "opt: too many elements");
  *total_chunks = chunks;
  return STGCN_OK;
}

int stgcn_opt_step(const stgcn_opt_desc_t *d, const void *dev_table, int ntensors,
                   int64_t total_chunks, void *stream) {
  if (int rc = stgcn_opt_check(d)) return rc;
  if (int rc = check_table_args(dev_table, ntensors, total_chunks)) return rc;
  const auto *tab = reinterpret_cast<const stgcn_opt_tensor_t *>(dev_table);
  const int64_t *cs = chunk_starts(dev_table, ntensors);
  const unsigned grid = (unsigned)total_chunks;
  hipStream_t s = (hipStream_t)stream;
  const bool coef = d->grad_coef != nullptr;
  const bool decoupled = (d->flags & STGCN_OPT_DECOUPLED_WD) != 0;
  AdamArgs a;
  a.lr = d->lr;
  a.beta1 = d->beta1;
  a.beta2 = d->beta2;
  a.eps = d->eps;
  a.wd = d->weight_decay;
  a.step = (double)d->step;
  a.step_dev = d->step_dev;
  a.lr_dev = d->lr_dev;
  a.coef = d->grad_coef;
  a.decoupled = decoupled;
  std::memset(&a.host, 0, sizeof(a.host));
  if (!d->step_dev && !d->lr_dev)
    a.host = adam_scalars(a.step, a.lr, a.beta1, a.beta2, a.eps, a.wd, decoupled);
  if (d->step_dev) hipLaunchKernelGGL(k_opt_tick, dim3(1), dim3(1), 0, s, d->step_dev);
  if (d->flags & STGCN_OPT_AMSGRAD)
    launch_adam<true>(coef, grid, s, tab, cs, ntensors, a);
  else
    launch_adam<false>(coef, grid, s, tab, cs, ntensors, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(STGCN_E_HIP, std::string("opt: ") + hipGetErrorString(e));
  return STGCN_OK;
}

}  // extern "C"
