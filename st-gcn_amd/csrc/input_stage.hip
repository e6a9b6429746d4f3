// Input stage (STGCN_FEATURE_INPUT_STAGE): ragged skeleton clips, packed frame
// after frame in the .npy layout (T, V, C_src), to the network input
// x (N, C, T_out, V) fp32 in ONE memory-bound kernel: the loop padding of
// src/data/util.py:12-30 (np.pad "wrap" == frame t mod T_i), the per-clip 2x2
// part of the augmentation matrix (src/data/augmentation.py:8-69, evaluated in
// fp64 like numpy, rounded once to fp32), the fp32 cast and the NTVC -> NCTV
// transpose of lightning_model.py:101.
//
// One thread per output point (n, t, v): it loads the point's C_src source
// values in one access (they are adjacent) and stores one value to each of the
// C output planes; consecutive lanes hold consecutive (t, v), so every plane
// store is a coalesced 256-byte row per wave and needs no alignment beyond the
// element's. Algorithmic bytes: N * T_out * V * (C_src * sizeof(src) + 4 * C).
// The clip table is read by every workgroup of a clip (uniform loads) when the
// kernel RUNS, so a captured launch sees the table of each replay; an entry
// that does not lie inside [0, src_frames) zero-fills its clip, flags it in
// status[] and reads nothing of src.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/stgcn_hip.h"
#include "host_common.h"

namespace {

constexpr int kStageThreads = 256;

using stgcn::check_aligned;
using stgcn::fail;

// One source point: CS adjacent elements at the element's own alignment (the
// load is one dwordx2 / x3 / x4: global loads need dword alignment only).
template <typename S, int CS>
struct alignas(alignof(S)) Point {
  S c[CS];
};

// grid: N * bpc workgroups, bpc = ceil(T_out * V / kStageThreads); workgroup b
// serves points [chunk * kStageThreads, ...) of clip n = b / bpc.
template <typename S, int CS>
__global__ void __launch_bounds__(kStageThreads)
k_input_stage(const S *__restrict__ src, const stgcn_clip_t *__restrict__ clips,
              float *__restrict__ x, int32_t *__restrict__ status, int C, int T_out, int V,
              int bpc, int64_t src_frames) {
  const int n = (int)(blockIdx.x / (unsigned)bpc);
  const int chunk = (int)(blockIdx.x - (unsigned)n * (unsigned)bpc);
  const int plane = T_out * V;  // < 2^31 (stgcn_input_check)
  // (int64: the last workgroup's indices may pass 2^31 when plane is close to it)
  const int64_t p64 = (int64_t)chunk * kStageThreads + (int64_t)threadIdx.x;
  const stgcn_clip_t clip = clips[n];
  // (frames >= 1 and src_frames >= 1: the difference cannot overflow)
  const bool ok = clip.frames >= 1 && clip.first_frame >= 0 &&
                  clip.first_frame <= src_frames - (int64_t)clip.frames;
  if (chunk == 0 && threadIdx.x == 0) status[n] = ok ? 0 : 1;
  if (p64 >= plane) return;
  const int p = (int)p64;
  float *out = x + (int64_t)n * C * plane + p;
  if (!ok) {
    for (int c = 0; c < C; ++c) out[(int64_t)c * plane] = 0.f;
    return;
  }
  const int t = p / V, v = p - t * V;
  const int64_t frame = clip.first_frame + (int64_t)((unsigned)t % (unsigned)clip.frames);
  const Point<S, CS> pt =
      *reinterpret_cast<const Point<S, CS> *>(src + (frame * V + v) * (int64_t)CS);
  if (clip.flags & 1) {
    // out_j = x m[0][j] + y m[1][j]: two products and one sum, each rounded to
    // fp64 (no fused multiply-add: numpy's arithmetic), then one rounding to fp32
    const double px = (double)pt.c[0], py = (double)pt.c[1];
    out[0] = (float)__dadd_rn(__dmul_rn(px, clip.m[0]), __dmul_rn(py, clip.m[2]));
    out[plane] = (float)__dadd_rn(__dmul_rn(px, clip.m[1]), __dmul_rn(py, clip.m[3]));
  } else {
    out[0] = (float)pt.c[0];
    out[plane] = (float)pt.c[1];
  }
#pragma unroll
  for (int c = 2; c < CS; ++c)
    if (c < C) out[(int64_t)c * plane] = (float)pt.c[c];
}

template <typename S>
void launch_stage(const stgcn_input_desc_t *d, const void *src, const stgcn_clip_t *clips,
                  float *x, int32_t *status, int bpc, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)d->N * bpc)), block(kStageThreads);
  const S *sp = (const S *)src;
#define STAGE_CASE(CS)                                                                        \
  case CS:                                                                                    \
    hipLaunchKernelGGL((k_input_stage<S, CS>), grid, block, 0, s, sp, clips, x, status, d->C, \
                       d->T_out, d->V, bpc, d->src_frames);                                   \
    break;
  switch (d->C_src) {
    STAGE_CASE(2)
    STAGE_CASE(3)
    STAGE_CASE(4)
  }
#undef STAGE_CASE
}

int blocks_per_clip(const stgcn_input_desc_t *d) {
  return (int)(((int64_t)d->T_out * d->V + kStageThreads - 1) / kStageThreads);
}

}  // namespace

static_assert(sizeof(stgcn_input_desc_t) == 32, "stgcn_input_desc_t is 32 bytes");
static_assert(sizeof(stgcn_clip_t) == 48, "stgcn_clip_t is 48 bytes");

extern "C" {

int stgcn_input_check(const stgcn_input_desc_t *d) {
  if (!d) return fail(STGCN_E_INVALID, "input: null descriptor");
  if (d->N <= 0) return fail(STGCN_E_INVALID, "input: N must be positive");
  if (d->T_out <= 0) return fail(STGCN_E_INVALID, "input: T_out must be positive");
  if (d->V <= 0) return fail(STGCN_E_INVALID, "input: V must be positive");
  if (d->C_src > 4) return fail(STGCN_E_INVALID, "input: C_src must be at most 4");
  if (d->C < 2) return fail(STGCN_E_INVALID, "input: C must be at least 2 (x, y)");
  if (d->C > d->C_src) return fail(STGCN_E_INVALID, "input: C must not exceed C_src");
  if (d->src_f64 != 0 && d->src_f64 != 1)
    return fail(STGCN_E_INVALID, "input: src_f64 must be 0 (fp32) or 1 (fp64)");
  if (d->src_frames <= 0) return fail(STGCN_E_INVALID, "input: src_frames must be positive");
  if ((int64_t)d->T_out * d->V > INT32_MAX)
    return fail(STGCN_E_UNSUPPORTED, "input: T_out * V exceeds 2^31 - 1");
  if ((int64_t)d->N * blocks_per_clip(d) > INT32_MAX)
    return fail(STGCN_E_UNSUPPORTED, "input: N * T_out * V too large for one launch");
  return STGCN_OK;
}

int stgcn_input_stage(const stgcn_input_desc_t *d, const void *src, const stgcn_clip_t *clips,
                      float *x, int32_t *status, void *stream) {
  if (int rc = stgcn_input_check(d)) return rc;
  if (!src || !clips || !x || !status)
    return fail(STGCN_E_INVALID, "input: null argument (src, clips, x, status)");
  if (int rc = check_aligned({NP(x)}, 16)) return rc;
  if (int rc = check_aligned({NP(src)}, d->src_f64 ? 8 : 4)) return rc;
  if (int rc = check_aligned({NP(clips)}, 8)) return rc;
  if (int rc = check_aligned({NP(status)}, 4)) return rc;
  const int bpc = blocks_per_clip(d);
  if (d->src_f64)
    launch_stage<double>(d, src, clips, x, status, bpc, (hipStream_t)stream);
  else
    launch_stage<float>(d, src, clips, x, status, bpc, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return fail(STGCN_E_HIP, std::string("input_stage launch: ") + hipGetErrorString(e));
  return STGCN_OK;
}

}  // extern "C"
