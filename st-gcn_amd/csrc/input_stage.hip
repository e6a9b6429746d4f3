// Input stage (STGCN_FEATURE_INPUT_STAGE): ragged skeleton clips, packed frame
// after frame in the .npy layout (T, V, C_src), to the network input
// x (N, C, T_out, V) fp32 in ONE memory-bound kernel: the loop padding of
// src/data/util.py:12-30 (np.pad "wrap" == frame t mod T_i), the per-clip 2x2
// part of the augmentation matrix (src/data/augmentation.py:8-69, evaluated in
// fp64, rounded once to fp32), the fp32 cast and the NTVC -> NCTV
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
//
// STGCN_FEATURE_INPUT_MOVE (k_input_stage_move, below): the same launch with one
// stgcn_move_t per clip -- rotation, scale and translation interpolated over the
// frames and applied per frame ("random moving"), validated in the kernel too.
//
// STGCN_FEATURE_INPUT_STREAMS (k_input_stage_streams): the same launch writing
// S of the four input streams of the ST-GCN descendants -- joint, bone (joint
// minus parent joint), joint motion (frame t + 1 minus frame t), bone motion --
// as S groups of C channels, formed from the augmented point in registers.
// Algorithmic bytes: N * T_out * V * (C_src * sizeof(src) + 4 * S * C).
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
    // out_j = x m[0][j] + y m[1][j] in fp64, then one rounding to fp32. As compiled
    // this is one product and one fused multiply-add, fma(x, m[0][j], y m[1][j]):
    // __dmul_rn / __dadd_rn are plain operators under the default contraction
    // (see store_point below, which writes that form out and must keep matching)
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

// ---- STGCN_FEATURE_INPUT_MOVE ------------------------------------------------

// From here on every fp64 operation is rounded on its own: the move's arithmetic
// is numpy's, operation by operation (data.apply_moves_reference). Plain
// operators, not __dmul_rn / __dadd_rn: those are header functions compiled in the
// default mode, whose product and sum the compiler would fuse again.
#pragma clang fp contract(off)

// k_input_stage's work on one point of a valid clip, for a clip without a move,
// with its bits. HIP's __dmul_rn / __dadd_rn are header functions over plain
// operators, and under the compiler's default contraction k_input_stage's
// transform is one product and one fused multiply-add in all six instances,
// out_j = fma(x, m[0][j], y m[1][j]) (v_mul_f64 + v_fmac_f64 in its code objects),
// not two products and a sum. That is what it has always computed and it is
// kept; it is written out here, so that this kernel does not depend on the
// compiler fusing the same pair again. The nk = 0 bit-equality does depend on
// the compiler still fusing that pair in k_input_stage itself, whose text is left
// alone so that its code objects stay the parent's; tests/test_gpu_input_move.py
// (test_no_move_has_the_plain_stage_bits) fails if a compiler ever stops.
template <typename S, int CS>
__device__ __forceinline__ void store_point(const Point<S, CS> &pt, const stgcn_clip_t &clip,
                                            float *out, int plane, int C) {
  if (clip.flags & 1) {
    const double px = (double)pt.c[0], py = (double)pt.c[1];
    out[0] = (float)__builtin_fma(px, clip.m[0], py * clip.m[2]);
    out[plane] = (float)__builtin_fma(px, clip.m[1], py * clip.m[3]);
  } else {
    out[0] = (float)pt.c[0];
    out[plane] = (float)pt.c[1];
  }
#pragma unroll
  for (int c = 2; c < CS; ++c)
    if (c < C) out[(int64_t)c * plane] = (float)pt.c[c];
}

// nk = 0, or 2..4 key frames from 0, strictly increasing, the last at T_out - 1
// or later, and finite parameters (uniform per workgroup)
__device__ __forceinline__ bool move_ok(const stgcn_move_t &mv, int T_out) {
  if (mv.nk == 0) return true;
  if (mv.nk < 2 || mv.nk > 4 || mv.frame[0] != 0) return false;
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < mv.nk) {
      if (i > 0) ok = ok && mv.frame[i] > mv.frame[i - 1];
      ok = ok && isfinite(mv.angle[i]) && isfinite(mv.scale[i]) && isfinite(mv.tx[i]) &&
           isfinite(mv.ty[i]);
    }
  // (constant indices only: an indexed access would put the record in scratch)
  const int last = mv.nk == 2 ? mv.frame[1] : mv.nk == 3 ? mv.frame[2] : mv.frame[3];
  return ok && last >= T_out - 1;
}

// p(t) = p_k + (t - f_k) * ((p_k1 - p_k) / (f_k1 - f_k)): np.linspace's start +
// i * step, every operation rounded on its own
__device__ __forceinline__ double lerp_key(double pk, double pk1, double i, double span) {
  return pk + i * ((pk1 - pk) / span);
}

struct Affine {
  double c, sn, tx, ty;
};

// frame t of a valid record with nk >= 2: its segment by selects (the record
// sits in scalar registers: no indexed access), the four parameters, then
// c = cos(a) * s, sn = sin(a) * s
__device__ __forceinline__ Affine frame_affine(const stgcn_move_t &mv, int t) {
  const bool s1 = mv.nk > 2 && t >= mv.frame[1], s2 = mv.nk > 3 && t >= mv.frame[2];
#define MOVE_SEL(a) (s2 ? a[2] : s1 ? a[1] : a[0])
#define MOVE_SEL1(a) (s2 ? a[3] : s1 ? a[2] : a[1])
  const int f0 = MOVE_SEL(mv.frame), f1 = MOVE_SEL1(mv.frame);
  const double i = (double)(t - f0), span = (double)(f1 - f0);
  const double a = lerp_key(MOVE_SEL(mv.angle), MOVE_SEL1(mv.angle), i, span);
  const double s = lerp_key(MOVE_SEL(mv.scale), MOVE_SEL1(mv.scale), i, span);
  Affine r;
  r.tx = lerp_key(MOVE_SEL(mv.tx), MOVE_SEL1(mv.tx), i, span);
  r.ty = lerp_key(MOVE_SEL(mv.ty), MOVE_SEL1(mv.ty), i, span);
#undef MOVE_SEL
#undef MOVE_SEL1
  r.c = cos(a) * s;
  r.sn = sin(a) * s;
  return r;
}

// k_input_stage with one stgcn_move_t per clip: same grid, same point per
// thread, same stores. A workgroup's 256 points lie in at most 255 / V + 2
// frames; their (c, sn, tx, ty) are evaluated once, by the first threads, into
// LDS (kMoveFrames covers V = 1), and every thread reads its frame's four
// doubles from there.
constexpr int kMoveFrames = kStageThreads + 1;

template <typename S, int CS>
__global__ void __launch_bounds__(kStageThreads)
k_input_stage_move(const S *__restrict__ src, const stgcn_clip_t *__restrict__ clips,
                   const stgcn_move_t *__restrict__ moves, float *__restrict__ x,
                   int32_t *__restrict__ status, int C, int T_out, int V, int bpc,
                   int64_t src_frames) {
  __shared__ Affine frames[kMoveFrames];
  const int n = (int)(blockIdx.x / (unsigned)bpc);
  const int chunk = (int)(blockIdx.x - (unsigned)n * (unsigned)bpc);
  const int plane = T_out * V;  // < 2^31 (stgcn_input_check)
  const int64_t p64 = (int64_t)chunk * kStageThreads + (int64_t)threadIdx.x;
  const stgcn_clip_t clip = clips[n];
  const stgcn_move_t &mv = moves[n];  // (fields are loaded where used: uniform loads)
  const bool clip_ok = clip.frames >= 1 && clip.first_frame >= 0 &&
                       clip.first_frame <= src_frames - (int64_t)clip.frames;
  const bool mv_ok = move_ok(mv, T_out);
  if (chunk == 0 && threadIdx.x == 0) status[n] = (clip_ok ? 0 : 1) | (mv_ok ? 0 : 2);
  const bool live = p64 < plane;
  const int p = live ? (int)p64 : 0;
  float *out = x + (int64_t)n * C * plane + p;
  if (!clip_ok || !mv_ok) {  // (uniform)
    if (live)
      for (int c = 0; c < C; ++c) out[(int64_t)c * plane] = 0.f;
    return;
  }
  // the point's source values first: the load is in flight while the frames'
  // parameters are evaluated
  const int t = p / V, v = p - t * V;
  Point<S, CS> pt = {};
  if (live) {
    const int64_t frame = clip.first_frame + (int64_t)((unsigned)t % (unsigned)clip.frames);
    pt = *reinterpret_cast<const Point<S, CS> *>(src + (frame * V + v) * (int64_t)CS);
  }
  if (mv.nk == 0) {  // (uniform) no move: k_input_stage's bits
    if (live) store_point<S, CS>(pt, clip, out, plane, C);
    return;
  }
  // the workgroup's first point is in range (bpc = ceil(plane / 256)); frames
  // t0 .. t0 + (255 / V + 1), cut at the plane's end. Every thread of the
  // workgroup reaches the barrier: the returns above are uniform.
  const int t0 = (int)(((int64_t)chunk * kStageThreads) / V);
  const int tf = t0 + (int)threadIdx.x;
  if ((int)threadIdx.x <= (kStageThreads - 1) / V + 1 && tf < T_out)
    frames[threadIdx.x] = frame_affine(mv, tf);
  __syncthreads();
  if (!live) return;
  const Affine f = frames[t - t0];
  double px = (double)pt.c[0], py = (double)pt.c[1];
  if (clip.flags & 1) {  // the clip's matrix first (two products, one sum), kept in fp64
    const double qx = px * clip.m[0] + py * clip.m[2];
    py = px * clip.m[1] + py * clip.m[3];
    px = qx;
  }
  // x' = (c x - sn y) + tx, y' = (sn x + c y) + ty, one rounding to fp32
  out[0] = (float)((f.c * px - f.sn * py) + f.tx);
  out[plane] = (float)((f.sn * px + f.c * py) + f.ty);
#pragma unroll
  for (int c = 2; c < CS; ++c)
    if (c < C) out[(int64_t)c * plane] = (float)pt.c[c];
}

// ---- STGCN_FEATURE_INPUT_STREAMS ---------------------------------------------

// J[.., t, v] of a valid clip from one source point, with the bits of the launch
// it restates: k_input_stage_move's unfused fp64 sequence on a moved clip (f is
// the frame's entry of the LDS table), store_point's fused form or plain cast
// otherwise. moved is uniform per workgroup.
template <typename S, int CS>
__device__ __forceinline__ void joint_point(const Point<S, CS> &pt, const stgcn_clip_t &clip,
                                            bool moved, const Affine &f, float (&j)[CS]) {
  double px = (double)pt.c[0], py = (double)pt.c[1];
  if (moved) {
    if (clip.flags & 1) {
      const double qx = px * clip.m[0] + py * clip.m[2];
      py = px * clip.m[1] + py * clip.m[3];
      px = qx;
    }
    j[0] = (float)((f.c * px - f.sn * py) + f.tx);
    j[1] = (float)((f.sn * px + f.c * py) + f.ty);
  } else if (clip.flags & 1) {
    j[0] = (float)__builtin_fma(px, clip.m[0], py * clip.m[2]);
    j[1] = (float)__builtin_fma(px, clip.m[1], py * clip.m[3]);
  } else {
    j[0] = (float)pt.c[0];
    j[1] = (float)pt.c[1];
  }
#pragma unroll
  for (int c = 2; c < CS; ++c) j[c] = (float)pt.c[c];
}

// One stream's C plane rows of a point: the difference b - a, or on the score
// channel the mean (b + a) * 0.5f; fp32, every operation rounded on its own.
__device__ __forceinline__ float stream_op(float b, float a, bool score) {
  return score ? (b + a) * 0.5f : b - a;
}

// The joint, bone, joint-motion and bone-motion streams of the staged input
// (streams: a non-empty mask of STGCN_STREAM_*, uniform), S = popcount(streams)
// groups of C channels in bit order: x (N, S * C, T_out, V). Same grid and same
// point per thread as the kernels above. A thread gathers up to four source
// points, (t, v), (t, p), (t + 1, v), (t + 1, p) with p = parents[v], forms J
// at each by joint_point and stores S * C coalesced plane rows; the last frame of
// the motion streams is 0. Frame t + 1 is the loop-padded one, as for frame t.
// Algorithmic bytes: N * T_out * V * (C_src * sizeof(src) + 4 * S * C) (the
// neighbour points are other threads' own points: cache hits).
// LDS: the parents table (V <= 256 with a bone bit, stgcn_input_streams_check),
// loaded by the workgroup and validated with one __syncthreads_or, and the
// frames' affine parameters of a moved clip, now up to frame t + 1: for V = 1
// the workgroup's 256 points and their successors lie in 257 frames; the general
// bound 255 / V + 3 gives 258.
constexpr int kStreamFrames = kMoveFrames + 1;
constexpr int kMaxParents = 256;  // (the block library's own limit on V)
constexpr int kAllStreams = STGCN_STREAM_JOINT | STGCN_STREAM_BONE | STGCN_STREAM_JOINT_MOTION |
                            STGCN_STREAM_BONE_MOTION;

template <typename S, int CS>
__global__ void __launch_bounds__(kStageThreads)
k_input_stage_streams(const S *__restrict__ src, const stgcn_clip_t *__restrict__ clips,
                      const stgcn_move_t *__restrict__ moves,
                      const int32_t *__restrict__ parents, float *__restrict__ x,
                      int32_t *__restrict__ status, int C, int T_out, int V, int bpc,
                      int64_t src_frames, int streams, int score_channel) {
  __shared__ Affine frames[kStreamFrames];
  __shared__ int32_t par[kMaxParents];
  const int n = (int)(blockIdx.x / (unsigned)bpc);
  const int chunk = (int)(blockIdx.x - (unsigned)n * (unsigned)bpc);
  const int plane = T_out * V;  // < 2^31 (stgcn_input_check)
  const int64_t p64 = (int64_t)chunk * kStageThreads + (int64_t)threadIdx.x;
  const stgcn_clip_t clip = clips[n];
  const stgcn_move_t *mv = moves ? moves + n : nullptr;  // (fields are loaded where used)
  const bool clip_ok = clip.frames >= 1 && clip.first_frame >= 0 &&
                       clip.first_frame <= src_frames - (int64_t)clip.frames;
  const bool mv_ok = mv ? move_ok(*mv, T_out) : true;
  const bool bone = (streams & (STGCN_STREAM_BONE | STGCN_STREAM_BONE_MOTION)) != 0;
  const bool motion = (streams & (STGCN_STREAM_JOINT_MOTION | STGCN_STREAM_BONE_MOTION)) != 0;
  int par_bad = 0;
  if (bone) {  // (uniform; V <= kMaxParents) the barrier also publishes par[]
    int bad = 0;
    if ((int)threadIdx.x < V) {
      const int32_t q = parents[threadIdx.x];
      par[threadIdx.x] = q;
      bad = q < 0 || q >= V;
    }
    par_bad = __syncthreads_or(bad);
  }
  if (chunk == 0 && threadIdx.x == 0)
    status[n] = (clip_ok ? 0 : 1) | (mv_ok ? 0 : 2) | (par_bad ? 4 : 0);
  const bool live = p64 < plane;
  const int p = live ? (int)p64 : 0;
  const int SC = __popc((unsigned)streams) * C;
  float *out = x + (int64_t)n * SC * plane + p;
  if (!clip_ok || !mv_ok || par_bad) {  // (uniform)
    if (live)
      for (int c = 0; c < SC; ++c) out[(int64_t)c * plane] = 0.f;
    return;
  }
  // the source points first: the loads are in flight while the frames'
  // parameters are evaluated
  const int t = p / V, v = p - t * V;
  const bool next = motion && t + 1 < T_out;  // (the last frame's motion is 0)
  const int q = bone ? par[v] : v;
  Point<S, CS> pv = {}, pq = {}, nv = {}, nq = {};
  if (live) {
    const int64_t f0 = clip.first_frame + (int64_t)((unsigned)t % (unsigned)clip.frames);
    pv = *reinterpret_cast<const Point<S, CS> *>(src + (f0 * V + v) * (int64_t)CS);
    if (bone) pq = *reinterpret_cast<const Point<S, CS> *>(src + (f0 * V + q) * (int64_t)CS);
    if (next) {
      const int64_t f1 =
          clip.first_frame + (int64_t)((unsigned)(t + 1) % (unsigned)clip.frames);
      nv = *reinterpret_cast<const Point<S, CS> *>(src + (f1 * V + v) * (int64_t)CS);
      if (bone) nq = *reinterpret_cast<const Point<S, CS> *>(src + (f1 * V + q) * (int64_t)CS);
    }
  }
  const bool moved = mv && mv->nk != 0;  // (uniform)
  const int t0 = (int)(((int64_t)chunk * kStageThreads) / V);
  if (moved) {
    // frames t0 .. t0 + (255 / V + 2), cut at the plane's end: those of the
    // workgroup's points and of their successors. Every thread of the workgroup
    // reaches the barrier: the returns above are uniform.
    const int nf = min((kStageThreads - 1) / V + 3, T_out - t0);
    for (int i = (int)threadIdx.x; i < nf; i += kStageThreads)
      frames[i] = frame_affine(*mv, t0 + i);
    __syncthreads();
  }
  if (!live) return;
  Affine fa = {}, fb = {};
  if (moved) {
    fa = frames[t - t0];
    if (next) fb = frames[t + 1 - t0];
  }
  float jv[CS], jq[CS] = {}, kv[CS] = {}, kq[CS] = {};
  joint_point<S, CS>(pv, clip, moved, fa, jv);
  if (bone) joint_point<S, CS>(pq, clip, moved, fa, jq);
  if (next) {
    joint_point<S, CS>(nv, clip, moved, fb, kv);
    if (bone) joint_point<S, CS>(nq, clip, moved, fb, kq);
  }
  const int64_t group = (int64_t)C * plane;
  if (streams & STGCN_STREAM_JOINT) {
#pragma unroll
    for (int c = 0; c < CS; ++c)
      if (c < C) out[(int64_t)c * plane] = jv[c];
    out += group;
  }
  if (streams & STGCN_STREAM_BONE) {
#pragma unroll
    for (int c = 0; c < CS; ++c)
      if (c < C) out[(int64_t)c * plane] = stream_op(jv[c], jq[c], c == score_channel);
    out += group;
  }
  if (streams & STGCN_STREAM_JOINT_MOTION) {
#pragma unroll
    for (int c = 0; c < CS; ++c)
      if (c < C)
        out[(int64_t)c * plane] = next ? stream_op(kv[c], jv[c], c == score_channel) : 0.f;
    out += group;
  }
  if (streams & STGCN_STREAM_BONE_MOTION) {
#pragma unroll
    for (int c = 0; c < CS; ++c)
      if (c < C) {
        const bool sc = c == score_channel;
        out[(int64_t)c * plane] =
            next ? stream_op(stream_op(kv[c], kq[c], sc), stream_op(jv[c], jq[c], sc), sc) : 0.f;
      }
  }
}

template <typename S>
void launch_streams(const stgcn_streams_desc_t *sd, const void *src, const stgcn_clip_t *clips,
                    const stgcn_move_t *moves, const int32_t *parents, float *x,
                    int32_t *status, int bpc, hipStream_t s) {
  const stgcn_input_desc_t *d = &sd->in;
  const dim3 grid((unsigned)((int64_t)d->N * bpc)), block(kStageThreads);
  const S *sp = (const S *)src;
#define STREAMS_CASE(CS)                                                                        \
  case CS:                                                                                      \
    hipLaunchKernelGGL((k_input_stage_streams<S, CS>), grid, block, 0, s, sp, clips, moves,     \
                       parents, x, status, d->C, d->T_out, d->V, bpc, d->src_frames,            \
                       sd->streams, sd->score_channel);                                         \
    break;
  switch (d->C_src) {
    STREAMS_CASE(2)
    STREAMS_CASE(3)
    STREAMS_CASE(4)
  }
#undef STREAMS_CASE
}

template <typename S>
void launch_stage(const stgcn_input_desc_t *d, const void *src, const stgcn_clip_t *clips,
                  const stgcn_move_t *moves, float *x, int32_t *status, int bpc, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)d->N * bpc)), block(kStageThreads);
  const S *sp = (const S *)src;
#define STAGE_CASE(CS)                                                                          \
  case CS:                                                                                      \
    if (moves)                                                                                  \
      hipLaunchKernelGGL((k_input_stage_move<S, CS>), grid, block, 0, s, sp, clips, moves, x,   \
                         status, d->C, d->T_out, d->V, bpc, d->src_frames);                     \
    else                                                                                        \
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
static_assert(sizeof(stgcn_move_t) == 160, "stgcn_move_t is 160 bytes");
static_assert(sizeof(stgcn_streams_desc_t) == 40, "stgcn_streams_desc_t is 40 bytes");

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

int stgcn_input_move_check(const stgcn_input_desc_t *d) { return stgcn_input_check(d); }

int stgcn_input_stage(const stgcn_input_desc_t *d, const void *src, const stgcn_clip_t *clips,
                      float *x, int32_t *status, void *stream) {
  return stgcn_input_stage_move(d, src, clips, nullptr, x, status, stream);
}

int stgcn_input_stage_move(const stgcn_input_desc_t *d, const void *src,
                           const stgcn_clip_t *clips, const stgcn_move_t *moves, float *x,
                           int32_t *status, void *stream) {
  if (int rc = stgcn_input_check(d)) return rc;
  if (!src || !clips || !x || !status)
    return fail(STGCN_E_INVALID, "input: null argument (src, clips, x, status)");
  if (int rc = check_aligned({NP(x)}, 16)) return rc;
  if (int rc = check_aligned({NP(src)}, d->src_f64 ? 8 : 4)) return rc;
  if (int rc = check_aligned({NP(clips)}, 8)) return rc;
  if (int rc = check_aligned({NP(status)}, 4)) return rc;
  if (int rc = check_aligned({NP(moves)}, 8)) return rc;  // (null passes)
  const int bpc = blocks_per_clip(d);
  if (d->src_f64)
    launch_stage<double>(d, src, clips, moves, x, status, bpc, (hipStream_t)stream);
  else
    launch_stage<float>(d, src, clips, moves, x, status, bpc, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return fail(STGCN_E_HIP, std::string("input_stage launch: ") + hipGetErrorString(e));
  return STGCN_OK;
}

int stgcn_input_streams_check(const stgcn_streams_desc_t *d) {
  if (!d) return fail(STGCN_E_INVALID, "streams: null descriptor");
  if (int rc = stgcn_input_check(&d->in)) return rc;
  if (d->streams <= 0 || (d->streams & ~kAllStreams))
    return fail(STGCN_E_INVALID,
                "streams: the mask is a non-empty subset of the four STGCN_STREAM_* bits");
  if (d->score_channel != -1 && (d->score_channel != d->in.C - 1 || d->score_channel < 2))
    return fail(STGCN_E_INVALID, "streams: score_channel is -1 or in.C - 1 (at least 2)");
  if ((d->streams & (STGCN_STREAM_BONE | STGCN_STREAM_BONE_MOTION)) && d->in.V > kMaxParents)
    return fail(STGCN_E_UNSUPPORTED, "streams: a bone stream needs V <= 256");
  // x (N, S * C, T_out, V) is indexed with int64 element offsets. Today the launch
  // limit of stgcn_input_check (N * T_out * V < 2^39, and S * C <= 16) keeps it far
  // inside them; the check stands on its own should that limit ever be relaxed.
  const int64_t rows = (int64_t)d->in.N * __builtin_popcount((unsigned)d->streams) * d->in.C;
  if (rows > INT64_MAX / 4 / ((int64_t)d->in.T_out * d->in.V))
    return fail(STGCN_E_UNSUPPORTED, "streams: N * S * C * T_out * V exceeds the int64 offsets");
  return STGCN_OK;
}

int stgcn_input_stage_streams(const stgcn_streams_desc_t *d, const void *src,
                              const stgcn_clip_t *clips, const stgcn_move_t *moves,
                              const int32_t *parents, float *x, int32_t *status, void *stream) {
  if (int rc = stgcn_input_streams_check(d)) return rc;
  const bool bone = (d->streams & (STGCN_STREAM_BONE | STGCN_STREAM_BONE_MOTION)) != 0;
  if (bone && !parents)
    return fail(STGCN_E_INVALID, "streams: null parents with a bone stream");
  if (d->streams == STGCN_STREAM_JOINT)  // (J does not depend on score_channel)
    return stgcn_input_stage_move(&d->in, src, clips, moves, x, status, stream);
  if (!src || !clips || !x || !status)
    return fail(STGCN_E_INVALID, "streams: null argument (src, clips, x, status)");
  if (int rc = check_aligned({NP(x)}, 16)) return rc;
  if (int rc = check_aligned({NP(src)}, d->in.src_f64 ? 8 : 4)) return rc;
  if (int rc = check_aligned({NP(clips)}, 8)) return rc;
  if (int rc = check_aligned({NP(status)}, 4)) return rc;
  if (int rc = check_aligned({NP(moves)}, 8)) return rc;  // (null passes)
  if (bone)
    if (int rc = check_aligned({NP(parents)}, 4)) return rc;
  const int bpc = blocks_per_clip(&d->in);
  if (d->in.src_f64)
    launch_streams<double>(d, src, clips, moves, bone ? parents : nullptr, x, status, bpc,
                           (hipStream_t)stream);
  else
    launch_streams<float>(d, src, clips, moves, bone ? parents : nullptr, x, status, bpc,
                          (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return fail(STGCN_E_HIP, std::string("input_stage_streams launch: ") + hipGetErrorString(e));
  return STGCN_OK;
}

}  // extern "C"
