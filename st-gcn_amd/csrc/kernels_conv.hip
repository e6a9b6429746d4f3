// fp32 convolution GEMMs and weight gradients of libstgcn_hip.so — gfx950
// (MI355X / CDNA4) only.
//
// The (9,1) temporal convolution forward / data-grad (k_conv_gemm, k_tconv) and
// the weight gradients (k_wgrad, k_wgrad_taps, k_wgrad_sp with its split-K
// reduction k_slab_reduce) on the exact-fp32 matrix cores
// (v_mfma_f32_32x32x2_f32: one fmaf chain per output, no reduced precision);
// k_wgrad_sp<.., X3> forms its products as exact 3-way bf16 splits instead
// (kernels_x3.hip). The launchers are declared in internal.h.
//
// Wave size is 64; every block is a multiple of 64 threads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "device_common.h"
#include "internal.h"

namespace stgcn {

// ---------------------------------------------------------------------------
// conv_gemm: see ConvGemmParams. Workgroup = 256 threads (4 waves), tile =
// 64 rows x (FT frames * V) columns (<= 256, padded to 8 MFMA column tiles).
// Wave w owns rows (w&1)*32..+31 and column tiles (w>>1)*4..+3: 4 accumulators
// of 32x32 fp32 (64 VGPRs). The reduction runs over input-channel chunks of CK:
// each chunk's weights (pre-packed [rtile][c][q][64], a contiguous block) and
// input windows (frames + temporal halo, zero-padded) are staged global ->
// registers -> LDS, double-buffered: the loads of chunk i+1 are in flight while
// chunk i runs on the matrix cores; one barrier per chunk. Each staged channel
// window serves all NQ taps (the tap shift is a per-lane LDS offset).
// ---------------------------------------------------------------------------
// Packs w[r*w_sr + c*w_sc + q*w_sq] into wpk[rt][c][q][r_local] (zero padded
// to n_rtiles*64 rows and Cpad channels).
__global__ void k_pack_conv_w(const float *w, float *wpk, int R, int C, int Cpad, int NQ,
                              int64_t w_sr, int64_t w_sc, int64_t w_sq, int n_rtiles) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)n_rtiles * Cpad * NQ * 64;
  if (idx >= total) return;
  const int rl = (int)(idx & 63);
  int64_t t = idx >> 6;
  const int q = (int)(t % NQ);
  t /= NQ;
  const int c = (int)(t % Cpad);
  const int rt = (int)(t / Cpad);
  const int r = rt * 64 + rl;
  float v = 0.f;
  if (r < R && c < C) v = w[(int64_t)r * w_sr + (int64_t)c * w_sc + (int64_t)q * w_sq];
  wpk[idx] = v;
}

template <int NQ, int CK>
__global__ __launch_bounds__(256, 2) void k_conv_gemm(ConvGemmParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int WSZ = CK * NQ * 64;   // floats of one weight chunk (multiple of 256)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 5, lo = lane & 31;
  const int nblk = gridDim.x;
  int bid = xcd_remap(blockIdx.x, nblk);
  const int rt = bid % p.n_rtiles;
  bid /= p.n_rtiles;
  const int mt = bid % p.n_mtiles;
  const int n = bid / p.n_mtiles;
  const int r0 = rt * kTileRows, m0 = mt * p.FT;
  const int V = p.V;
  const int span = (p.s_in * (p.FT - 1) + NQ) * V;
  const int SP = span | 1;  // odd pitch
  const int ISZ = round64(CK * SP);
  float *Ws0 = smem, *Ws1 = smem + WSZ;
  float *Is0 = smem + 2 * WSZ, *Is1 = smem + 2 * WSZ + ISZ;
  const int cstride = p.T_src * V;
  const int g0 = (p.s_in * m0 + p.off) * V;
  const float *inN = p.in + (int64_t)n * p.in_bstride;
  const float *wblk = p.wpk + (int64_t)rt * p.Cpad * NQ * 64;
  const int ncols = p.FT * V;
  const int nchunks = (p.C + CK - 1) / CK;

  const int mi = wave & 1;
  const int nj0 = (wave >> 1) * 4;
  int bbase[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = (nj0 + j) * 32 + lo;
    if (col < ncols) {
      const int mf = col / V;
      bbase[j] = p.s_in * mf * V + (col - mf * V);
    } else {
      bbase[j] = 0;  // padding column: reads a staged value, result discarded
    }
  }
  // LDS-DMA staging of chunk `chunk` into (Ws, Is). Input image [CK][SP]:
  // element e -> (c = e / SP, o = e % SP); this lane starts at e = wave*64+lane
  // and advances by 256 per instruction.
  const int e_init = wave * 64 + lane;
  const int c_init = e_init / SP, o_init = e_init - c_init * SP;
  const int dc = 256 / SP, dO = 256 - dc * SP;
  const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(wblk, (int64_t)p.Cpad * NQ * 64);
  const __amdgpu_buffer_rsrc_t rs_in = make_rsrc(inN, (int64_t)p.C * cstride);
  auto stage = [&](int chunk, float *Ws, float *Is) {
    const unsigned wbase = (unsigned)(chunk * WSZ + wave * 64 + lane) * 4u;
#pragma unroll
    for (int i = 0; i < WSZ / 256; ++i) blds_f32(rs_w, wbase + i * 1024u, Ws + (i * 4 + wave) * 64);
    const int climit = p.C - chunk * CK;
    const int cbase = chunk * CK * cstride + g0;
    int c = c_init, o = o_init;
    for (int E0 = wave * 64; E0 < ISZ; E0 += 256) {
      const int g = g0 + o;
      const bool ok = c < CK && c < climit && o < span && g >= 0 && g < cstride;
      blds_f32(rs_in, ok ? (unsigned)(cbase + c * cstride + o) * 4u : kOOB, Is + E0);
      o += dO;
      c += dc;
      if (o >= SP) {
        o -= SP;
        ++c;
      }
    }
  };

  floatx16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  stage(0, Ws0, Is0);
  __syncthreads();
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    const bool odd = chunk & 1;
    const float *Ws = odd ? Ws1 : Ws0;
    const float *Is = odd ? Is1 : Is0;
    if (chunk + 1 < nchunks) stage(chunk + 1, odd ? Ws0 : Ws1, odd ? Is0 : Is1);
    const float *wp = Ws + hi * NQ * 64 + mi * 32 + lo;
    const float *ip = Is + hi * SP;
#pragma unroll 2
    for (int cp = 0; cp < CK / 2; ++cp) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const float a = wp[(2 * cp * NQ + q) * 64];
        const float *iq = ip + 2 * cp * SP + q * V;
        const float b0 = iq[bbase[0]], b1 = iq[bbase[1]], b2 = iq[bbase[2]], b3 = iq[bbase[3]];
        acc[0] = mfma32(a, b0, acc[0]);
        acc[1] = mfma32(a, b1, acc[1]);
        acc[2] = mfma32(a, b2, acc[2]);
        acc[3] = mfma32(a, b3, acc[3]);
      }
    }
    __syncthreads();  // retires this wave's LDS-DMA (vmcnt(0)) and publishes the next chunk
  }

  // Epilogue: bias, store, optional per-row BN statistics (fp64).
  float *outN = p.out + (int64_t)n * p.out_bstride;
  const int64_t ostride = (int64_t)p.T_dst * V;
  int64_t ocol[4];
  bool cok[4];
  int cv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = (nj0 + j) * 32 + lo;
    const int mf = col / V;
    const int v = col - mf * V;
    const int m = m0 + mf;
    cok[j] = col < ncols && m < p.M;
    cv[j] = v;
    ocol[j] = (int64_t)(p.s_out * m + p.p_out) * V + v;
  }
  // per-lane partial BN statistics (fp64 over this lane's 4 columns), summed
  // across lanes and waves through LDS (the staging buffers are free now).
  double *red = reinterpret_cast<double *>(smem);  // [4 waves][16 regs][2][64 lanes]
  // (every load ahead of the stores that follow it: vmcnt counts loads and
  // stores in one in-order counter, so a load issued after a store is only
  // waited for together with that store. Row biases first; bias-table and
  // residual values one register ahead of their stores)
  float brv[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = r0 + mi * 32 + (i & 3) + 8 * (i >> 2) + 4 * hi;
    brv[i] = (row < p.R && p.bias_r) ? p.bias_r[row] : 0.f;
  }
  const float *resN = p.res ? p.res + (p.res_shared ? 0 : (int64_t)n * p.out_bstride) : nullptr;
  float pbv[2][4], prs[2][4];
  auto pre = [&](int i, float (&bv)[4], float (&rs)[4]) {
    const int row = r0 + mi * 32 + (i & 3) + 8 * (i >> 2) + 4 * hi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bv[j] = 0.f;
      rs[j] = 0.f;
      if (row < p.R && cok[j]) {
        if (p.bias_rv) bv[j] = p.bias_rv[row * V + cv[j]];
        if (resN) rs[j] = resN[row * ostride + ocol[j]];
      }
    }
  };
  // (DROP: a compile-time copy of the loop for calls with dropout, so the copy
  // every other call runs holds no seed and has no dropout branch)
  auto rows = [&](auto drop_c) {
    constexpr bool DROP = decltype(drop_c)::value;
    Dropout drop;
    if constexpr (DROP) drop = dropout_resolve(p.drop);
    pre(0, pbv[0], prs[0]);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i + 1 < 16) pre(i + 1, pbv[(i + 1) & 1], prs[(i + 1) & 1]);
      const int row = r0 + mi * 32 + (i & 3) + 8 * (i >> 2) + 4 * hi;
      const bool rok = row < p.R;
      const float br = brv[i];
      double s = 0.0, sq = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (rok && cok[j]) {
          float val = acc[j][i] + br;
          if (p.bias_rv) val += pbv[i & 1][j];
          if (p.res) val += prs[i & 1][j];
          if (p.relu_out) val = relu_max(val);
          if constexpr (DROP)
            val = dropout_keep(drop, (uint64_t)n * p.out_bstride + row * ostride + ocol[j])
                      ? val * drop.scale
                      : 0.f;
          outN[row * ostride + ocol[j]] = val;
          s += val;
          sq += (double)val * val;
        }
      }
      if (p.stat_sum) {
        red[((wave * 16 + i) * 2 + 0) * 64 + lane] = s;
        red[((wave * 16 + i) * 2 + 1) * 64 + lane] = sq;
      }
    }
  };
  if (p.drop.thresh)  // (uniform)
    rows(std::true_type{});
  else
    rows(std::false_type{});
  if (p.stat_sum) {
    __syncthreads();
    if (tid < 128) {
      // row rl of the tile: wave halves mi = rl / 32 (waves mi and mi + 2),
      // register i and lane half h from rl % 32 = (i&3) + 8*(i>>2) + 4*h
      const int rl = tid >> 1, st = tid & 1;
      const int m = rl >> 5, rr = rl & 31;
      const int h = (rr >> 2) & 1, i = (rr & 3) + 4 * (rr >> 3);
      double acc_s = 0.0;
      for (int w = m; w < 4; w += 2) {
        const double *src = red + ((w * 16 + i) * 2 + st) * 64 + h * 32;
        // rotated start: the 32 lanes of a wave half read 32 different banks
        for (int l = 0; l < 32; ++l) acc_s += src[(l + tid) & 31];
      }
      const int row = r0 + rl;
      if (row < p.R) atomicAdd((st ? p.stat_sq : p.stat_sum) + row, acc_s);
    }
  }
}

// ---------------------------------------------------------------------------
// k_tconv: conv_gemm specialised on the joint count V and the input stride
// (FT = kTileCols / V frames per tile). With the image geometry known at
// compile time every LDS operand read is (per-lane base + immediate), the
// input DMA offsets of a lane are the same for every channel chunk (computed
// once; the chunk and the channel bound live in the buffer resource, so the
// last partial chunk and the temporal halo zero-fill through the hardware
// range check), the packed-weight chunk moves in 16-byte LDS-DMA pieces, and
// the k-loop is fully unrolled with explicitly double-buffered operands (the
// LDS reads of step s+1 are in flight under the 4 MFMAs of step s).
// ---------------------------------------------------------------------------
template <int NQ, int CK, int V, int SIN>
struct ConvGeo {
  static constexpr int FT = kTileCols / V;
  static constexpr int NCOLS = FT * V;
  static constexpr int SPAN = (SIN * (FT - 1) + NQ) * V;
  static constexpr int SP = SPAN | 1;  // odd pitch
  static constexpr int ISZ = round64(CK * SP);
  static constexpr int WSZ = CK * NQ * 64;
  static constexpr int IROWS = ISZ / 64;              // 64-float DMA rows of the input image
  static constexpr int NI = (IROWS + 3) / 4;          // rows per wave (upper bound)
  static constexpr int WROWS = (WSZ + 255) / 256;     // 256-float (16 B/lane) weight rows
  static constexpr int WLAST = (WSZ % 256) / 4;       // lanes of a partial last row (0: full)
  static constexpr int NS = CK / 2 * NQ;              // MFMA k-steps per chunk
  static_assert(CK % 2 == 0 && WSZ % 4 == 0, "k-steps pair channels; 16-byte weight pieces");
  // ring-buffered staging: the chunk's DMA rows (WROWS 16-byte weight rows,
  // then input rows) are dealt round-robin to the 4 waves, padded with extra
  // input rows (zero-filled, never read) so every wave issues DPW DMAs.
  static constexpr int DPW = (WROWS + IROWS + 3) / 4;   // DMAs per wave per chunk
  static constexpr int IROWS_P = 4 * DPW - WROWS;       // input rows incl. padding
  static constexpr int WBUF = WROWS * 256, IBUF = IROWS_P * 64;
  static constexpr int BUF = WBUF + IBUF;               // floats per ring slot
  // ring depth: 3 slots (the short spatial chunks too: 2 slots measured 4-5%
  // slower at the cfg2 layer shapes once bias_rv moved to LDS)
  static constexpr int STAGES = 3;
  static_assert((STAGES - 2) * DPW < 64, "vmcnt range");
  // Input stride 2: each channel's window is stored de-interleaved, even
  // frames first (NFE of them) then odd frames, so output column (mf, v) at
  // tap q reads position TAPOFF(q) + mf*V + v: consecutive columns hit
  // consecutive words (the interleaved layout read 2- to 3-way bank conflicts).
  static constexpr int NF = SPAN / V;                  // window frames
  static constexpr int NFE = (NF + 1) / 2;             // even frames
  static __host__ __device__ constexpr int tapoff(int q) {
    return SIN == 2 ? (q & 1) * NFE * V + (q >> 1) * V : q * V;
  }
  // window position (de-interleaved layout) -> frame offset within the window
  static __host__ __device__ constexpr int src_pos(int o) {
    return SIN != 2 ? o
                    : (o < NFE * V ? 2 * (o / V) * V + o % V
                                   : (2 * ((o - NFE * V) / V) + 1) * V + (o - NFE * V) % V);
  }
};

template <int NQ, int CK, int V, int SIN>
__global__ __launch_bounds__(256, 2) void k_tconv(ConvGemmParams p) {
  using G = ConvGeo<NQ, CK, V, SIN>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, lo = lane & 31;
  int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int rt = bid % p.n_rtiles;
  bid /= p.n_rtiles;
  const int mt = bid % p.n_mtiles;
  const int n = bid / p.n_mtiles;
  const int r0 = rt * kTileRows, m0 = mt * G::FT;
  const int cstride = p.T_src * V;
  const int g0 = (SIN * m0 + p.off) * V;
  const float *inN = p.in + (int64_t)n * p.in_bstride;
  const float *wblk = p.wpk + (int64_t)rt * p.Cpad * NQ * 64;
  const int nchunks = (p.C + CK - 1) / CK;
  const int mi = wave & 1;
  const int nj0 = (wave >> 1) * 4;

  int bb[4];  // per-lane LDS offset of this lane's B column (k-row hi) in the image
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = (nj0 + j) * 32 + lo;
    const int mf = col / V;
    bb[j] = hi * G::SP + (col < G::NCOLS ? (SIN == 2 ? col : SIN * mf * V + (col - mf * V)) : 0);
  }
  // DMA slot k of this wave: row d = 4k + wave; d < WROWS: weight row d
  // (16 B/lane), else input row d - WROWS (4 B/lane, byte offset voff[k]
  // relative to the chunk's first channel; kOOB outside the image)
  unsigned voff[G::DPW];
#pragma unroll
  for (int k = 0; k < G::DPW; ++k) {
    const int d = 4 * k + wave;
    const int e = (d - G::WROWS) * 64 + lane;
    const int c = e / G::SP, o = e - c * G::SP;
    const int g = g0 + (o < G::SPAN ? G::src_pos(o) : o);
    const bool ok = d >= G::WROWS && c < CK && o < G::SPAN && g >= 0 && g < cstride;
    voff[k] = ok ? (unsigned)(c * cstride + g) * 4u : kOOB;
  }
  const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(wblk, (int64_t)p.Cpad * NQ * 64);
  auto stage = [&](int chunk, float *Ws, float *Is) {
    const __amdgpu_buffer_rsrc_t rs_in =
        make_rsrc(inN + (int64_t)chunk * CK * cstride, (int64_t)(p.C - chunk * CK) * cstride);
#pragma unroll
    for (int k = 0; k < G::DPW; ++k) {
      const int d = 4 * k + wave;  // wave-uniform
      if (d < G::WROWS) {
        // a partial last weight row still issues (OOB lanes: zero) so that every
        // wave's DMA count stays DPW
        const bool lane_ok = G::WLAST == 0 || d < G::WROWS - 1 || lane < G::WLAST;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rs_w, Ws + d * 256, 16,
            lane_ok ? (unsigned)(chunk * G::WSZ + d * 256 + lane * 4) * 4u : kOOB, 0, 0, 0);
      } else {
        blds_f32(rs_in, voff[k], Is + (d - G::WROWS) * 64);
      }
    }
  };

  floatx16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  // STAGES-slot ring: chunks c+1 .. c+STAGES-1 are in flight while chunk c
  // computes. Each wave waits only for its own DMAs of chunk c (vmcnt counts
  // retire in order), then one barrier publishes the chunk (a fenced
  // __syncthreads would drain the whole ring).
  constexpr int S = G::STAGES;
  auto wbuf = [&](int slot) { return smem + slot * G::BUF; };
  auto ibuf = [&](int slot) { return smem + slot * G::BUF + G::WBUF; };
#pragma unroll
  for (int c = 0; c < S - 1; ++c)
    if (c < nchunks) stage(c, wbuf(c), ibuf(c));
  auto body = [&](int chunk, auto slot_c) {
    constexpr int SLOT = decltype(slot_c)::value;
    if (chunk + 1 < nchunks)  // chunk c+1 may stay in flight
      asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((S - 2) * G::DPW) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    if (chunk + S - 1 < nchunks)
      stage(chunk + S - 1, wbuf((SLOT + S - 1) % S), ibuf((SLOT + S - 1) % S));
    const float *Ws = wbuf(SLOT), *Is = ibuf(SLOT);
    const float *wp = Ws + hi * NQ * 64 + mi * 32 + lo;
    const float *ib0 = Is + bb[0], *ib1 = Is + bb[1], *ib2 = Is + bb[2], *ib3 = Is + bb[3];
    constexpr int PD = 2;  // operands are read PD k-steps ahead of their MFMAs
    float a[PD + 1], b[PD + 1][4];
    auto ld = [&](int s, int set) {
      const int cp = s / NQ, q = s - cp * NQ;
      const int bo = 2 * cp * G::SP + G::tapoff(q);
      a[set] = wp[(2 * cp * NQ + q) * 64];
      b[set][0] = ib0[bo];
      b[set][1] = ib1[bo];
      b[set][2] = ib2[bo];
      b[set][3] = ib3[bo];
    };
#pragma unroll
    for (int s = 0; s < PD && s < G::NS; ++s) ld(s, s);
#pragma unroll
    for (int s = 0; s < G::NS; ++s) {
      if (s + PD < G::NS) ld(s + PD, (s + PD) % (PD + 1));
      const int c = s % (PD + 1);
      acc[0] = mfma32(a[c], b[c][0], acc[0]);
      acc[1] = mfma32(a[c], b[c][1], acc[1]);
      acc[2] = mfma32(a[c], b[c][2], acc[2]);
      acc[3] = mfma32(a[c], b[c][3], acc[3]);
      // issue order per step: step s+PD's 5 LDS reads, then step s's 4 MFMAs
      __builtin_amdgcn_sched_group_barrier(0x100, 5, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  static_assert(S == 3, "ring depth");
  for (int chunk = 0; chunk < nchunks; chunk += S) {
    body(chunk, std::integral_constant<int, 0>{});
    if (chunk + 1 < nchunks) body(chunk + 1, std::integral_constant<int, 1>{});
    if (chunk + 2 < nchunks) body(chunk + 2, std::integral_constant<int, 2>{});
  }
  asm volatile("s_barrier" ::: "memory");  // every wave done reading the ring (LDS reuse)

  conv_tile_epilogue<V, G::NCOLS, NQ == 1>(p, acc, n, r0, m0, smem);
}




// The (V, stride, NQ) combinations with a specialised k_tconv instantiation:
// the joint counts of the reference's skeleton graphs (coco18, body25,
// two-person body25), input stride 1 (and 2 for the strided temporal forward).
static bool tconv_specialised(const ConvGemmParams &p) {
  if (p.V != 18 && p.V != 25 && p.V != 50) return false;
  if (p.FT != kTileCols / p.V) return false;
  if (p.s_in == 2) return p.NQ == 9;
  return p.s_in == 1 && (p.NQ == 1 || p.NQ == 4 || p.NQ == 5 || p.NQ == 9);
}

// Channels per reduction chunk. Specialised kernels: 8 for the spatial GEMM,
// 2 for the temporal taps (3-slot ring, 27 KB of LDS: 4 workgroups per CU);
// measured against 16/32 and 4/6/8.
constexpr int kCk1 = 8, kCkTaps = 2;
static int conv_ck(const ConvGemmParams &p) {
  if (!tconv_specialised(p)) return p.NQ == 1 ? 32 : 8;
  return p.NQ == 1 ? kCk1 : kCkTaps;
}

int conv_gemm_cpad(const ConvGemmParams &p) {
  const int CK = conv_ck(p);
  return (p.C + CK - 1) / CK * CK;
}

size_t conv_gemm_wpk_floats(const ConvGemmParams &p) {
  return (size_t)p.n_rtiles * conv_gemm_cpad(p) * p.NQ * 64;
}

int conv_gemm_span(const ConvGemmParams &p) { return (p.s_in * (p.FT - 1) + p.NQ) * p.V; }

size_t conv_gemm_lds_bytes(const ConvGemmParams &p) {
  const int CK = conv_ck(p);
  const size_t stage = sizeof(float) * 2 * ((size_t)CK * p.NQ * 64 + round64(CK * (conv_gemm_span(p) | 1)));
  if (tconv_specialised(p)) {  // ring of ConvGeo::STAGES slots; stats partials (2 KiB) reuse it
    const int WROWS = (CK * p.NQ * 64 + 255) / 256;
    const int IROWS = round64(CK * (conv_gemm_span(p) | 1)) / 64;
    const int DPW = (WROWS + IROWS + 3) / 4;
    constexpr int stages = 3;  // ConvGeo::STAGES
    return sizeof(float) * stages * ((size_t)WROWS * 256 + (size_t)(4 * DPW - WROWS) * 64);
  }
  const size_t stats = sizeof(double) * 4 * 16 * 2 * 64;  // k_conv_gemm epilogue buffer
  return stage > stats ? stage : stats;
}

bool conv_gemm_supported(const ConvGemmParams &p) {
  return p.FT * p.V <= kTileCols && conv_gemm_lds_bytes(p) <= 160 * 1024;
}

template <int NQ, int CK, int V, int SIN>
static bool launch_tconv_if(const ConvGemmParams &p, int nblk, size_t lds, hipStream_t s) {
  if (p.V != V || p.s_in != SIN || p.FT != ConvGeo<NQ, CK, V, SIN>::FT) return false;
  hipLaunchKernelGGL((k_tconv<NQ, CK, V, SIN>), dim3(nblk), dim3(256), lds, s, p);
  return true;
}

template <int NQ, int CK>
static bool launch_tconv_v(const ConvGemmParams &p, int nblk, size_t lds, hipStream_t s) {
  if (launch_tconv_if<NQ, CK, 18, 1>(p, nblk, lds, s)) return true;
  if (launch_tconv_if<NQ, CK, 25, 1>(p, nblk, lds, s)) return true;
  if (launch_tconv_if<NQ, CK, 50, 1>(p, nblk, lds, s)) return true;
  if constexpr (NQ == 9) {
    if (launch_tconv_if<NQ, CK, 18, 2>(p, nblk, lds, s)) return true;
    if (launch_tconv_if<NQ, CK, 25, 2>(p, nblk, lds, s)) return true;
    if (launch_tconv_if<NQ, CK, 50, 2>(p, nblk, lds, s)) return true;
  }
  return false;
}

hipError_t launch_conv_gemm(const ConvGemmParams &p0, hipStream_t s) {
  // (per-tile statistics partials: k_conv_x3's row-major epilogue only)
  if (p0.stat_part && (p0.s_out != 1 || !p0.stat_sum)) return hipErrorInvalidValue;
  if (p0.bf16 == 3 && conv_x3_supported(p0)) return launch_conv_x3(p0, s);
  // (the fused SpatialConv backward epilogue and the fp16 operand scales exist in
  // k_conv_x3 only: any other kernel would ignore them and write H / wrong results)
  if (p0.spb || p0.f16x2 || p0.stat_part) return hipErrorInvalidValue;
  if (p0.bf16 == 1 && conv_b1_supported(p0)) return launch_conv_b1(p0, s);
  if (p0.bf16 == 1 && conv_bf16_supported(p0)) return launch_conv_bf16(p0, s);
  // (bf16-stored operands: only the kernels above read / write them)
  if (p0.in_bf16 || p0.out_bf16) return hipErrorInvalidValue;
  ConvGemmParams p = p0;
  if (!conv_gemm_supported(p) || !p.wpk) return hipErrorInvalidValue;
  p.Cpad = conv_gemm_cpad(p);
  {
    const int64_t total = (int64_t)conv_gemm_wpk_floats(p);
    hipLaunchKernelGGL(k_pack_conv_w, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                       p.w, p.wpk, p.R, p.C, p.Cpad, p.NQ, p.w_sr, p.w_sc, p.w_sq, p.n_rtiles);
  }
  const int nblk = p.N * p.n_mtiles * p.n_rtiles;
  const size_t lds = conv_gemm_lds_bytes(p);
  if (tconv_specialised(p)) {
    bool done = false;  // (chunk channels as conv_ck)
    switch (p.NQ) {
      case 1:
        done = launch_tconv_v<1, kCk1>(p, nblk, lds, s);
        break;
      case 4:
        done = launch_tconv_v<4, kCkTaps>(p, nblk, lds, s);
        break;
      case 5:
        done = launch_tconv_v<5, kCkTaps>(p, nblk, lds, s);
        break;
      case 9:
        done = launch_tconv_v<9, kCkTaps>(p, nblk, lds, s);
        break;
    }
    return done ? hipGetLastError() : hipErrorInvalidValue;
  }
  switch (p.NQ) {
    case 1:
      hipLaunchKernelGGL((k_conv_gemm<1, 32>), dim3(nblk), dim3(256), lds, s, p);
      break;
    case 4:
      hipLaunchKernelGGL((k_conv_gemm<4, 8>), dim3(nblk), dim3(256), lds, s, p);
      break;
    case 5:
      hipLaunchKernelGGL((k_conv_gemm<5, 8>), dim3(nblk), dim3(256), lds, s, p);
      break;
    case 9:
      hipLaunchKernelGGL((k_conv_gemm<9, 8>), dim3(nblk), dim3(256), lds, s, p);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// wgrad: see WgradParams. Workgroup = 256 threads, output tile 64 rows (r) x
// JT columns (j = c*NQ + q), JT = 192 (NQ=9) or 128 (NQ=1). Wave w owns rows
// (w&1)*32..+31 and column tiles (w>>1)*NJW..+NJW-1 (NJW = JT/64). The
// reduction runs over work items (clip n, FT frames): P[64 rows][FT*V cols]
// and the Q channel windows of the tile's j range are staged global ->
// registers -> LDS, double-buffered; one barrier per item. The split's partial
// tile is written to its slab (reduced in fixed order by k_slab_reduce).
// ---------------------------------------------------------------------------
template <int NQ, int JT>
__global__ __launch_bounds__(256, 2) void k_wgrad(WgradParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NJW = JT / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 5, lo = lane & 31;
  const int nblk = gridDim.x;
  int bid = xcd_remap(blockIdx.x, nblk);
  const int split = bid % p.S;
  bid /= p.S;
  const int jt = bid % p.n_jtiles;
  const int rt = bid / p.n_jtiles;
  const int r0 = rt * 64, j0 = jt * JT;
  const int J = p.C * NQ;
  const int V = p.V;
  const int Vp = (V + 1) & ~1;          // joints padded to even: k-steps never straddle frames
  const int ncols = p.FT * Vp;          // P image columns (frame-padded)
  const int PP = ncols | 1;             // odd pitch
  const int c_lo = j0 / NQ;
  int c_hi = (j0 + JT - 1) / NQ + 1;
  if (c_hi > p.C) c_hi = p.C;
  const int nc = c_hi - c_lo;
  const int span = (p.s_in * (p.FT - 1) + NQ) * V;
  const int QP = (span + 2) | 1;        // >= span + 1: the odd-V pad column reads a finite value
  const int PSZ = round64(64 * PP), QSZ = round64((nc + 1) * QP);  // Q row nc = zeros
  float *Ps0 = smem, *Qs0 = smem + PSZ;
  float *Ps1 = smem + PSZ + QSZ, *Qs1 = Ps1 + PSZ;
  const int mi = wave & 1;
  const int nj0 = (wave >> 1) * NJW;
  int qoff[NJW];
#pragma unroll
  for (int t = 0; t < NJW; ++t) {
    const int j = j0 + (nj0 + t) * 32 + lo;
    if (j < J) {
      const int c = j / NQ, q = j - c * NQ;
      qoff[t] = (c - c_lo) * QP + q * V;
    } else {
      qoff[t] = nc * QP;  // zero row
    }
  }
  floatx16 acc[NJW];
#pragma unroll
  for (int t = 0; t < NJW; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  const int total = p.N * p.n_mtiles;
  const int per = (total + p.S - 1) / p.S;
  const int it0 = split * per;
  int it1 = it0 + per;
  if (it1 > total) it1 = total;
  const int pcs = p.M * V;      // P channel stride
  const int qcs = p.T_src * V;  // Q channel stride
  // per-lane staging walk: element e = wave*64 + lane + 256*i of each image
  const int e_init = wave * 64 + lane;
  const int prow_i = e_init / PP, po_i = e_init - prow_i * PP;
  const int dpr = 256 / PP, dpo = 256 - dpr * PP;
  const int qrow_i = e_init / QP, qo_i = e_init - qrow_i * QP;
  const int dqr = 256 / QP, dqo = 256 - dqr * QP;
  const int prow_lim = min(64, p.R - r0);

  // LDS-DMA staging of work item `it`: P image [64][PP] (frame-padded columns)
  // and Q image [nc+1][QP]; out-of-range elements read as 0 (buffer OOB).
  auto stage = [&](int it, float *Ps, float *Qs) {
    const int n = it / p.n_mtiles, mt = it - n * p.n_mtiles;
    const int m0 = mt * p.FT;
    const __amdgpu_buffer_rsrc_t rs_p =
        make_rsrc(p.P + (int64_t)n * p.p_bstride + (int64_t)r0 * pcs, (int64_t)prow_lim * pcs);
    const int fl = p.M - m0;  // frames left in this clip
    int row = prow_i, o = po_i;
    for (int E0 = wave * 64; E0 < PSZ; E0 += 256) {
      const int mf = o / Vp, v = o - mf * Vp;
      const bool ok = row < prow_lim && o < ncols && v < V && mf < fl;
      blds_f32(rs_p, ok ? (unsigned)(row * pcs + (m0 + mf) * V + v) * 4u : kOOB, Ps + E0);
      o += dpo;
      row += dpr;
      if (o >= PP) {
        o -= PP;
        ++row;
      }
    }
    const int qg0 = (p.s_in * m0 + p.off) * V;
    const __amdgpu_buffer_rsrc_t rs_q =
        make_rsrc(p.Q + (int64_t)n * p.q_bstride + (int64_t)c_lo * qcs, (int64_t)nc * qcs);
    row = qrow_i;
    o = qo_i;
    for (int E0 = wave * 64; E0 < QSZ; E0 += 256) {
      const int g = qg0 + o;
      const bool ok = row < nc && o < span && g >= 0 && g < qcs;
      blds_f32(rs_q, ok ? (unsigned)(row * qcs + g) * 4u : kOOB, Qs + E0);
      o += dqo;
      row += dqr;
      if (o >= QP) {
        o -= QP;
        ++row;
      }
    }
  };

  const int hv = Vp / 2;  // k-steps per frame
  if (it0 < it1) stage(it0, Ps0, Qs0);
  __syncthreads();
  for (int it = it0; it < it1; ++it) {
    const bool odd = (it - it0) & 1;
    const float *Ps = odd ? Ps1 : Ps0;
    const float *Qs = odd ? Qs1 : Qs0;
    if (it + 1 < it1) stage(it + 1, odd ? Ps0 : Ps1, odd ? Qs0 : Qs1);
    // k-steps walk the frame-padded P columns contiguously (A offset += 2) and
    // the Q window of each frame (B offset += 2, jump s*V - Vp per frame).
    // Operands of step k+1 are read before the MFMAs of step k.
    const float *pa = Ps + (mi * 32 + lo) * PP + hi;
    const float *qb = Qs + hi;
    const int nsteps = p.FT * hv;
    const int fjump = p.s_in * V - Vp;
    int aoff = 0, boff = 0, kin = 0;
    float a_cur = pa[0];
    float b_cur[NJW];
#pragma unroll
    for (int t = 0; t < NJW; ++t) b_cur[t] = qb[qoff[t]];
    for (int kk = 0; kk < nsteps - 1; ++kk) {
      aoff += 2;
      boff += 2;
      if (++kin == hv) {
        kin = 0;
        boff += fjump;
      }
      const float a_nxt = pa[aoff];
      float b_nxt[NJW];
#pragma unroll
      for (int t = 0; t < NJW; ++t) b_nxt[t] = qb[qoff[t] + boff];
#pragma unroll
      for (int t = 0; t < NJW; ++t) acc[t] = mfma32(a_cur, b_cur[t], acc[t]);
      a_cur = a_nxt;
#pragma unroll
      for (int t = 0; t < NJW; ++t) b_cur[t] = b_nxt[t];
    }
#pragma unroll
    for (int t = 0; t < NJW; ++t) acc[t] = mfma32(a_cur, b_cur[t], acc[t]);
    __syncthreads();  // retires this wave's LDS-DMA and publishes the next item
  }
  float *dst = p.slab + (int64_t)split * p.R * J;
#pragma unroll
  for (int t = 0; t < NJW; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = r0 + mi * 32 + (i & 3) + 8 * (i >> 2) + 4 * hi;
      const int j = j0 + (nj0 + t) * 32 + lo;
      if (row < p.R && j < J) dst[(int64_t)row * J + j] = acc[t][i];
    }
}

// ---------------------------------------------------------------------------
// wgrad_taps: the (9,1) temporal conv weight gradient,
//   dWt[r][c][q] = sum_{n,m,v} P[n,r,m,v] * Q[n,c, s*m + q + off, v],
// tile = 64 rows x CB channels x all 9 taps. 4 waves; wave w: rows
// (w&1)*32..+31; CB=64: channels (w>>1)*32..+31, taps 0..8 (9 MFMA tiles);
// CB=32: all 32 channels, taps (w>>1) ? 5..8 : 0..4. MFMA column tiles are
// tap-major/channel-minor, so a B read is 32 lanes on 32 channel rows of an
// odd-pitch image (conflict-free) and one A read feeds up to 9 MFMAs.
// Work items (clip n, FT frames) are staged by LDS-DMA, double-buffered.
// ---------------------------------------------------------------------------
// VT > 0: specialised on the joint count VT, input stride SIN and FTT frames
// per item (compile-time image geometry, fully unrolled scheduled k-loop);
// VT = 0: runtime geometry.
template <int CB, int NW, int VT, int SIN, int FTT>
__global__ __launch_bounds__(NW * 64, 1) void k_wgrad_taps(WgradParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  // waves: (row half mi, channel half cb, tap group qh); CB=64/NW=8 -> 2x2x2,
  // CB=32/NW=4 -> 2x1x2; tap groups 0..4 and 5..8
  constexpr int NT = 5;  // MFMA column tiles per wave
  constexpr int NTH = NW * 64;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, lo = lane & 31;
  const int nblk = gridDim.x;
  int bid = xcd_remap(blockIdx.x, nblk);
  const int split = bid % p.S;
  bid /= p.S;
  const int ct = bid % p.n_jtiles;
  const int rt = bid / p.n_jtiles;
  const int r0 = rt * 64, c0 = ct * CB;
  const int V = VT ? VT : p.V;
  const int FT = VT ? FTT : p.FT;
  const int s_in = VT ? SIN : p.s_in;
  const int Vp = (V + 1) & ~1;
  const int ncols = FT * Vp;
  const int PP = ncols | 1;
  const int span = (s_in * (FT - 1) + 9) * V;
  const int QP = (span + 2) | 1;
  // images padded to whole DMA rounds of the workgroup (every wave issues the
  // same number of DMAs; the padding reads as zero)
  const int PSZ = (64 * PP + NTH - 1) / NTH * NTH, QSZ = (CB * QP + NTH - 1) / NTH * NTH;
  float *Ps0 = smem, *Qs0 = smem + PSZ;
  float *Ps1 = smem + PSZ + QSZ, *Qs1 = Ps1 + PSZ;
  const int mi = wave & 1;
  const int cb = CB == 64 ? ((wave >> 1) & 1) : 0;
  const int qh = CB == 64 ? (wave >> 2) : (wave >> 1);
  const int q0 = qh ? 5 : 0;
  const int nq = qh ? 4 : 5;
  int qoff[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) qoff[t] = (cb * 32 + lo) * QP + (q0 + t) * V;
  floatx16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  const int total = p.N * p.n_mtiles;
  const int per = (total + p.S - 1) / p.S;
  const int it0 = split * per;
  int it1 = it0 + per;
  if (it1 > total) it1 = total;
  const int pcs = p.M * V;
  const int qcs = p.T_src * V;
  const int prow_lim = min(64, p.R - r0);
  const int crow_lim = min(CB, p.C - c0);
  // P staging: per-lane element list is the same for every item; precompute
  // packed (offset | frame << 26), -1 when statically out of range.
  constexpr int MAXPE = VT ? (64 * ((FTT * ((VT + 1) & ~1)) | 1) + NTH - 1) / NTH
                          : 24 * 4 / NW;  // >= ceil(64 * PP / NTH) for PP <= 95
  int ppk[MAXPE];
  const int npe = PSZ / NTH;
  {
#pragma unroll
    for (int i = 0; i < MAXPE; ++i) {
      const int e = (i * NW + wave) * 64 + lane;
      const int row = e / PP, o = e - row * PP;
      const int mf = o / Vp, v = o - mf * Vp;
      const bool ok = i < npe && row < prow_lim && o < ncols && v < V;
      ppk[i] = ok ? ((row * pcs + mf * V + v) | (mf << 26)) : -1;
    }
  }
  const int qrow_i = (wave * 64 + lane) / QP, qo_i = (wave * 64 + lane) - qrow_i * QP;
  const int dqr = NTH / QP, dqo = NTH - dqr * QP;
  // Specialised geometry: the Q element list of a lane is also fixed per item;
  // precompute packed (row*qcs + o) | (o << 21), -1 when statically out of range
  // (qcs * 64 < 2^21 and o < 2^10 for the instantiated V, T <= 300).
  constexpr int QN = VT ? (CB * ((((SIN * (FTT - 1) + 9) * VT) + 2) | 1) + NTH - 1) / NTH : 1;
  int qpk[QN];
  if constexpr (VT > 0) {
#pragma unroll
    for (int i = 0; i < QN; ++i) {
      const int e = (i * NW + wave) * 64 + lane;
      const int row = e / QP, o = e - row * QP;
      const bool ok = row < crow_lim && o < span;
      qpk[i] = ok ? ((row * qcs + o) | (o << 21)) : -1;
    }
  }

  auto stage = [&](int it, float *Ps, float *Qs) {
    const int n = it / p.n_mtiles, mt = it - n * p.n_mtiles;
    const int m0 = mt * FT;
    const int fl = p.M - m0;
    const __amdgpu_buffer_rsrc_t rs_p =
        make_rsrc(p.P + (int64_t)n * p.p_bstride + (int64_t)r0 * pcs, (int64_t)prow_lim * pcs);
    const int m0V = m0 * V;
#pragma unroll
    for (int i = 0; i < MAXPE; ++i) {
      if (VT > 0 || i < npe) {
        const int pk = ppk[i];
        const bool ok = pk >= 0 && (pk >> 26) < fl;
        blds_f32(rs_p, ok ? (unsigned)((pk & 0x3ffffff) + m0V) * 4u : kOOB,
                 Ps + (i * NW + wave) * 64);
      }
    }
    const int qg0 = (s_in * m0 + p.off) * V;
    const __amdgpu_buffer_rsrc_t rs_q =
        make_rsrc(p.Q + (int64_t)n * p.q_bstride + (int64_t)c0 * qcs, (int64_t)crow_lim * qcs);
    if constexpr (VT > 0) {
      // interior items (no temporal halo outside the clip) skip the frame test
      auto qdma = [&](auto interior_c) {
        constexpr bool INTERIOR = decltype(interior_c)::value;
#pragma unroll
        for (int i = 0; i < QN; ++i) {
          const int pk = qpk[i];
          bool ok = pk >= 0;
          if constexpr (!INTERIOR) {
            const int g = qg0 + (pk >> 21);
            ok = ok && g >= 0 && g < qcs;
          }
          blds_f32(rs_q, ok ? (unsigned)((pk & 0x1fffff) + qg0) * 4u : kOOB,
                   Qs + (i * NW + wave) * 64);
        }
      };
      if (qg0 >= 0 && qg0 + span <= qcs)
        qdma(std::true_type{});
      else
        qdma(std::false_type{});
      return;
    }
    int row = qrow_i, o = qo_i;
    for (int E0 = wave * 64; E0 < QSZ; E0 += NTH) {
      const int g = qg0 + o;
      const bool ok = row < crow_lim && o < span && g >= 0 && g < qcs;
      blds_f32(rs_q, ok ? (unsigned)(row * qcs + g) * 4u : kOOB, Qs + E0);
      o += dqo;
      row += dqr;
      if (o >= QP) {
        o -= QP;
        ++row;
      }
    }
  };

  const int hv = Vp / 2;
  const int nsteps = FT * hv;
  const int fjump = s_in * V - Vp;
  if (it0 < it1) stage(it0, Ps0, Qs0);
  __syncthreads();
  for (int it = it0; it < it1; ++it) {
    const bool odd = (it - it0) & 1;
    const float *Ps = odd ? Ps1 : Ps0;
    const float *Qs = odd ? Qs1 : Qs0;
    if (it + 1 < it1) stage(it + 1, odd ? Ps0 : Ps1, odd ? Qs0 : Qs1);
    const float *pa = Ps + (mi * 32 + lo) * PP + hi;
    const float *qb = Qs + hi;
    if constexpr (VT > 0) {
      // fully unrolled; issue order per step: step k+PD's reads, then step k's MFMAs
      constexpr int HV = ((VT + 1) & ~1) / 2, NS = FTT * HV;
      constexpr int FJ = SIN * VT - 2 * HV;
      const float *qb0 = qb + qoff[0], *qb1 = qb + qoff[1], *qb2 = qb + qoff[2];
      const float *qb3 = qb + qoff[3], *qb4 = qb + qoff[4];
      const float *qbt[NT] = {qb0, qb1, qb2, qb3, qb4};
      // the tap count of the wave (5 or 4) is a template constant of the loop
      // body; operands are read PD steps ahead of their MFMAs (PD + 1 sets)
      auto body = [&](auto nqc) {
        constexpr int NQW = decltype(nqc)::value;
        constexpr int PD = 2;
        float a[PD + 1], b[PD + 1][NQW];
        auto ld = [&](int k, int set) {
          const int bo = 2 * k + (k / HV) * FJ;
          a[set] = pa[2 * k];
#pragma unroll
          for (int t = 0; t < NQW; ++t) b[set][t] = qbt[t][bo];
        };
#pragma unroll
        for (int k = 0; k < PD; ++k) ld(k, k);
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          if (k + PD < NS) ld(k + PD, (k + PD) % (PD + 1));
          const int c = k % (PD + 1);
#pragma unroll
          for (int t = 0; t < NQW; ++t) acc[t] = mfma32(a[c], b[c][t], acc[t]);
          __builtin_amdgcn_sched_group_barrier(0x100, NQW + 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, NQW, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      if (qh)
        body(std::integral_constant<int, 4>{});
      else
        body(std::integral_constant<int, 5>{});
      __syncthreads();
      continue;
    }
    // 2x-unrolled ping-pong operand sets: the reads of step k+1 are issued
    // before the MFMAs of step k and land in the other register set (no
    // rotation moves, so the wait before step k+1 covers only its own reads).
    int aoff = 0, boff = 0, kin = 0;
    auto advance = [&]() {
      aoff += 2;
      boff += 2;
      if (++kin == hv) {
        kin = 0;
        boff += fjump;
      }
    };
    float a0 = pa[0], a1 = 0.f;
    float b0[NT], b1[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) b0[t] = qb[qoff[t]];
    int kk = 0;
    for (; kk + 1 < nsteps; kk += 2) {
      advance();
      a1 = pa[aoff];
#pragma unroll
      for (int t = 0; t < NT; ++t) b1[t] = qb[qoff[t] + boff];
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (t < nq) acc[t] = mfma32(a0, b0[t], acc[t]);
      if (kk + 2 < nsteps) {
        advance();
        a0 = pa[aoff];
#pragma unroll
        for (int t = 0; t < NT; ++t) b0[t] = qb[qoff[t] + boff];
      }
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (t < nq) acc[t] = mfma32(a1, b1[t], acc[t]);
    }
    if (kk < nsteps) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (t < nq) acc[t] = mfma32(a0, b0[t], acc[t]);
    }
    __syncthreads();  // retires this wave's LDS-DMA and publishes the next item
  }
  // slab layout = the Conv2d weight (R, C, 9)
  float *dst = p.slab + (int64_t)split * p.R * p.C * 9;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t >= nq) continue;
    const int c = c0 + cb * 32 + lo;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = r0 + mi * 32 + (i & 3) + 8 * (i >> 2) + 4 * hi;
      if (row < p.R && c < p.C) dst[((int64_t)row * p.C + c) * 9 + q0 + t] = acc[t][i];
    }
  }
}

int wgrad_taps_cb(const WgradParams &p) { return p.V > 32 ? 32 : 64; }

size_t wgrad_taps_lds_bytes(const WgradParams &p) {
  const int CB = wgrad_taps_cb(p);
  const int NTH = CB == 64 ? 512 : 256;
  const int Vp = (p.V + 1) & ~1;
  const int PP = (p.FT * Vp) | 1;
  const int QP = ((p.s_in * (p.FT - 1) + 9) * p.V + 2) | 1;
  auto rnd = [&](int x) { return (x + NTH - 1) / NTH * NTH; };
  return sizeof(float) * 2 * (rnd(64 * PP) + rnd(CB * QP));
}

bool wgrad_taps_supported(const WgradParams &p) {
  const int Vp = (p.V + 1) & ~1;
  const int PP = (p.FT * Vp) | 1;
  return p.NQ == 9 && (64 * PP + 255) / 256 <= 24 && wgrad_taps_lds_bytes(p) <= 160 * 1024;
}

hipError_t launch_wgrad_taps(const WgradParams &p, hipStream_t s) {
  if (p.bf16 == 3) return launch_wgrad_x3(p, s);
  if (p.bf16) return launch_wgrad_bf16(p, s);
  if (!wgrad_taps_supported(p)) return hipErrorInvalidValue;
  const int nblk = p.n_rtiles * p.n_jtiles * p.S;
  const size_t lds = wgrad_taps_lds_bytes(p);
  // the plans make_wgrad_taps builds for the reference's graphs (FT = 80 / V,
  // reduced until the double-buffered images fit in LDS), else the runtime-geometry kernels
  if (p.V == 18 && p.FT == 4 && p.s_in == 1)
    hipLaunchKernelGGL((k_wgrad_taps<64, 8, 18, 1, 4>), dim3(nblk), dim3(512), lds, s, p);
  else if (p.V == 18 && p.FT == 3 && p.s_in == 2)
    hipLaunchKernelGGL((k_wgrad_taps<64, 8, 18, 2, 3>), dim3(nblk), dim3(512), lds, s, p);
  else if (p.V == 25 && p.FT == 2 && p.s_in == 1)
    hipLaunchKernelGGL((k_wgrad_taps<64, 8, 25, 1, 2>), dim3(nblk), dim3(512), lds, s, p);
  else if (p.V == 25 && p.FT == 1 && p.s_in == 2)
    hipLaunchKernelGGL((k_wgrad_taps<64, 8, 25, 2, 1>), dim3(nblk), dim3(512), lds, s, p);
  else if (p.V == 50 && p.FT == 1 && p.s_in == 1)
    hipLaunchKernelGGL((k_wgrad_taps<32, 4, 50, 1, 1>), dim3(nblk), dim3(256), lds, s, p);
  else if (p.V == 50 && p.FT == 1 && p.s_in == 2)
    hipLaunchKernelGGL((k_wgrad_taps<32, 4, 50, 2, 1>), dim3(nblk), dim3(256), lds, s, p);
  else if (wgrad_taps_cb(p) == 64)
    hipLaunchKernelGGL((k_wgrad_taps<64, 8, 0, 1, 1>), dim3(nblk), dim3(512), lds, s, p);
  else
    hipLaunchKernelGGL((k_wgrad_taps<32, 4, 0, 1, 1>), dim3(nblk), dim3(256), lds, s, p);
  return hipGetLastError();
}

static int wgrad_jt(int NQ) { return NQ == 1 ? 128 : 192; }

static void wgrad_geom(const WgradParams &p, int &PP, int &nc, int &QP) {
  const int JT = wgrad_jt(p.NQ);
  PP = (p.FT * ((p.V + 1) & ~1)) | 1;
  nc = JT / p.NQ + 2;
  if (nc > p.C) nc = p.C;
  QP = ((p.s_in * (p.FT - 1) + p.NQ) * p.V + 2) | 1;
}

int wgrad_ntiles_j(int C, int NQ) { return (C * NQ + wgrad_jt(NQ) - 1) / wgrad_jt(NQ); }

size_t wgrad_lds_bytes(const WgradParams &p) {
  int PP, nc, QP;
  wgrad_geom(p, PP, nc, QP);
  return sizeof(float) * 2 * (round64(64 * PP) + round64((nc + 1) * QP));
}

bool wgrad_supported(const WgradParams &p) { return wgrad_lds_bytes(p) <= 160 * 1024; }

// ---------------------------------------------------------------------------
// k_wgrad_sp: weight gradient of the 1x1 spatial conv (NQ = 1) as a split-K GEMM
//   slab[split][r][c] = sum_{(n, chunk) in split} sum_{l in chunk} P[n][r][l] Q[n][c][l]
// over the L = T*V contiguous columns of each clip row, in chunks of KC. Both
// operands are staged row-major [rows][PITCH = KC + 4] (PITCH/4 odd: each
// 16-lane group of a ds_read_b128 hits 16 distinct 16-byte slots), by 16-byte
// LDS-DMA when rows are 16-byte aligned, else 4-byte. One ds_read_b128 per
// operand feeds 4 MFMAs: lane (i, h) holds k = kb + 4h + u for MFMA u, the same
// k permutation on both operands. Workgroups of one split are consecutive in
// the (XCD-remapped) grid, so the tiles sharing a chunk share an L2.
// X3 (STGCN_F_F32X3 blocks): the same staging, the products as exact 3-way bf16
// splits on v_mfma_f32_32x32x16_bf16 (six products, h*h apart; kernels_x3.hip):
// 16-deep k-steps, lane half h holding k = kb + 8h + u (u < 8) of both operands
// (two 16-byte reads per operand), split in registers at fragment read.
// ---------------------------------------------------------------------------
// 8 floats (two 16-byte LDS reads) -> exact bf16 planes h, m, l (x == h + m + l)
__device__ __forceinline__ void wsp_planes(const float *src, uint4 &h, uint4 &m, uint4 &l) {
  const floatx4 *v = reinterpret_cast<const floatx4 *>(__builtin_assume_aligned(src, 16));
  const floatx4 x0 = v[0], x1 = v[1];
  const float f[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
  split_bf16x3(f[0], f[1], h.x, m.x, l.x);
  split_bf16x3(f[2], f[3], h.y, m.y, l.y);
  split_bf16x3(f[4], f[5], h.z, m.z, l.z);
  split_bf16x3(f[6], f[7], h.w, m.w, l.w);
}

template <int CT, bool X4, bool X3>
__global__ __launch_bounds__(256, 2) void k_wgrad_sp(WgradParams p) {
  constexpr int KC = CT == 64 ? 64 : 32, PITCH = KC + 4;
  static_assert((PITCH / 4) % 2 == 1, "ds_read_b128 conflict-free pitch");
  constexpr int PSZ = 64 * PITCH, QSZ = CT * PITCH;
  constexpr int NJ = CT / 64;               // 32-column accumulators per wave
  constexpr int G = X4 ? 4 : 1;             // floats per lane per DMA
  constexpr int PN = (PSZ / G + 255) / 256;  // DMA rounds per wave (upper bound)
  constexpr int QN = (QSZ / G + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *Ps0 = smem, *Qs0 = smem + PSZ, *Ps1 = smem + PSZ + QSZ, *Qs1 = Ps1 + PSZ;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, lo = lane & 31;
  int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int ntiles = p.n_rtiles * p.n_jtiles;
  const int tile = bid % ntiles;
  const int split = bid / ntiles;
  const int ct = tile % p.n_jtiles, rt = tile / p.n_jtiles;
  const int L = p.M * p.V;
  const int r0 = rt * 64, c0 = ct * CT;
  const int prow_lim = min(64, p.R - r0), qrow_lim = min(CT, p.C - c0);
  const int total = p.N * p.n_mtiles;
  const int per = (total + p.S - 1) / p.S;
  const int it0 = split * per;
  const int it1 = min(total, it0 + per);

  // fixed per-lane staging map: DMA round i of this wave fills LDS floats
  // [((i*4 + wave)*64 + lane) * G, +G) of the image
  int poff[PN], pcol[PN], qoff[QN], qcol[QN];
#pragma unroll
  for (int i = 0; i < PN; ++i) {
    const int pos = ((i * 4 + wave) * 64 + lane) * G;
    const int row = pos / PITCH, col = pos - row * PITCH;
    pcol[i] = col;
    poff[i] = (pos < PSZ && col < KC && row < prow_lim) ? row * L + col : -1;
  }
#pragma unroll
  for (int i = 0; i < QN; ++i) {
    const int pos = ((i * 4 + wave) * 64 + lane) * G;
    const int row = pos / PITCH, col = pos - row * PITCH;
    qcol[i] = col;
    qoff[i] = (pos < QSZ && col < KC && row < qrow_lim) ? row * L + col : -1;
  }
  auto dma = [&](__amdgpu_buffer_rsrc_t rs, unsigned voff, float *lds) {
    if constexpr (X4)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, lds, 16, voff, 0, 0, 0);
    else
      blds_f32(rs, voff, lds);
  };
  auto stage = [&](int it, float *Ps, float *Qs) {
    const int n = it / p.n_mtiles, kc = it - n * p.n_mtiles;
    const int l0 = kc * KC, lrem = L - l0;
    const __amdgpu_buffer_rsrc_t rs_p = make_rsrc(
        p.P + (int64_t)n * p.p_bstride + (int64_t)r0 * L + l0, (int64_t)prow_lim * L - l0);
    const __amdgpu_buffer_rsrc_t rs_q = make_rsrc(
        p.Q + (int64_t)n * p.q_bstride + (int64_t)c0 * L + l0, (int64_t)qrow_lim * L - l0);
#pragma unroll
    for (int i = 0; i < PN; ++i) {
      if ((i * 4 + wave) * 64 * G < PSZ) {
        const bool ok = poff[i] >= 0 && pcol[i] < lrem;
        dma(rs_p, ok ? (unsigned)poff[i] * 4u : kOOB, Ps + (i * 4 + wave) * 64 * G);
      }
    }
#pragma unroll
    for (int i = 0; i < QN; ++i) {
      if ((i * 4 + wave) * 64 * G < QSZ) {
        const bool ok = qoff[i] >= 0 && qcol[i] < lrem;
        dma(rs_q, ok ? (unsigned)qoff[i] * 4u : kOOB, Qs + (i * 4 + wave) * 64 * G);
      }
    }
  };

  const int mi = wave & 1, nj = wave >> 1;
  floatx16 acc[NJ], acl[NJ];
#pragma unroll
  for (int t = 0; t < NJ; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = acl[t][i] = 0.f;
  // x3 products of one staged item (P rows at Ps, Q rows at Qs)
  auto x3_item = [&](const float *Ps, const float *Qs) {
    const float *pa = Ps + (mi * 32 + lo) * PITCH + 8 * hi;
    const float *qb = Qs + (nj * (CT / 2) + lo) * PITCH + 8 * hi;
#pragma unroll
    for (int s = 0; s < KC / 16; ++s) {
      uint4 ah, am, al, bh[NJ], bm[NJ], bl[NJ];
      wsp_planes(pa + 16 * s, ah, am, al);
#pragma unroll
      for (int t = 0; t < NJ; ++t) wsp_planes(qb + t * 32 * PITCH + 16 * s, bh[t], bm[t], bl[t]);
#pragma unroll
      for (int t = 0; t < NJ; ++t) {
        acc[t] = mfma_bf16(ah, bh[t], acc[t]);
        acl[t] = mfma_bf16(ah, bm[t], acl[t]);
        acl[t] = mfma_bf16(am, bh[t], acl[t]);
        acl[t] = mfma_bf16(ah, bl[t], acl[t]);
        acl[t] = mfma_bf16(am, bm[t], acl[t]);
        acl[t] = mfma_bf16(al, bh[t], acl[t]);
      }
    }
  };
  if (it0 < it1) stage(it0, Ps0, Qs0);
  __syncthreads();
  for (int it = it0; it < it1; ++it) {
    const bool odd = (it - it0) & 1;
    const float *Ps = odd ? Ps1 : Ps0;
    const float *Qs = odd ? Qs1 : Qs0;
    if (it + 1 < it1) stage(it + 1, odd ? Ps0 : Ps1, odd ? Qs0 : Qs1);
    if constexpr (X3) {
      x3_item(Ps, Qs);
      __syncthreads();  // retires this wave's LDS-DMA and publishes the next chunk
      continue;
    }
    const float *pa = Ps + (mi * 32 + lo) * PITCH + 4 * hi;
    const float *qb = Qs + (nj * (CT / 2) + lo) * PITCH + 4 * hi;
    // element-wise reads (merged into ds_read_b128 by the backend; a float4
    // load here loses the alias info that keeps the next chunk's LDS-DMA from
    // being waited on before these reads); k-block s+1 is read before the
    // MFMAs of k-block s.
    float a[2][4], b[2][NJ][4];
    auto ld = [&](int kb, int set) {
#pragma unroll
      for (int u = 0; u < 4; ++u) a[set][u] = pa[kb + u];
#pragma unroll
      for (int t = 0; t < NJ; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) b[set][t][u] = qb[t * 32 * PITCH + kb + u];
    };
    ld(0, 0);
#pragma unroll
    for (int s = 0; s < KC / 8; ++s) {
      if (s + 1 < KC / 8) ld((s + 1) * 8, (s + 1) & 1);
      const int c = s & 1;
#pragma unroll
      for (int t = 0; t < NJ; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[t] = mfma32(a[c][u], b[c][t][u], acc[t]);
      __builtin_amdgcn_sched_group_barrier(0x100, 1 + NJ, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4 * NJ, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // retires this wave's LDS-DMA and publishes the next chunk
  }
  float *dst = p.slab + (int64_t)split * p.R * p.C;
#pragma unroll
  for (int t = 0; t < NJ; ++t) {
    const int c = c0 + nj * (CT / 2) + t * 32 + lo;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = r0 + mi * 32 + (i & 3) + 8 * (i >> 2) + 4 * hi;
      if (row < p.R && c < p.C) dst[(int64_t)row * p.C + c] = X3 ? acc[t][i] + acl[t][i] : acc[t][i];
    }
  }
}

void plan_wgrad_sp(WgradParams &w) {
  w.CT = w.C <= 64 ? 64 : 128;
  const int KC = wgrad_sp_kc(w.CT);
  const int L = w.M * w.V;
  w.n_mtiles = (L + KC - 1) / KC;
  w.n_rtiles = (w.R + 63) / 64;
  w.n_jtiles = (w.C + w.CT - 1) / w.CT;
  const int tiles = w.n_rtiles * w.n_jtiles;
  w.S = std::max(1, std::min((512 + tiles - 1) / tiles, w.N * w.n_mtiles));
}

static hipError_t launch_wgrad_sp(const WgradParams &p, hipStream_t s) {
  if ((p.CT != 64 && p.CT != 128) || p.n_mtiles != (p.M * p.V + wgrad_sp_kc(p.CT) - 1) /
                                                       wgrad_sp_kc(p.CT))
    return hipErrorInvalidValue;
  const int64_t L = (int64_t)p.M * p.V;
  const bool x4 = L % 4 == 0 && p.p_bstride % 4 == 0 && p.q_bstride % 4 == 0 &&
                  ((uintptr_t)p.P & 15) == 0 && ((uintptr_t)p.Q & 15) == 0;
  const int nblk = p.n_rtiles * p.n_jtiles * p.S;
  const int KC = wgrad_sp_kc(p.CT);
  const size_t lds = sizeof(float) * 2 * (size_t)(64 + p.CT) * (KC + 4);
  const bool x3 = p.bf16 == 3;
  // (x3: the two-buffer schedule at two workgroups per CU; a deeper LDS-DMA ring at
  // one per CU measured 1% slower on cfg2, 4356-4375 vs 4403-4415 clips/s)
#define WSP_LAUNCH(CT, X4, X3) \
  hipLaunchKernelGGL((k_wgrad_sp<CT, X4, X3>), dim3(nblk), dim3(256), lds, s, p)
  if (p.CT == 64) {
    if (x4)
      { if (x3) WSP_LAUNCH(64, true, true); else WSP_LAUNCH(64, true, false); }
    else
      { if (x3) WSP_LAUNCH(64, false, true); else WSP_LAUNCH(64, false, false); }
  } else {
    if (x4)
      { if (x3) WSP_LAUNCH(128, true, true); else WSP_LAUNCH(128, true, false); }
    else
      { if (x3) WSP_LAUNCH(128, false, true); else WSP_LAUNCH(128, false, false); }
  }
#undef WSP_LAUNCH
  return hipGetLastError();
}

bool wgrad_sp_applies(const WgradParams &p) {
  return p.NQ == 1 && p.s_in == 1 && p.off == 0 && p.M == p.T_src;
}

hipError_t launch_wgrad(const WgradParams &p, hipStream_t s) {
  if (p.bf16 == 3 && wgrad_sp_applies(p)) return launch_wgrad_sp(p, s);  // x3 products
  if (p.bf16) return launch_wgrad_bf16(p, s);
  if (wgrad_sp_applies(p)) return launch_wgrad_sp(p, s);
  if (!wgrad_supported(p)) return hipErrorInvalidValue;
  const int nblk = p.n_rtiles * p.n_jtiles * p.S;
  const size_t lds = wgrad_lds_bytes(p);
  switch (p.NQ) {
    case 1:  // strided 1x1 (residual projection)
      hipLaunchKernelGGL((k_wgrad<1, 128>), dim3(nblk), dim3(256), lds, s, p);
      break;
    case 9:
      hipLaunchKernelGGL((k_wgrad<9, 192>), dim3(nblk), dim3(256), lds, s, p);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// Block = 32 consecutive outputs x 8 split groups (group g sums splits
// g, g+8, ... in fp64); the 8 partials are combined in a fixed order, so the
// result is deterministic.
__global__ __launch_bounds__(256) void k_slab_reduce(const float *slab, int S, int64_t n,
                                                     float *dst, int mode, int R, int K, int C) {
  __shared__ double red[8][33];
  const int o = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int64_t idx = (int64_t)blockIdx.x * 32 + o;
  double s = 0.0;
  if (idx < n) {
#pragma unroll 8
    for (int k = g; k < S; k += 8) s += slab[(int64_t)k * n + idx];
  }
  red[g][o] = s;
  __syncthreads();
  if (g != 0 || idx >= n) return;
#pragma unroll
  for (int j = 1; j < 8; ++j) s += red[j][o];
  int64_t d = idx;
  if (mode == 1) {  // idx = co*(K*C) + k*C + ci  ->  (k*R + co)*C + ci
    const int64_t KC = (int64_t)K * C;
    const int64_t co = idx / KC, rem = idx - co * KC;
    const int64_t k = rem / C, ci = rem - k * C;
    d = (k * R + co) * C + ci;
  }
  dst[d] = (float)s;
}

hipError_t launch_slab_reduce(const float *slab, int S, int64_t n, float *dst, int mode, int R,
                              int K, int C, hipStream_t s) {
  const int nb = (int)((n + 31) / 32);
  hipLaunchKernelGGL(k_slab_reduce, dim3(nb), dim3(256), 0, s, slab, S, n, dst, mode, R, K, C);
  return hipGetLastError();
}

}  // namespace stgcn
