// What the convolution translation units share (internal; include/nsm.h is the
// public C ABI): included by nsm_conv.hip (fp32 GEMMs and Winograd),
// nsm_conv_h2.hip (the f16 LDS-DMA GEMMs on h2 operands) and nsm_conv_bf16.hip /
// nsm_conv_f16.hip (the 16-bit convolutions, one unit per format). The
// epilogues more than one GEMM family applies, bf16 operand images, the
// format-independent LDS-DMA helpers, the tile plans, and the functions one
// unit calls in another.
#pragma once
#include <algorithm>
#include <type_traits>

#include "nsm_common.h"

namespace nsm {

constexpr int BK = 32;
constexpr int LDK = BK + 4;

// Branch-free operand loads: buffer_load_dwordx4 through a per-block resource
// descriptor whose base sits just below the block's lowest address; an
// invalid lane gets an offset past num_records and the hardware returns 0
// (zero padding / tails without exec-mask branches).
constexpr uint32_t OOB = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const float* base, long long floats) {
  long long bytes = floats * 4;
  if (bytes > 0x7FFFFFFFll) bytes = 0x7FFFFFFFll;
  if (bytes < 0) bytes = 0;
  return __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 bload4(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}

// ---- bf16 operand images (nsm_conv_split.inc, nsm_conv_s16.inc) -----------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int BKB = 64;
constexpr int LDKB = BKB + 8;

template <int R>
struct KMStride {  // bf16 elements per KM row: (row dwords) = 16 (mod 32)
  static constexpr int value = R == 32 ? 96 : R + 32;
};

// fragment of k-step s (0..3) for rows rb..rb+31 of the tile
template <bool KM, int R>
__device__ __forceinline__ bf16x8 read_frag_b(const bf16_t* S, int rb, int lane, int s) {
  if constexpr (!KM) {
    const int r = lane & 31, h = lane >> 5;
    return __builtin_bit_cast(bf16x8, *(const u32x4*)&S[(rb + r) * LDKB + 16 * s + 8 * h]);
  } else {
    constexpr int KMS = KMStride<R>::value;
    const int h = lane >> 5, g16 = (lane >> 4) & 1, q = (lane >> 2) & 3, p = lane & 3;
    const bf16_t* a = S + (16 * s + 8 * h + q) * KMS + rb + 16 * g16 + 4 * p;
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a + 4 * KMS));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return __builtin_bit_cast(bf16x8, v);
  }
}

// ---- LDS-DMA helpers of the 16-bit GEMMs (nsm_conv_s16_dma.inc, nsm_conv_h2.inc) ----
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc_b(const bf16_t* base, long long elems) {
  long long bytes = elems * 2;
  if (bytes > 0x7FFFFFFFll) bytes = 0x7FFFFFFFll;
  if (bytes < 0) bytes = 0;
  return __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, (int)bytes, 0x00020000);
}
constexpr int DBK = 64;
// 16-B chunk XOR of MK row `row` for BK-wide rows: spreads the rows that share
// a 256-B bank line ((128 / BK) consecutive rows) over distinct chunks
template <int BK = DBK>
__device__ __forceinline__ int dswz(int row) {
  return (row / (128 / BK)) & (BK / 8 - 1);
}

typedef __attribute__((address_space(3))) void lds_void;

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, const bf16_t* dst, uint32_t off) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void*)dst, 16, off, 0, 0, 0);
}
template <int N>
__device__ __forceinline__ void vm_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// every wave's LDS reads done (lgkmcnt) and, with its own DMAs retired by
// vm_wait before, after this barrier a retired stage is readable and the
// stage read in the previous iteration is free to refill
__device__ __forceinline__ void dma_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int LPT, int MAXAHEAD>
__device__ __forceinline__ void wait_retire(int ahead) {
  // retire the oldest tile, leave `ahead` (<= MAXAHEAD) younger tiles (LPT DMAs
  // each) in flight
  static_assert(MAXAHEAD * LPT <= 63, "vmcnt range");
  if constexpr (MAXAHEAD >= 1) {
    if (ahead >= MAXAHEAD) {
      vm_wait<MAXAHEAD * LPT>();
      return;
    }
    wait_retire<LPT, MAXAHEAD - 1>(ahead);
  } else {
    vm_wait<0>();
  }
}

// 16-B chunk XOR of KM pixel row k (weight-gradient images)
template <int R>
__device__ __forceinline__ int kmswz(int k) {
  // 16-B chunk XOR for pixel row k of a [64][R] image (rows of 2R bytes)
  if constexpr (2 * R >= 256) return 4 * (k & 3);
  else if constexpr (2 * R == 128) return 4 * ((k >> 1) & 1);
  else return 0;
}

// one K-tile's DMA instruction j of this wave (A's first, then B's)
template <class AL, class BL>
__device__ __forceinline__ void dma_one(const AL& a, const BL& b, const typename AL::P& ap,
                                        const typename BL::P& bp, const bf16_t* stage, int a_el,
                                        int wid, int j) {
  if (j < AL::NI) a.one(ap, stage, wid, j);
  else b.one(bp, stage + a_el, wid, j - AL::NI);
}

__device__ __forceinline__ void lgkm_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
template <int N>
__device__ __forceinline__ void lgkm_fence_n() {
  static_assert(N >= 0 && N <= 15, "lgkmcnt range");
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}

// XCD-aware block order: blocks are dealt round-robin over the 8 XCDs, so
// dispatch slot L runs on XCD L % 8; slot L becomes logical block
// (L % 8) * (total / 8) + L / 8, each XCD a contiguous range of them, so the
// blocks that share an operand tile share one L2. mode 1: M-blocks fastest
// (batched / split-K grids: whole Winograd components / K-splits per XCD);
// mode 2: N-blocks fastest (2-D grids: the N-blocks reading one activation
// panel run together on one XCD, which then fetches the panel once)
__device__ __forceinline__ void xcd_block_order(int& bx, int& by, int& bz, int mode) {
  const unsigned gx = gridDim.x, gy = gridDim.y, total = gx * gy * gridDim.z;
  const unsigned L = bx + gx * (by + gy * bz);
  const unsigned lg = (L & 7) * (total >> 3) + (L >> 3);
  if (mode == 2) {
    by = lg % gy;
    bx = (lg / gy) % gx;
  } else {
    bx = lg % gx;
    by = (lg / gx) % gy;
  }
  bz = lg / (gx * gy);
}

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------
// Epilogues. acc[tm][tn] register i holds C[row][col] with
//   col = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5).
// ---------------------------------------------------------------------------
struct EpiCtx {
  int m0, n0;  // block origin
  int mb, nb;  // this wave's tile origin
  int wm, wn, lane;
  float* lds;  // the GEMM's LDS array (free after the main loop)
  int mblk;    // M-block index (BN-partial row)
  int zslab;   // split-K / batch slab of EpiSlab (blockIdx.z unless remapped)
};

struct EpiStoreP {
  float* y;
  int ldy;
  const float* bias;
  float* stats;  // optional BN partials [gridDim.x][2][N]: {sum, M2 about block mean}
  long long bstride;  // batched GEMM (Winograd): output offset per blockIdx.z
  // optional eval-mode BN + LeakyReLU (+ skip) on the stored value:
  // y = lrelu((acc + bias) * act_scale + act_shift, slope) (+ res)
  const float* act_scale;
  const float* act_shift;
  float slope;
  const float* res;
  int ldres;
  int vec;  // 16-B row stores staged through LDS (NSM_F32_EPI_VEC=0: 4-byte stores)
};
struct EpiStore {
  using P = EpiStoreP;
  template <int TM, int TN, int WM, int WN>
  __device__ static void apply(const P& e, f32x16 (&acc)[TM][TN], const EpiCtx& cx, int M, int N,
                               int) {
    const int col = cx.lane & 31, h = cx.lane >> 5;
    float* yb = e.y + (size_t)cx.zslab * e.bstride;  // store paths run with zsplit == 1
    float bv[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      int n = cx.nb + tn * 32 + col;
      bv[tn] = (e.bias && n < N) ? e.bias[n] : 0.f;
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[tm][tn][i] += bv[tn];
    }
    if (e.vec && (e.ldy & 3) == 0 && (((uintptr_t)yb) & 15) == 0 &&
        (!e.res || ((e.ldres & 3) == 0 && (((uintptr_t)e.res) & 15) == 0))) {
      // each wave stages its tile as rows in LDS (stride WC + 4 floats: the two
      // row halves of a store land on different banks) and writes 16-B chunks
      constexpr int WR = TM * 32, WC = TN * 32, WCP = WC + 4, CPR = WC / 4;
      float* reg = cx.lds + (cx.wm * WN + cx.wn) * (WR * WCP);
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            reg[(tm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * WCP + tn * 32 + col] = acc[tm][tn][i];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int it = 0; it < WR * CPR / 64; ++it) {
        const int q = it * 64 + cx.lane, r = q / CPR, cc = q - r * CPR;
        const int m = cx.mb + r, n = cx.nb + cc * 4;
        if (m >= M || n >= N) continue;
        f32x4 v = *(const f32x4*)&reg[r * WCP + cc * 4];
        if (e.act_scale) {
          const f32x4 a = *(const f32x4*)(e.act_scale + n), b = *(const f32x4*)(e.act_shift + n);
          v = v * a + b;
          v = f32x4{lrelu(v.x, e.slope), lrelu(v.y, e.slope), lrelu(v.z, e.slope),
                    lrelu(v.w, e.slope)};
          if (e.res) v += *(const f32x4*)(e.res + (size_t)m * e.ldres + n);
        }
        *(f32x4*)(yb + (size_t)m * e.ldy + n) = v;
      }
      if (!e.stats) return;
      __syncthreads();  // stats_only reuses the LDS
      stats_only<TM, TN, WM, WN>(e, acc, cx, M, N);
      return;
    }
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      int n = cx.nb + tn * 32 + col;
      if (n >= N) continue;
      const float asc = e.act_scale ? e.act_scale[n] : 0.f;
      const float ash = e.act_scale ? e.act_shift[n] : 0.f;
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          int m = cx.mb + tm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
          if (m >= M) continue;
          float v = acc[tm][tn][i];
          if (e.act_scale) {
            v = lrelu(v * asc + ash, e.slope);
            if (e.res) v += e.res[(size_t)m * e.ldres + n];
          }
          yb[(size_t)m * e.ldy + n] = v;
        }
      }
    }
    if (!e.stats) return;
    stats_only<TM, TN, WM, WN>(e, acc, cx, M, N);
  }
  // fused BatchNorm batch statistics of this block's rows (two-pass); also
  // used by the bf16 store epilogue on its rounded values
  // RPP: rows per partial; a block of WM*TM*32 rows writes (WM*TM*32)/RPP
  // partial rows, each over its own group of M-waves
  template <int TM, int TN, int WM, int WN, int RPP = WM * TM * 32>
  __device__ static void stats_only(const P& e, f32x16 (&acc)[TM][TN], const EpiCtx& cx, int M,
                                    int N) {
    const int col = cx.lane & 31, h = cx.lane >> 5;
    constexpr int BN = WN * TN * 32;
    constexpr int G = (WM * TM * 32) / RPP, WG = WM / G;
    static_assert(G >= 1 && G * RPP == WM * TM * 32 && WG * G == WM, "partial groups");
    float* red = cx.lds;  // [WM][BN]
    const int g = cx.wm / WG, w0 = g * WG;
    const int cnt = min(M - (cx.m0 + g * RPP), RPP);
    float s[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      float t = 0.f;
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          int m = cx.mb + tm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
          t += (m < M) ? acc[tm][tn][i] : 0.f;
        }
      t += __shfl_xor(t, 32, 64);
      s[tn] = t;
    }
    if (h == 0)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) red[cx.wm * BN + cx.wn * TN * 32 + tn * 32 + col] = s[tn];
    __syncthreads();
    float mean[TN], tot[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < WG; ++w) t += red[(w0 + w) * BN + cx.wn * TN * 32 + tn * 32 + col];
      tot[tn] = t;
      mean[tn] = t / (float)cnt;
    }
    __syncthreads();
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      float t = 0.f;
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          int m = cx.mb + tm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
          float d = acc[tm][tn][i] - mean[tn];
          t += (m < M) ? d * d : 0.f;
        }
      t += __shfl_xor(t, 32, 64);
      s[tn] = t;
    }
    if (h == 0)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) red[cx.wm * BN + cx.wn * TN * 32 + tn * 32 + col] = s[tn];
    __syncthreads();
    if (cx.wm == w0 && h == 0 && cnt > 0) {
      float* pr = e.stats + ((size_t)cx.mblk * G + g) * 2 * N;
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        int n = cx.nb + tn * 32 + col;
        if (n >= N) continue;
        float q = 0.f;
#pragma unroll
        for (int w = 0; w < WG; ++w) q += red[(w0 + w) * BN + cx.wn * TN * 32 + tn * 32 + col];
        pr[n] = tot[tn];
        pr[N + n] = q;
      }
    }
  }
};

// BN-backward epilogue of the 1x1 input-gradient GEMM of a DoubleConv
// (g = dA1 = dY2 W2, the gradient wrt the activated output of the block's
// first BN; Unetmodel.py:22-26). With y = Y1 (that BN's input):
//   dz = g * lrelu'(y*scale + shift) * mask[b][c]
// mode 0: partials {sum dz, sum dz*(y-mean)*invstd} per row chunk (the
//         nsm_bn_bwd_reduce format; chunk = nsm_conv_stat_rows rows), g not stored
// mode 1: mode 0 and g stored (nsm_bn_bwd_apply then reads it)
// mode 2: dy = k1*dz + k2*(y-mean) + k3 stored (coef from nsm_bn_bwd_finalize)
// Modes 0 then 2 run the same GEMM twice, so dA1 never goes through HBM.
struct BnBwdEpiP {
  void* out;
  int ldo;
  const void* y;
  int ldy;
  const float* scale;
  const float* shift;
  const float* mean;
  const float* invstd;
  const float* coef;
  const float* mask;  // [B][N] or null
  FastDiv fdHW;
  float slope;
  float* partial;  // [nchunk][2][N]
  int mode;
  uint32_t* amax = nullptr;  // mode 2 (fp32): max|dy| written (an h2 scale source)
  uint32_t* k1dz = nullptr;  // modes 0/1 (fp32): max|scale * dz| (the dy bound's k1 term)
};

__device__ __forceinline__ f32x4 lrelu_grad_v4(f32x4 z, float slope) {
  return f32x4{lrelu_grad(z.x, slope), lrelu_grad(z.y, slope), lrelu_grad(z.z, slope),
               lrelu_grad(z.w, slope)};
}
__device__ __forceinline__ f32x4 shfl_xor_v4(f32x4 v, int o) {
  return f32x4{__shfl_xor(v.x, o, 64), __shfl_xor(v.y, o, 64), __shfl_xor(v.z, o, 64),
               __shfl_xor(v.w, o, 64)};
}

// Each wave stages its accumulator tile as rows in LDS (row stride WC + 4
// floats: the two row halves of a store land on different banks), then every
// lane keeps ONE 4-column group and walks the rows with 16-B accesses: all Y1
// loads of the lane issue back to back, the accumulators are dead by then, so
// the epilogue adds no register pressure to the GEMM loop.
struct EpiBnBwd {
  using P = BnBwdEpiP;
  // Y1 rows of the wave tile, loaded before the GEMM's K loop (gemm_h2_kernel:
  // with the short K of most 1x1 input gradients the epilogue's Y1 read is the
  // kernel's main traffic; issued first, it overlaps the operand DMA instead of
  // following the MFMAs). Lane layout of apply's loop: one 4-column group
  // (lane % CPR) per lane, rows (it * 64 + lane) / CPR.
  template <int TM, int TN>
  struct PreT {
    static constexpr int NIT = TM * 32 * (TN * 32 / 4) / 64;
    f32x4 yv[NIT];
  };
  template <int TM, int TN, int WM, int WN>
  __device__ static void prefetch(const P& e, PreT<TM, TN>& pre, int mb, int nb, int lane, int M,
                                  int N) {
    constexpr int CPR = TN * 32 / 4;
    const int n = nb + (lane % CPR) * 4, nc = n < N ? n : 0;
    const float* __restrict__ Y = (const float*)e.y;
#pragma unroll
    for (int it = 0; it < PreT<TM, TN>::NIT; ++it) {
      const int m = min(mb + (it * 64 + lane) / CPR, M - 1);
      pre.yv[it] = *(const f32x4*)(Y + (size_t)m * e.ldy + nc);
    }
  }
  // LDS of the h2 GEMMs' epilogue (gemm_h2_kernel): the staged wave tiles, then
  // the [WM][2][BNT] partial rows
  template <int TM, int TN, int WM, int WN>
  static constexpr int lds_bytes() {
    constexpr int a = WM * WN * TM * 32 * (TN * 32 + 4) * 4, b = WM * 2 * WN * TN * 32 * 4;
    return a > b ? a : b;
  }
  template <int TM, int TN, int WM, int WN>
  __device__ static void apply(const P& e, f32x16 (&acc)[TM][TN], const EpiCtx& cx, int M, int N,
                               int) {
    apply_impl<TM, TN, WM, WN>(e, acc, cx, M, N, nullptr);
  }
  template <int TM, int TN, int WM, int WN>
  __device__ static void apply_pre(const P& e, f32x16 (&acc)[TM][TN], const EpiCtx& cx, int M,
                                   int N, const PreT<TM, TN>& pre) {
    apply_impl<TM, TN, WM, WN>(e, acc, cx, M, N, &pre);
  }
  template <int TM, int TN, int WM, int WN>
  __device__ static void apply_impl(const P& e, f32x16 (&acc)[TM][TN], const EpiCtx& cx, int M,
                                    int N, const PreT<TM, TN>* pre) {
    const int col = cx.lane & 31, h = cx.lane >> 5;
    constexpr int BNT = WN * TN * 32, WR = TM * 32, WC = TN * 32, WCP = WC + 4;
    constexpr int CPR = WC / 4;  // 16-B chunks per row
    constexpr int NIT = WR * CPR / 64;
    static_assert(64 % CPR == 0, "a lane keeps one column group");
    float* reg = cx.lds + (cx.wm * WN + cx.wn) * (WR * WCP);
    __syncthreads();  // the GEMM's last LDS reads are done everywhere
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          reg[(tm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * WCP + tn * 32 + col] = acc[tm][tn][i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float* __restrict__ Y = (const float*)e.y;
    float* __restrict__ O = (float*)e.out;
    const float* __restrict__ mk = e.mask;
    const bool red = e.mode != 2;
    const int cc = cx.lane % CPR, n = cx.nb + cc * 4;
    const bool nok = n < N;
    const int nc = nok ? n : 0;
    f32x4 yv[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if (pre) {
        yv[it] = pre->yv[it];
      } else {
        const int m = min(cx.mb + (it * 64 + cx.lane) / CPR, M - 1);
        yv[it] = *(const f32x4*)(Y + (size_t)m * e.ldy + nc);
      }
    }
    const f32x4 sc = *(const f32x4*)(e.scale + nc), sh = *(const f32x4*)(e.shift + nc),
                mu = *(const f32x4*)(e.mean + nc);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 is = red ? *(const f32x4*)(e.invstd + nc) : zero;
    const f32x4 k1 = red ? zero : *(const f32x4*)(e.coef + nc),
                k2 = red ? zero : *(const f32x4*)(e.coef + N + nc),
                k3 = red ? zero : *(const f32x4*)(e.coef + 2 * N + nc);
    f32x4 s1 = zero, s2 = zero;
    uint32_t am = 0;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int r = (it * 64 + cx.lane) / CPR, m = cx.mb + r;
      const bool ok = m < M && nok;
      const f32x4 g = *(const f32x4*)&reg[r * WCP + cc * 4], v = yv[it];
      f32x4 dz = g * lrelu_grad_v4(v * sc + sh, e.slope);
      if (mk) dz = dz * *(const f32x4*)(mk + (size_t)fdiv((uint32_t)min(m, M - 1), e.fdHW) * N + nc);
      if (!red) {
        if (ok) {
          const f32x4 d = k1 * dz + k2 * (v - mu) + k3;
          *(f32x4*)(O + (size_t)m * e.ldo + n) = d;
          amax_fold(am, d);
        }
      } else if (ok) {
        s1 += dz;
        s2 += dz * ((v - mu) * is);
        if (e.mode == 1) *(f32x4*)(O + (size_t)m * e.ldo + n) = g;
        if (e.k1dz) amax_fold(am, sc * dz);
      }
    }
    if (!red) {
      amax_flush(am, e.amax);
      return;
    }
    amax_flush(am, e.k1dz);
#pragma unroll
    for (int o = CPR; o < 64; o <<= 1) {
      s1 += shfl_xor_v4(s1, o);
      s2 += shfl_xor_v4(s2, o);
    }
    // one partial row per block (RPP = BM = nsm_conv_stat_rows): the waves of
    // one column range meet in LDS, fixed order
    __syncthreads();
    float* lds = cx.lds;  // [WM][2][BNT]
    if (cx.lane < CPR) {
      *(f32x4*)(lds + (cx.wm * 2) * BNT + cx.wn * WC + cc * 4) = s1;
      *(f32x4*)(lds + (cx.wm * 2 + 1) * BNT + cx.wn * WC + cc * 4) = s2;
    }
    __syncthreads();
    if (cx.wm == 0) {
      float* pr = e.partial + (size_t)cx.mblk * 2 * N;
      for (int j = cx.lane; j < 2 * WC; j += 64) {
        const int k = j / WC, c = j - k * WC, nn = cx.nb + c;
        if (nn >= N) continue;
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < WM; ++w) t += lds[(w * 2 + k) * BNT + cx.wn * WC + c];
        pr[k * N + nn] = t;
      }
    }
  }
};

struct EpiSlabP {
  float* ws;
  int vec;  // EpiSlabV: 16-B row stores staged through LDS
};
struct EpiSlab {
  using P = EpiSlabP;
  template <int TM, int TN, int WM, int WN>
  __device__ static void apply(const P& e, f32x16 (&acc)[TM][TN], const EpiCtx& cx, int M, int N,
                               int split) {
    const int col = cx.lane & 31, h = cx.lane >> 5;
    const int mb = cx.mb, nb = cx.nb;
    float* out = e.ws + (size_t)cx.zslab * M * N;  // slab per (batch, split)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      int n = nb + tn * 32 + col;
      if (n >= N) continue;
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          int m = mb + tm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
          if (m < M) out[(size_t)m * N + n] = acc[tm][tn][i];
        }
      }
    }
  }
};

// ---- host side ---------------------------------------------------------------
// NSM_SPLIT_XCD=0: dispatch order as launched (no XCD-contiguous remap)
inline bool split_xcd() { static const bool v = env_flag("NSM_SPLIT_XCD", true); return v; }

inline int cu_count() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    return v;
  }();
  return n;
}

inline int conv_fwd_bm(long long M, int N) {
  long long mb128 = ceil_div(M, 128);
  if (N >= 128) return mb128 * ceil_div(N, 128) >= 512 ? 128 : 64;
  if (N >= 64) return mb128 * ceil_div(N, 64) >= 512 ? 128 : 64;
  return mb128 >= 512 ? 128 : 64;
}
struct WgradPlan {
  int BM, BN, splits, kchunk;
  size_t ws_floats;
};


// Bounds of the Winograd transforms, (max_i sum_j |T_ij|)^2 rounded up:
// which 0 = the input transform B^T d B, 1 = the output-gradient transform
// A dY A^T, 2 = the filter transform G g G^T. max|transform| <= beta * max|in|
// (the h2 operands' scale source, nsm_conv_h2.inc)
__host__ __device__ constexpr float wino_beta(int tile, int which) {
  return which == 0   ? (tile == 6 ? 225.f : tile == 4 ? 49.f : 4.f)
         : which == 1 ? (tile == 6 ? 3969.f : tile == 4 ? 225.f : 4.f)
                      : (tile == 6 ? 1.5625f : tile == 4 ? 3.5f : 2.25f);
}

// ---- Winograd host side: tile in {2, 4} selects F(2x2,3x3) / F(4x4,3x3) -------
struct WinoGeom {
  int m, alpha2, TH, TW;
  long long T;
};

inline bool wino_geom(int tile, int B, int H, int W, WinoGeom& g) {
  if (tile != 2 && tile != 4 && tile != 6) return false;
  g.m = tile;
  g.alpha2 = (tile + 2) * (tile + 2);
  g.TH = (H + tile - 1) / tile;
  g.TW = (W + tile - 1) / tile;
  g.T = (long long)B * g.TH * g.TW;
  return B > 0 && H > 0 && W > 0 && g.T < (1ll << 30);
}

struct WinoWgradPlan {
  int BM, BN, splits, kchunk;
  size_t slab_floats, dm_floats;
};


// nsm_conv.hip (Winograd)
WinoWgradPlan plan_wino_wgrad(long long T, int cin_p, int cout_p, int nb);
int wgrad_wino_finish(float* slab, const WinoWgradPlan& pl, int nb, int M, int N, int cin, int cout,
                      int tile, float* dw, hipStream_t s);
// nsm_conv_h2.hip: the bf16 path's Winograd GEMMs on single-plane f16 operands
int wino_gemm_f16(const bf16_t* V, const bf16_t* U, long long T, int cin_p, int cout_p, int nb,
                  float* Mb, H2Scale sv, H2Scale su, hipStream_t s, bool o16 = false,
                  int* m16e = nullptr);
WinoWgradPlan plan_wino_wgrad_f16(long long T, int cin_p, int cout_p, int nb);
int wino_wgrad_gemm_f16(const bf16_t* dM, const bf16_t* V, long long T, int cin_p, int cout_p,
                        int nb, int BM, int BN, int kchunk, int splits, float* slab, H2Scale sdm,
                        H2Scale sv, hipStream_t s);

// nsm_conv.hip
int conv_fwd_bm_f(long long M, int N);
WgradPlan plan_wgrad(int B, int H, int W, int cin_p, int cout_p, int ksize);
int wgrad_finish(float* ws, const WgradPlan& pl, int M, int N, int cin_p, int taps, int cin,
                 int cout, float* dw, hipStream_t s);
// the fp32 cases of nsm_conv_fwd_act and nsm_conv1x1_dgrad_bnbwd (nsm_conv_bf16.hip)
int conv_fwd_act_f32(const float* x, int ldx, int B, int H, int W, int cin_p, const float* wpk,
                     const float* bias, int cout_p, int ksize, float* y, int ldy,
                     const float* act_scale, const float* act_shift, float slope, const float* res,
                     int ldres, hipStream_t s);
int conv1x1_dgrad_bnbwd_f32(const float* dy2, int lddy2, int B, int H, int W, int cop,
                            const float* w2d, int cip, const BnBwdEpiP& ep,
                            const uint32_t* amax_dy2, const uint32_t* amax_w, hipStream_t s);
// nsm_conv_f16.hip: the f16 cases of the same two entries
int conv_fwd_act_f16(const void* x, int ldx, int B, int H, int W, int cin_p, const void* wpk,
                     const float* bias, int cout_p, int ksize, void* y, int ldy,
                     const float* act_scale, const float* act_shift, float slope, const void* res,
                     int ldres, hipStream_t s);
int conv1x1_dgrad_bnbwd_f16(const void* dy2, int lddy2, int B, int H, int W, int cop,
                            const void* w2d, int cip, const BnBwdEpiP& ep, hipStream_t s);

}  // namespace nsm
