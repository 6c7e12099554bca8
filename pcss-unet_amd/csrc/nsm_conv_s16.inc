// 16-bit-storage MFMA implicit-GEMM convolutions: bf16 (BASELINE config 3)
// and f16 (the fp16-autocast mode). This body is compiled twice, once per
// translation unit: nsm_conv_bf16.hip includes it in namespace nsm_bf (bf16),
// nsm_conv_f16.hip in namespace nsm_h (f16), where nsm_fmt_f16.h shadows the
// format helpers this body calls (bf_lo / bf_hi / pack_bf2 / round_bf /
// s16_bits / ld1 / ld8 / st8 and the mfma_s16_* wrappers). Both include
// nsm_conv.h first (epilogue contexts, bf16 operand images, LDS-DMA helpers,
// tile plans); the C entries follow the inclusion in each.
//
// Storage bf16 (activations, packed weights, activation gradients), products
// bf16 x bf16 on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; BN
// statistics, weight gradients, optimizer state stay fp32.
//
// Operand maps (32x32x16 bf16): lane l (r = l&31, h = l>>5) holds
// A[row r][k = 8h + j] and B[k = 8h + j][col r], j = 0..7, per 16-deep k-step;
// C/D as the f32 form. A slab is BKB = 64 bf16 of K (4 k-steps).
//   MK image [rows][BKB+8]: one ds_read_b128 per fragment (144-B rows, the
//       same conflict-free geometry as the f32 kernel's [rows][36] floats).
//   KM image [BKB][rows+pad] (weight gradient: K = pixels is the row index):
//       two ds_read_b64_tr_b16 per fragment, the hardware transpose read
//       (per 16-lane group a 4-row x 16-column block delivered column-major).
//       Row stride = 16 (mod 32) dwords: the 4 rows of a read land on disjoint
//       bank quarters.
// Global loads are 16 B (8 bf16) per lane through the same buffer-descriptor
// OOB zero-fill as the f32 loaders.

// bf16x8, BKB, LDKB, KMStride, read_frag_b, make_rsrc_b: nsm_conv.h

__device__ __forceinline__ u32x4 bload16(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}

// 8 bf16 -> lrelu(v*sc+sh, slope)*mask -> 8 bf16 (channels c..c+7)
__device__ __forceinline__ u32x4 prologue8(u32x4 v, const float* scale, const float* shift,
                                           const float* mask, int c, float slope, bool mask_on) {
  const f32x4 s0 = *(const f32x4*)(scale + c), s1 = *(const f32x4*)(scale + c + 4);
  const f32x4 h0 = *(const f32x4*)(shift + c), h1 = *(const f32x4*)(shift + c + 4);
  f32x4 m0 = *(const f32x4*)(mask + c), m1 = *(const f32x4*)(mask + c + 4);
  if (!mask_on) m0 = m1 = f32x4{1.f, 1.f, 1.f, 1.f};
  u32x4 o;
  o.x = pack_bf2(lrelu(bf_lo(v.x) * s0.x + h0.x, slope) * m0.x,
                 lrelu(bf_hi(v.x) * s0.y + h0.y, slope) * m0.y);
  o.y = pack_bf2(lrelu(bf_lo(v.y) * s0.z + h0.z, slope) * m0.z,
                 lrelu(bf_hi(v.y) * s0.w + h0.w, slope) * m0.w);
  o.z = pack_bf2(lrelu(bf_lo(v.z) * s1.x + h1.x, slope) * m1.x,
                 lrelu(bf_hi(v.z) * s1.y + h1.y, slope) * m1.y);
  o.w = pack_bf2(lrelu(bf_lo(v.w) * s1.z + h1.z, slope) * m1.z,
                 lrelu(bf_hi(v.w) * s1.w + h1.w, slope) * m1.w);
  return o;
}

// ConvActPB, RowsKPB, PixRowsPB and their LDS-DMA loaders
#include "nsm_conv_s16_loaders.inc"

template <int R, int NT, bool PRO>
struct ConvActLoaderB {
  static constexpr bool KM = false;
  static constexpr int CPR = BKB / 8;
  static constexpr int NPT = R * CPR / NT;
  static constexpr int RSTEP = NT / CPR;
  static constexpr int LDS_ELEMS = R * LDKB;
  static_assert(NPT >= 1 && NPT * RSTEP == R, "loader shape");
  __amdgpu_buffer_rsrc_t rsrc;
  int rel[NPT], py[NPT], px[NPT], pb[NPT];
  int kc, row0, k;

  __device__ void init(const ConvActPB& p, int m0, int kbeg, int tid, int) {
    kc = (tid % CPR) * 8;
    row0 = tid / CPR;
    const int base_pix = max(0, m0 - p.W - 1);
    rsrc = make_rsrc_b(p.x + (size_t)base_pix * p.ld, (long long)(p.M - base_pix) * p.ld);
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      int q = m0 + row0 + i * RSTEP;
      bool v = q < p.M;
      q = v ? q : 0;
      int t = (int)fdiv((uint32_t)q, p.fdW);
      int xx = q - t * p.W;
      int b = (int)fdiv((uint32_t)t, p.fdH);
      int yy = t - b * p.H;
      rel[i] = q - base_pix;
      px[i] = xx;
      py[i] = v ? yy : -0x40000000;
      pb[i] = b;
    }
    k = kbeg + kc;
  }
  __device__ void load(const ConvActPB& p, u32x4* r) const {
    const int tap = (int)fdiv((uint32_t)k, p.fdC);
    const int c = k - tap * p.cin;
    const bool kok = k < p.K;
    int dy = 0, dx = 0;
    if (p.ksize == 3) {
      dy = tap / 3 - 1;
      dx = tap - (tap / 3) * 3 - 1;
    }
    const int shift = dy * p.W + dx;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      int yy = py[i] + dy, xx = px[i] + dx;
      bool ok = kok & ((unsigned)yy < (unsigned)p.H) & ((unsigned)xx < (unsigned)p.W);
      uint32_t off = ((uint32_t)((rel[i] + shift) * p.ld + c) * 2u) | (ok ? 0u : OOB);
      u32x4 v = bload16(rsrc, off);
      if constexpr (PRO) {
        const int cc = kok ? c : 0;
        u32x4 a = prologue8(v, p.scale, p.shift, p.mask + (size_t)pb[i] * p.mask_ld, cc, p.slope,
                            p.mask_on);
        v = ok ? a : u32x4{0u, 0u, 0u, 0u};
      }
      r[i] = v;
    }
  }
  __device__ void advance(const ConvActPB&) { k += BKB; }
  __device__ void store(bf16_t* S, const u32x4* r) const {
#pragma unroll
    for (int i = 0; i < NPT; ++i) *(u32x4*)&S[(row0 + i * RSTEP) * LDKB + kc] = r[i];
  }
};

template <int R, int NT>
struct RowsKLoaderB {
  static constexpr bool KM = false;
  static constexpr int CPR = BKB / 8;
  static constexpr int NPT = R * CPR / NT;
  static constexpr int RSTEP = NT / CPR;
  static constexpr int LDS_ELEMS = R * LDKB;
  static_assert(NPT >= 1 && NPT * RSTEP == R, "loader shape");
  __amdgpu_buffer_rsrc_t rsrc;
  int kc, row0, k0, n0;

  __device__ void init(const RowsKPB& p, int n0_, int kbeg, int tid, int) {
    kc = (tid % CPR) * 8;
    row0 = tid / CPR;
    k0 = kbeg;
    n0 = n0_;
    rsrc = make_rsrc_b(p.w + (size_t)n0 * p.ldw, (long long)(p.nrows - n0) * p.ldw);
  }
  __device__ void load(const RowsKPB& p, u32x4* r) const {
    const bool kok = k0 + kc < p.K;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      int row = row0 + i * RSTEP;
      uint32_t off = ((uint32_t)(row * p.ldw + k0 + kc) * 2u) |
                     ((kok & (n0 + row < p.nrows)) ? 0u : OOB);
      r[i] = bload16(rsrc, off);
    }
  }
  __device__ void advance(const RowsKPB&) { k0 += BKB; }
  __device__ void store(bf16_t* S, const u32x4* r) const {
#pragma unroll
    for (int i = 0; i < NPT; ++i) *(u32x4*)&S[(row0 + i * RSTEP) * LDKB + kc] = r[i];
  }
};

template <int R, int NT, bool SHIFT, bool PRO>
struct PixRowsLoaderB {
  static constexpr bool KM = true;
  static constexpr int C8 = R / 8;
  static constexpr int KSTEP = NT / C8;
  static constexpr int NPT = BKB / KSTEP;
  static constexpr int KMS = KMStride<R>::value;
  static constexpr int LDS_ELEMS = BKB * KMS;
  static_assert(NPT >= 1 && NPT * KSTEP == BKB && KSTEP * C8 == NT, "loader shape");
  __amdgpu_buffer_rsrc_t rsrc;
  int col, c8o, krow0, k0, kend, dy, dx, base_pix;
  bool colok;

  __device__ void init(const PixRowsPB& p, int off, int kbeg, int kend_, int tid, int) {
    int c8 = tid % C8;
    c8o = c8 * 8;
    krow0 = tid / C8;
    // this thread's column and, for the shifted operand, its own tap (an N
    // tile may span several taps when BN > Cin)
    int tap = 0, c = off + c8 * 8;
    if (p.cin > 0) {
      tap = c / p.cin;
      c -= tap * p.cin;
    }
    col = c;
    colok = col < p.ncols && (p.cin == 0 || tap < p.ksize * p.ksize);
    dy = dx = 0;
    if (SHIFT && p.ksize == 3) {
      dy = tap / 3 - 1;
      dx = tap % 3 - 1;
    }
    k0 = kbeg;
    kend = kend_;
    base_pix = max(0, kbeg - p.W - 1);
    rsrc = make_rsrc_b(p.x + (size_t)base_pix * p.ld, (long long)(p.M - base_pix) * p.ld);
  }
  __device__ void load(const PixRowsPB& p, u32x4* r) const {
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const int q = k0 + krow0 + i * KSTEP;
      bool ok = colok & (q < kend);
      int b = 0;
      int src = q;
      if constexpr (SHIFT || PRO) {
        const int t = (int)fdiv((uint32_t)q, p.fdW);
        const int xx = q - t * p.W;
        b = (int)fdiv((uint32_t)t, p.fdH);
        const int yy = t - b * p.H;
        if constexpr (SHIFT) {
          ok = ok & ((unsigned)(yy + dy) < (unsigned)p.H) & ((unsigned)(xx + dx) < (unsigned)p.W);
          src = q + dy * p.W + dx;
        }
        if constexpr (PRO) b = ok ? b : 0;
      }
      uint32_t off = ((uint32_t)((src - base_pix) * p.ld + col) * 2u) | (ok ? 0u : OOB);
      u32x4 v = bload16(rsrc, off);
      if constexpr (PRO) {
        u32x4 a = prologue8(v, p.scale, p.shift, p.mask + (size_t)b * p.mask_ld,
                            colok ? col : 0, p.slope, p.mask_on);
        v = ok ? a : u32x4{0u, 0u, 0u, 0u};
      }
      r[i] = v;
    }
  }
  __device__ void advance(const PixRowsPB&) { k0 += BKB; }
  __device__ void store(bf16_t* S, const u32x4* r) const {
#pragma unroll
    for (int i = 0; i < NPT; ++i) *(u32x4*)&S[(krow0 + i * KSTEP) * KMS + c8o] = r[i];
  }
};


__device__ __forceinline__ F8 shfl_xor8(F8 v, int o) {
  F8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r.a[i] = __shfl_xor(v.a[i], o, 64);
    r.b[i] = __shfl_xor(v.b[i], o, 64);
  }
  return r;
}
__device__ __forceinline__ F8 unpack8(u32x4 w) {
  return F8{f32x4{bf_lo(w.x), bf_hi(w.x), bf_lo(w.y), bf_hi(w.y)},
            f32x4{bf_lo(w.z), bf_hi(w.z), bf_lo(w.w), bf_hi(w.w)}};
}
__device__ __forceinline__ F8 lrelu_grad8(F8 z, float slope) {
  F8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r.a[i] = lrelu_grad(z.a[i], slope);
    r.b[i] = lrelu_grad(z.b[i], slope);
  }
  return r;
}

// bf16 store epilogue: y = bf16(acc + bias); optional BN partials of the
// ROUNDED values (the tensor BatchNorm reads, as under autocast).
struct EpiStoreBP {
  bf16_t* y;
  int ldy;
  const float* bias;
  float* stats;
  int vec = 1;  // 16-B stores staged through LDS (NSM_BF16_EPI_VEC=0: 2-byte stores)
  // optional eval-mode BN + LeakyReLU (+ skip) of the bf16-rounded conv output:
  // y = bf16(lrelu(bf16(acc + bias) * act_scale + act_shift, slope) (+ res))
  const float* act_scale = nullptr;
  const float* act_shift = nullptr;
  float slope = 0.f;
  const bf16_t* res = nullptr;
  int ldres = 0;
};
struct EpiStoreB {
  using P = EpiStoreBP;
  template <int TM, int TN, int WM, int WN>
  __device__ static void apply(const P& e, f32x16 (&acc)[TM][TN], const EpiCtx& cx, int M, int N,
                               int) {
    const int col = cx.lane & 31, h = cx.lane >> 5;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      int n = cx.nb + tn * 32 + col;
      float bv = (e.bias && n < N) ? e.bias[n] : 0.f;
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[tm][tn][i] = round_bf(acc[tm][tn][i] + bv);
    }
    // 16-B row stores through LDS: each wave stages its (TM*32) x (TN*32)
    // tile as bf16 rows in its own LDS region and writes whole 16-B chunks
    // (16 vector stores per lane at 256x256 instead of 128 2-byte stores,
    // which bound the store tail of the short-K launches). The regions fit:
    // every bf16 kernel's LDS holds >= 2 x 64 K-columns of (BM + BN) rows.
    constexpr int BMT = WM * TM * 32, BNT = WN * TN * 32, WR = TM * 32, WC = TN * 32;
    static_assert(BMT * BNT <= 128 * (BMT + BNT), "LDS staging region");
    if (e.vec && (N & 7) == 0 && (e.ldy & 7) == 0 && (((uintptr_t)e.y) & 15) == 0) {
      bf16_t* reg = (bf16_t*)cx.lds + (cx.wm * WN + cx.wn) * (WR * WC);
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int r = tm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            reg[r * WC + tn * 32 + col] = s16_bits(acc[tm][tn][i]);
          }
      // the wave reads back what its own lanes wrote (one wave's LDS ops
      // complete in order); the fences keep the reads below the writes
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      constexpr int CPR = WC / 8;  // 16-B chunks per region row
#pragma unroll
      for (int it = 0; it < WR * CPR / 64; ++it) {
        const int q = it * 64 + cx.lane, r = q / CPR, cc = q - r * CPR;
        const int m = cx.mb + r, n = cx.nb + cc * 8;
        u32x4 v = *(const u32x4*)&reg[r * WC + cc * 8];
        if (m < M && n < N) {
          if (e.act_scale) {
            F8 f = unpack8(v) * ld8(e.act_scale + n) + ld8(e.act_shift + n);
            f = F8{f32x4{lrelu(f.a.x, e.slope), lrelu(f.a.y, e.slope), lrelu(f.a.z, e.slope),
                         lrelu(f.a.w, e.slope)},
                   f32x4{lrelu(f.b.x, e.slope), lrelu(f.b.y, e.slope), lrelu(f.b.z, e.slope),
                         lrelu(f.b.w, e.slope)}};
            if (e.res) f += ld8(e.res + (size_t)m * e.ldres + n);
            v = u32x4{pack_bf2(f.a.x, f.a.y), pack_bf2(f.a.z, f.a.w), pack_bf2(f.b.x, f.b.y),
                      pack_bf2(f.b.z, f.b.w)};
          }
          *(u32x4*)&e.y[(size_t)m * e.ldy + n] = v;
        }
      }
      if (e.stats) __syncthreads();  // stats_only reuses the LDS
    } else {
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        int n = cx.nb + tn * 32 + col;
        if (n >= N) continue;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            int m = cx.mb + tm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (m >= M) continue;
            float v = acc[tm][tn][i];
            if (e.act_scale) {
              v = lrelu(v * e.act_scale[n] + e.act_shift[n], e.slope);
              if (e.res) v += ld1(e.res + (size_t)m * e.ldres + n);
              v = round_bf(v);
            }
            e.y[(size_t)m * e.ldy + n] = s16_bits(v);
          }
        }
      }
    }
    if (!e.stats) return;
    EpiStoreP ef{nullptr, 0, nullptr, e.stats, 0};
    // BN partials stay per 256 rows (nsm_conv_stat_rows_bf16) for 512-row tiles
    EpiStore::stats_only<TM, TN, WM, WN, (WM * TM * 32 > 256 ? 256 : WM * TM * 32)>(ef, acc, cx,
                                                                                    M, N);
  }
};

// epilogues that prefetch operands of their own before the K loop (EP::PreT,
// gemm_bf16_dma_kernel; the h2 GEMMs' has_pre / pre_of in nsm_conv_h2.inc)
template <class E, class = void>
struct s16_has_pre : std::false_type {};
template <class E>
struct s16_has_pre<E, std::void_t<typename E::template PreT<1, 1>>> : std::true_type {};
template <class E, int TM, int TN, bool = s16_has_pre<E>::value>
struct s16_pre_of {
  struct type {};
};
template <class E, int TM, int TN>
struct s16_pre_of<E, TM, TN, true> {
  using type = typename E::template PreT<TM, TN>;
};

// bf16 form of EpiBnBwd (nsm_conv.hip): g = bf16(acc), the dA1 tensor the
// unfused path stores, is staged as bf16 rows in LDS (as EpiStoreB); each
// lane then takes 16-B chunks of ONE 8-column group, loads the matching 16 B
// of Y1 and applies the BN backward there. Partials per 256-row chunk
// (nsm_conv_stat_rows_bf16), waves of one chunk combined in LDS, fixed order.
struct EpiBnBwdB {
  using P = BnBwdEpiP;
  // Y1 rows of the wave tile, loaded before the K loop (gemm_bf16_dma_kernel):
  // with the short K of the 1x1 input gradients the epilogue's Y1 read is the
  // kernel's main traffic; issued first it overlaps the operand DMA. Lane
  // layout of apply's loop: one 8-column group (lane % CPR), rows
  // (it * 64 + lane) / CPR. Only where the registers allow (wave tiles of
  // <= 64 x 64: 32 VGPRs; the 128 x 64 ones of 256 x 256 blocks load in the
  // epilogue)
  // (the prefetching form is EpiBnBwdBP below: PreT switches it on)
  template <int TM, int TN>
  struct PreTile {
    static constexpr int NIT = TM * 32 * (TN * 32 / 8) / 64;
    u32x4 yv[NIT];
  };
  template <int TM, int TN, int WM, int WN>
  __device__ static void prefetch(const P& e, PreTile<TM, TN>& pre, int mb, int nb, int lane, int M,
                                  int N) {
    constexpr int CPR = TN * 32 / 8;
    const int n = nb + (lane % CPR) * 8, nc = n < N ? n : 0;
    const bf16_t* __restrict__ Y = (const bf16_t*)e.y;
#pragma unroll
    for (int it = 0; it < PreTile<TM, TN>::NIT; ++it) {
      const int m = min(mb + (it * 64 + lane) / CPR, M - 1);
      pre.yv[it] = *(const u32x4*)(Y + (size_t)m * e.ldy + nc);
    }
  }
  template <int TM, int TN, int WM, int WN>
  __device__ static void apply(const P& e, f32x16 (&acc)[TM][TN], const EpiCtx& cx, int M, int N,
                               int) {
    apply_impl<TM, TN, WM, WN>(e, acc, cx, M, N, nullptr);
  }
  template <int TM, int TN, int WM, int WN>
  __device__ static void apply_pre(const P& e, f32x16 (&acc)[TM][TN], const EpiCtx& cx, int M,
                                   int N, const PreTile<TM, TN>& pre) {
    apply_impl<TM, TN, WM, WN>(e, acc, cx, M, N, &pre);
  }
  template <int TM, int TN, int WM, int WN>
  __device__ static void apply_impl(const P& e, f32x16 (&acc)[TM][TN], const EpiCtx& cx, int M,
                                    int N, const PreTile<TM, TN>* pre) {
    const int col = cx.lane & 31, h = cx.lane >> 5;
    constexpr int BMT = WM * TM * 32, BNT = WN * TN * 32, WR = TM * 32, WC = TN * 32;
    constexpr int CPR = WC / 8;  // 16-B chunks per region row
    static_assert(64 % CPR == 0, "a lane keeps one column group");
    static_assert(BMT * BNT <= 128 * (BMT + BNT), "LDS staging region");
    static_assert(WM * 2 * BNT * 4 <= 2 * BMT * BNT, "LDS reduction region");
    bf16_t* reg = (bf16_t*)cx.lds + (cx.wm * WN + cx.wn) * (WR * WC);
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int r = tm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
          reg[r * WC + tn * 32 + col] = (bf16_t)(pack_bf2(acc[tm][tn][i], 0.f) & 0xFFFFu);
        }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int cc = cx.lane % CPR, n = cx.nb + cc * 8;
    const bool nok = n < N, red = e.mode != 2;
    const int nc = nok ? n : 0;
    const F8 sc = ld8(e.scale + nc), sh = ld8(e.shift + nc), mu = ld8(e.mean + nc);
    const F8 is = red ? ld8(e.invstd + nc) : f8zero();
    const F8 k1 = red ? f8zero() : ld8(e.coef + nc), k2 = red ? f8zero() : ld8(e.coef + N + nc),
             k3 = red ? f8zero() : ld8(e.coef + 2 * N + nc);
    const bf16_t* __restrict__ Y = (const bf16_t*)e.y;
    bf16_t* __restrict__ O = (bf16_t*)e.out;
    const float* __restrict__ mk = e.mask;
    // all Y1 chunks of this lane first (clamped rows: unconditional, so they
    // issue back to back), then the arithmetic and stores
    constexpr int NIT = WR * CPR / 64;
    u32x4 yr[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if (pre) {
        yr[it] = pre->yv[it];
      } else {
        const int m = min(cx.mb + (it * 64 + cx.lane) / CPR, M - 1);
        yr[it] = *(const u32x4*)(Y + (size_t)m * e.ldy + nc);
      }
    }
    F8 s1 = f8zero(), s2 = f8zero();
    uint32_t am = 0;  // max|scale * dz| (e.k1dz: the k1 term of the dY1 bound)
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int r = (it * 64 + cx.lane) / CPR, m = cx.mb + r;
      const bool ok = m < M && nok;
      const u32x4 raw = *(const u32x4*)&reg[r * WC + cc * 8];
      const F8 g = unpack8(raw), v = unpack8(yr[it]);
      F8 dz = g * lrelu_grad8(v * sc + sh, e.slope);
      if (mk) dz = dz * ld8(mk + (size_t)fdiv((uint32_t)min(m, M - 1), e.fdHW) * N + nc);
      if (!red) {
        if (ok) st8s(O + (size_t)m * e.ldo + n, k1 * dz + k2 * (v - mu) + k3);
      } else if (ok) {
        s1 += dz;
        s2 += dz * ((v - mu) * is);
        if (e.mode == 1) *(u32x4*)(O + (size_t)m * e.ldo + n) = raw;
        if (e.k1dz) {
          amax_fold(am, sc.a * dz.a);
          amax_fold(am, sc.b * dz.b);
        }
      }
    }
    if (!red) return;
    if (e.k1dz) amax_flush(am, e.k1dz);  // uniform: every lane of the wave
#pragma unroll
    for (int o = CPR; o < 64; o <<= 1) {
      s1 += shfl_xor8(s1, o);
      s2 += shfl_xor8(s2, o);
    }
    __syncthreads();  // every wave is done with its staging region
    float* lds = cx.lds;  // [WM][2][BNT]
    if (cx.lane < CPR) {
      st8(lds + (cx.wm * 2) * BNT + cx.wn * WC + cc * 8, s1);
      st8(lds + (cx.wm * 2 + 1) * BNT + cx.wn * WC + cc * 8, s2);
    }
    __syncthreads();
    constexpr int RPP = BMT > 256 ? 256 : BMT;
    constexpr int G = BMT / RPP, WG = WM / G;
    static_assert(G * RPP == BMT && WG * G == WM, "partial groups");
    const int g = cx.wm / WG;
    if (cx.wm == g * WG && cx.m0 + g * RPP < M) {
      float* pr = e.partial + ((size_t)cx.mblk * G + g) * 2 * N;
      for (int j = cx.lane; j < 2 * WC; j += 64) {
        const int k = j / WC, c = j - k * WC, nn = cx.nb + c;
        if (nn >= N) continue;
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < WG; ++w) t += lds[((cx.wm + w) * 2 + k) * BNT + cx.wn * WC + c];
        pr[k * N + nn] = t;
      }
    }
  }
};

// EpiBnBwdB with its Y1 rows prefetched before the K loop (wave tiles of 64 x
// 64: 256 x 128 / 128 x 128 blocks)
struct EpiBnBwdBP : EpiBnBwdB {
  template <int TM, int TN>
  using PreT = PreTile<TM, TN>;
};

// NST = 1: single-K-slab launches (K <= BKB, e.g. the 1x1 convs of the 32-
// and 64-channel layers): one LDS stage, no next-slab loads, so two to three
// blocks share a CU and overlap each other's load and store phases.
template <int BM, int BN, int WM, int WN, class AL, class BL, class EP, class AP, class BP,
          int NST = 2>
__global__ void __launch_bounds__(WM * WN * 64) __attribute__((amdgpu_waves_per_eu(1, 2)))
    gemm_bf16_kernel(AP ap, BP bp, typename EP::P ep, int M, int N, int K, int kchunk, int zsplit) {
  constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);
  constexpr int A_SZ = AL::LDS_ELEMS, B_SZ = BL::LDS_ELEMS, STAGE = A_SZ + B_SZ;
  __shared__ __attribute__((aligned(16))) bf16_t lds[NST * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  // N-blocks vary fastest (grid.x): the column blocks of one row block are
  // dispatched together, one per XCD when N/BN = 8, so each XCD's L2 keeps
  // its weight slice and the activation rows are fetched once into the MALL
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int split = blockIdx.z % zsplit, batch = blockIdx.z / zsplit;
  const int kbeg = split * kchunk;
  const int kend = min(K, kbeg + kchunk);
  const int nk = (kend - kbeg + BKB - 1) / BKB;

  AL a;
  BL b;
  if constexpr (AL::KM) a.init(ap, m0, kbeg, kend, tid, batch);
  else a.init(ap, m0, kbeg, tid, batch);
  if constexpr (BL::KM) b.init(bp, n0, kbeg, kend, tid, batch);
  else b.init(bp, n0, kbeg, tid, batch);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  u32x4 ar[AL::NPT], br[BL::NPT];
  if (nk > 0) {
    a.load(ap, ar);
    b.load(bp, br);
    a.store(lds, ar);
    b.store(lds + A_SZ, br);
  }
  __syncthreads();

  const int arb = wm * TM * 32, brb = wn * TN * 32;
  for (int it = 0; it < nk; ++it) {
    const bf16_t* As = lds + (it & 1) * STAGE;
    const bf16_t* Bs = As + A_SZ;
    a.advance(ap);
    b.advance(bp);
    bf16x8 fa[2][TM], fb[2][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) fa[0][tm] = read_frag_b<AL::KM, BM>(As, arb + tm * 32, lane, 0);
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) fb[0][tn] = read_frag_b<BL::KM, BN>(Bs, brb + tn * 32, lane, 0);
    if constexpr (NST == 2) {
      a.load(ap, ar);
      b.load(bp, br);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int cur = s & 1;
      if (s < 3) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
          fa[cur ^ 1][tm] = read_frag_b<AL::KM, BM>(As, arb + tm * 32, lane, s + 1);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          fb[cur ^ 1][tn] = read_frag_b<BL::KM, BN>(Bs, brb + tn * 32, lane, s + 1);
      }
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          acc[tm][tn] = mfma_s16_32(fa[cur][tm], fb[cur][tn],
                                                                acc[tm][tn], 0, 0, 0);
    }
    if constexpr (NST == 2) {
      bf16_t* An = lds + ((it + 1) & 1) * STAGE;
      a.store(An, ar);
      b.store(An + A_SZ, br);
    }
    __syncthreads();
  }
  EpiCtx cx{m0, n0, m0 + arb, n0 + brb, wm, wn, lane, (float*)lds, (int)blockIdx.y,
            (int)blockIdx.z};
  EP::template apply<TM, TN, WM, WN>(ep, acc, cx, M, N, split);
}

#include "nsm_conv_s16_dma.inc"

// ---- host side ----------------------------------------------------------------
// 2-stage rings for the narrow DMA tiles (256x64 fwd, 128x128 / 64x64 wgrad):
// two or more blocks share a CU and hide each other's pipeline fill and
// epilogue (short K for the 64-channel layers); +0.6 % end to end.
// NSM_BF16_SMALL_STAGES=0 restores the 3/4-stage rings.
static bool small_stages() {
  static const bool v = env_flag("NSM_BF16_SMALL_STAGES", true);
  return v;
}

// NSM_BF16_DMA32=0: the 32-channel 3x3 convs on the register path
static bool bf16_dma32() { static const bool v = env_flag("NSM_BF16_DMA32", true); return v; }

// NSM_BF16_ONE_STAGE=0: single-K-slab register-path launches keep the 2-stage LDS
static bool bf16_one_stage() {
  static const bool v = env_flag("NSM_BF16_ONE_STAGE", true);
  return v;
}

template <int BM, int BN, int WM, int WN, bool PRO, class EP = EpiStoreB>
static int launch_conv_fwd_b(const ConvActPB& ap, const RowsKPB& bp, const typename EP::P& ep,
                             int M, int N, int K, hipStream_t s) {
  constexpr int NT = WM * WN * 64;
  using AL = ConvActLoaderB<BM, NT, PRO>;
  using BL = RowsKLoaderB<BN, NT>;
  dim3 grid(ceil_div(N, BN), ceil_div(M, BM), 1);
  // the store epilogue stages the BM x BN tile in the kernel's LDS: one stage
  // holds it only while BM * BN <= (BM + BN) * BKB
  constexpr bool ONE_FITS = BM * BN <= (BM + BN) * BKB;
  if (ONE_FITS && K <= BKB && bf16_one_stage())
    hipLaunchKernelGGL((gemm_bf16_kernel<BM, BN, WM, WN, AL, BL, EP, ConvActPB, RowsKPB,
                                         ONE_FITS ? 1 : 2>),
                       grid, dim3(NT), 0, s, ap, bp, ep, M, N, K, K, 1);
  else
    hipLaunchKernelGGL((gemm_bf16_kernel<BM, BN, WM, WN, AL, BL, EP, ConvActPB, RowsKPB>), grid,
                       dim3(NT), 0, s, ap, bp, ep, M, N, K, K, 1);
  NSM_LAUNCH_CHECK("conv_fwd_bf16");
  return 0;
}

// NSM_BF16_EPI_VEC=0: the store epilogue writes 2-byte elements directly
static int bf16_epi_vec() { static const int v = env_flag("NSM_BF16_EPI_VEC", true); return v; }
// NSM_BF16_WIDE128=0: the N = 128 DMA convolutions on 256x128 blocks
static bool bf16_wide128() { static const bool v = env_flag("NSM_BF16_WIDE128", true); return v; }

// NSM_BF16_DMA_MIN: grid size (in 256x128 blocks) from which the forward
// takes the 256-row LDS-DMA tiles
static long long bf16_dma_min_blocks() {
  static const long long v = env_int("NSM_BF16_DMA_MIN", 480);
  return v;
}
// rows per BN-partial row of the bf16 forward tile policy (256-row M-blocks,
// or 512-row blocks writing two partials)
static int conv_fwd_bm_b(long long M, int N) {
  // >= ~2 blocks of 256x128 per CU (1080p inference: conv6 at 135x240 gives
  // 127 x 8 = 1016 and runs the 256x256 LDS-DMA tiles: 720 -> ~420 us)
  if (N >= 128 && ceil_div(M, 256) * ceil_div(N, 128) >= bf16_dma_min_blocks()) return 256;
  if (N == 64 && ceil_div(M, 256) >= 1024) return 256;
  return conv_fwd_bm(M, N);
}

// NSM_BF16_BNB_TILE: block tile of the 16-bit 1x1 input gradient with the BN
// backward in its epilogue: 0 = the forward's policy (EpiBnBwdB; 256x256 /
// 512x128 LDS-DMA tiles, whose 128 x 64 wave tiles load Y1 in the epilogue),
// 1 = 128x128 and 2 = 256x128 DMA tiles with Y1 prefetched before the K loop
// (EpiBnBwdBP)
static int bf16_bnb_tile() { static const int v = (int)env_int("NSM_BF16_BNB_TILE", 0); return v; }
// the 1x1 shapes the tile knob takes (64-channel K-tiles of the LDS-DMA loader)
static bool bnb_tiled(int N, int cop) {
  return bf16_bnb_tile() && N % 128 == 0 && cop % DBK == 0 && bf16_dma_mode();
}

// rows per BN-partial row of the 16-bit EpiBnBwdB GEMM (its M tile, <= 256)
static int bnbwd_rows_b(long long M, int N, int cop) {
  if (bnb_tiled(N, cop)) return bf16_bnb_tile() == 1 ? 128 : 256;
  return conv_fwd_bm_b(M, N);
}

template <bool PRO, class EP = EpiStoreB>
static int dispatch_conv_fwd_b(const ConvActPB& ap, const RowsKPB& bp, const typename EP::P& ep,
                               int M, int N, int K, hipStream_t s) {
  constexpr bool STD = std::is_same<EP, EpiStoreB>::value;  // the A/B knobs: store epilogue only
  if constexpr (std::is_same<EP, EpiBnBwdB>::value) {
    // (the BN-partial rows follow the tile: bnbwd_rows_b, nsm_conv1x1_bnbwd_chunks)
    if (!PRO && bnb_tiled(N, ap.cin)) {
      if (bf16_bnb_tile() == 1)
        return launch_conv_fwd_dma<128, 128, 2, 2, 2, EpiBnBwdBP>(ap, bp, ep, M, N, K, s);
      return launch_conv_fwd_dma<256, 128, 4, 2, 2, EpiBnBwdBP>(ap, bp, ep, M, N, K, s);
    }
  }
  // the narrow 3x3 layers: halo-tiled direct convolution (its 512-row tiles
  // write two 256-row BN partials, as the 256-row policy counts them)
  if constexpr (STD)
    if (!PRO && conv_fwd_bm_b(M, N) == 256 && halo_fits(ap, bp, M, N))
      return dispatch_conv3x3_halo<EP>(ap, bp, ep, M, N, s);
  // the 32-channel 3x3 convs (conv2.0 fwd / dgrad): LDS-DMA with 32-deep
  // K-tiles (one tap each), 128x32 blocks of 2 waves, a 4-stage ring (40 KB:
  // four blocks per CU) instead of the latency-bound register path
  if (!PRO && N == 32 && ap.ksize == 3 && ap.cin == 32 && conv_fwd_bm_b(M, N) == 128 &&
      bf16_dma_mode() && bf16_dma32())
    return launch_conv_fwd_dma_v<128, 32, 2, 1, 4, 32, 0, EP>(ap, bp, ep, M, N, K, s);
  // 256x128 blocks of 8 waves (64x64 each) where the grid stays >= 4 blocks
  // per CU: half the operand bytes per FLOP of 128x128 (global-load bound in
  // bf16); otherwise the f32 path's policy
  if (conv_fwd_bm_b(M, N) == 256 && N == 64) {
    // the 64-channel layers (conv3, conv9, 1x1 into 64): 256x64 blocks of 8
    // waves (64x32 each), LDS-DMA with 3 stages when prologue-free
    if (!PRO && bf16_dma_mode() && ap.cin % DBK == 0)
      return small_stages() ? launch_conv_fwd_dma<256, 64, 4, 2, 2, EP>(ap, bp, ep, M, N, K, s)
                            : launch_conv_fwd_dma<256, 64, 4, 2, 3, EP>(ap, bp, ep, M, N, K, s);
    return launch_conv_fwd_b<256, 64, 4, 2, PRO, EP>(ap, bp, ep, M, N, K, s);
  }
  if (conv_fwd_bm_b(M, N) == 256) {
    // prologue-free, whole 64-channel K-tiles: the LDS-DMA pipeline (same
    // BM = 256, so the BN-partial row chunks are unchanged)
    const int mode = bf16_dma_mode();
    if (!PRO && mode && ap.cin % DBK == 0 && N % 128 == 0) {
      if (mode == 2 && N % 256 == 0) {
        if constexpr (STD) {
          switch (bf16_dma_pipe()) {
            case 1: return launch_conv_fwd_dma_v<256, 256, 2, 4, 5, 32, 0>(ap, bp, ep, M, N, K, s);
            case 2: return launch_conv_fwd_dma_v<256, 256, 2, 4, 4, 32, 0>(ap, bp, ep, M, N, K, s);
            case 3: return launch_conv_fwd_dma_v<256, 256, 2, 4, 2, 64, 1>(ap, bp, ep, M, N, K, s);
            default: break;
          }
        }
        return launch_conv_fwd_dma<256, 256, 2, 4, 2, EP>(ap, bp, ep, M, N, K, s);
      }
      // N = 128: 512x128 blocks (8 waves of 128x64, the 256x256 wave tile)
      // in a 2-stage ring of all 160 KiB: 80 KB of operands per 8.4 MFLOP
      // K-tile instead of 48 KB per 4.2 MFLOP at 256x128
      if (N == 128 && bf16_wide128())
        return launch_conv_fwd_dma<512, 128, 4, 2, 2, EP>(ap, bp, ep, M, N, K, s);
      return launch_conv_fwd_dma<256, 128, 4, 2, 3, EP>(ap, bp, ep, M, N, K, s);
    }
    return launch_conv_fwd_b<256, 128, 4, 2, PRO, EP>(ap, bp, ep, M, N, K, s);
  }
  long long mb128 = ceil_div(M, 128);
  if (N >= 128) {
    if (mb128 * ceil_div(N, 128) >= 512)
      return launch_conv_fwd_b<128, 128, 2, 2, PRO, EP>(ap, bp, ep, M, N, K, s);
    return launch_conv_fwd_b<64, 128, 2, 2, PRO, EP>(ap, bp, ep, M, N, K, s);
  }
  if (N >= 64) {
    if (mb128 * ceil_div(N, 64) >= 512)
      return launch_conv_fwd_b<128, 64, 2, 2, PRO, EP>(ap, bp, ep, M, N, K, s);
    return launch_conv_fwd_b<64, 64, 2, 2, PRO, EP>(ap, bp, ep, M, N, K, s);
  }
  if (mb128 >= 512) return launch_conv_fwd_b<128, 32, 4, 1, PRO, EP>(ap, bp, ep, M, N, K, s);
  return launch_conv_fwd_b<64, 32, 2, 1, PRO, EP>(ap, bp, ep, M, N, K, s);
}

template <int BM, int BN, int WM, int WN, bool SHIFT, bool PRO>
static int launch_wgrad_b(const PixRowsPB& ap, const PixRowsPB& bp, const EpiSlabP& ep, int M,
                          int N, int K, int kchunk, int splits, hipStream_t s) {
  constexpr int NT = WM * WN * 64;
  using AL = PixRowsLoaderB<BM, NT, false, false>;
  using BL = PixRowsLoaderB<BN, NT, SHIFT, PRO>;
  dim3 grid(ceil_div(N, BN), ceil_div(M, BM), splits);
  hipLaunchKernelGGL((gemm_bf16_kernel<BM, BN, WM, WN, AL, BL, EpiSlab, PixRowsPB, PixRowsPB>),
                     grid, dim3(NT), 0, s, ap, bp, ep, M, N, K, kchunk, splits);
  NSM_LAUNCH_CHECK("conv_wgrad_bf16");
  return 0;
}

template <bool SHIFT, bool PRO>
static int dispatch_wgrad_b(int BM, int BN, const PixRowsPB& ap, const PixRowsPB& bp,
                            const EpiSlabP& ep, int M, int N, int K, int kchunk, int splits,
                            hipStream_t s) {
#define NSM_WGB(bm, bn, wm, wn) \
  if (BM == bm && BN == bn)     \
    return launch_wgrad_b<bm, bn, wm, wn, SHIFT, PRO>(ap, bp, ep, M, N, K, kchunk, splits, s);
  NSM_WGB(128, 128, 2, 2)
  NSM_WGB(128, 64, 2, 2)
  NSM_WGB(128, 32, 4, 1)
  NSM_WGB(64, 128, 2, 2)
  NSM_WGB(64, 64, 2, 2)
  NSM_WGB(64, 32, 2, 1)
  NSM_WGB(32, 128, 1, 4)
  NSM_WGB(32, 64, 1, 2)
  NSM_WGB(32, 32, 1, 1)
#undef NSM_WGB
  return fail(NSM_E_ARG, "wgrad_bf16: no tile %dx%d", BM, BN);
}

// NSM_BF16_WGRAD_MULTITAP=0: one tap per weight-gradient N tile everywhere
static bool wgrad_multitap() {
  static const bool v = env_flag("NSM_BF16_WGRAD_MULTITAP", true);
  return v;
}

// NSM_BF16_WGRAD_WIDE=0 keeps 256x128 weight-gradient tiles where 256x256 fit
static bool wgrad_wide() { static const bool v = env_flag("NSM_BF16_WGRAD_WIDE", true); return v; }

// Prologue-free weight gradients (every 3x3, and the 1x1 whose activated
// operand is materialised) run on the LDS-DMA kernel: tile per channel counts
static bool wgrad_dma_tile(int cin_p, int cout_p, int ksize, bool pro, int& BM, int& BN) {
  if (!bf16_dma_mode() || pro || (ksize != 3 && ksize != 1)) return false;
  if (ksize == 3 && cin_p == 32 && cout_p == 32 && wgrad_multitap() && bf16_dma32()) {
    BM = 32;   // conv2.0: one N tile = 4 taps of 32 channels (the 3rd: 1 tap + zero fill)
    BN = 128;
    return true;
  }
  if (cin_p % 64 || cout_p % 64) return false;
  if (cout_p % 256 == 0 && cin_p % 256 == 0 && wgrad_wide()) {
    BM = 256;  // the forward's 256x256 geometry: 2 stages, 1.5 tr-reads per MFMA
    BN = 256;
  } else if (cout_p % 256 == 0 && cin_p % 128 == 0) {
    BM = 256;
    BN = 128;
  } else if (ksize == 3 && cin_p == 128 && cout_p == 128 && wgrad_multitap()) {
    BM = 128;  // one N tile = 3 whole taps: 5 fragments per 6 MFMAs (vs 3 per 2)
    BN = 384;
  } else if (ksize == 3 && cin_p == 64 && cout_p == 64 && wgrad_multitap()) {
    BM = 64;   // one N tile = 4 taps (the 3rd tile is 1 tap + zero fill)
    BN = 256;
  } else if (cout_p % 128 == 0 && cin_p % 128 == 0) {
    BM = 128;
    BN = 128;
  } else {
    BM = 64;
    BN = 64;
  }
  return true;
}

// NSM_BF16_WAVEQ=0: split count of the DMA weight gradients without the
// dispatch-round fit below
static bool wgrad_waveq() { static const bool v = env_flag("NSM_BF16_WAVEQ", true); return v; }
// resident blocks per CU of the DMA weight-gradient tiles (wgrad_dma_tile):
// LDS ring = STAGES x (BM + BN) x 64 bf16 out of 160 KiB; the 8-wave blocks
// (~100 VGPRs: 4 waves per SIMD) at most 2, the 4-wave ones at most 8
static int wgrad_blocks_per_cu(int bm, int bn) {
  int stages = 2, waves = 8;
  if (bm == 256 && bn == 128) stages = 3;
  if ((bm == 128 && bn == 128) || (bm == 64 && bn == 64)) stages = small_stages() ? 2 : 4;
  if ((bm == 64 && bn == 256) || (bm == 64 && bn == 64) || bm == 32) waves = 4;
  const int lds = stages * (bm + bn) * DBK * 2;
  return std::max(1, std::min(163840 / lds, waves == 8 ? 2 : 8));
}

static WgradPlan plan_wgrad_b(int B, int H, int W, int cin_p, int cout_p, int ksize, bool pro) {
  int dbm, dbn;
  if (wgrad_dma_tile(cin_p, cout_p, ksize, pro, dbm, dbn)) {
    // ~1024 blocks (4 per CU), >= 16 K-tiles per split, slabs <= 512 MB
    WgradPlan pl;
    pl.BM = dbm;
    pl.BN = dbn;
    const long long M = cout_p, N = (long long)ksize * ksize * cin_p, K = (long long)B * H * W;
    const long long tiles = ((M + dbm - 1) / dbm) * ((N + dbn - 1) / dbn);
    long long sp = (1024 + tiles - 1) / tiles;
    const long long cap = std::max(1ll, std::min({(K + 1023) / 1024,
                                                  std::max(1ll, (128ll << 20) / (M * N)), 512ll}));
    sp = std::max(1ll, std::min(sp, cap));
    auto fit = [&](long long s_, long long& kc_) {  // split count after K-chunk rounding
      kc_ = (K + s_ - 1) / s_;
      kc_ = (kc_ + DBK - 1) / DBK * DBK;
      return (K + kc_ - 1) / kc_;
    };
    long long kc;
    sp = fit(sp, kc);
    if (wgrad_waveq()) {
      // whole dispatch rounds: every block does the same work, so the time goes
      // as ceil(blocks / slots) rounds of one K-chunk each; among split counts
      // within 25 % of the default, take the fewest rounds x chunk length
      // (ties: fewer splits, i.e. less slab traffic). E.g. conv7's 3x3 weight
      // gradient: 36 tiles x 29 splits = 1044 blocks = 5 rounds of 256 CUs,
      // 28 splits = 1008 blocks = 4 rounds of a 3.5 % longer chunk.
      const long long slots = (long long)cu_count() * wgrad_blocks_per_cu(dbm, dbn);
      double best = 1e30;
      long long bsp = sp, bkc = kc;
      for (long long t = std::max(1ll, sp * 3 / 4); t <= std::min(cap, sp + sp / 4 + 1); ++t) {
        long long kt;
        const long long st = fit(t, kt);
        const double cost = (double)((tiles * st + slots - 1) / slots) * (double)kt;
        if (cost < best * (1 - 1e-9) || (cost <= best * (1 + 1e-9) && st < bsp)) {
          best = cost;
          bsp = st;
          bkc = kt;
        }
      }
      sp = bsp;
      kc = bkc;
    }
    pl.splits = (int)sp;
    pl.kchunk = (int)kc;
    pl.ws_floats = (size_t)sp * M * N;
    if (sp > 16) pl.ws_floats += (size_t)((sp + 15) / 16) * M * N;
    return pl;
  }
  WgradPlan pl = plan_wgrad(B, H, W, cin_p, cout_p, ksize);
  // an N tile covers whole taps or divides one (s16_conv_wgrad checks it): the
  // channel counts that fit the planned tile neither way (96: 128 columns of a
  // 3x3, 64 of a 1x1) take 32-column tiles
  if (cin_p % pl.BN != 0 && pl.BN % cin_p != 0 && cin_p % 32 == 0) pl.BN = 32;
  const long long K = (long long)B * H * W;
  long long kc = (pl.kchunk + BKB - 1) / BKB * BKB;
  long long sp = (K + kc - 1) / kc;
  pl.kchunk = (int)kc;
  pl.splits = (int)sp;
  const long long MN = (long long)cout_p * ksize * ksize * cin_p;
  pl.ws_floats = (size_t)sp * MN;
  if (sp > 16) pl.ws_floats += (size_t)((sp + 15) / 16) * MN;
  return pl;
}

__global__ void pack_weight_bf16_kernel(const float* __restrict__ w, int cout, int cin, int taps,
                                        int cout_p, int cin_p, int mode, bf16_t* __restrict__ out) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  int total = cout_p * cin_p * taps;
  if (idx >= total) return;
  float v;
  if (mode == NSM_PACK_FWD) {
    int ci = idx % cin_p;
    int t = idx / cin_p;
    int tap = t % taps;
    int co = t / taps;
    v = (co < cout && ci < cin) ? w[((size_t)co * cin + ci) * taps + tap] : 0.f;
  } else {
    int co = idx % cout_p;
    int t = idx / cout_p;
    int tap = t % taps;
    int ci = t / taps;
    v = (co < cout && ci < cin) ? w[((size_t)co * cin + ci) * taps + (taps - 1 - tap)] : 0.f;
  }
  out[idx] = (bf16_t)(pack_bf2(v, 0.f) & 0xFFFFu);
}

// ---- the 16-bit entry bodies (C entries: after the inclusion) -------------------
static int s16_pack_conv_weight(const float* w, int cout, int cin, int ksize, int cout_p, int cin_p,
                                int mode, void* out, void* stream) {
  NSM_CHECK_ARG(w && out && cout > 0 && cin > 0 && cout_p >= cout && cin_p >= cin,
                "pack_conv_weight_s16: bad args");
  NSM_CHECK_ARG(mode == NSM_PACK_FWD || mode == NSM_PACK_DGRAD, "pack_conv_weight_s16: mode");
  int taps = ksize * ksize;
  int total = cout_p * cin_p * taps;
  hipLaunchKernelGGL(pack_weight_bf16_kernel, dim3(ceil_div(total, 256)), dim3(256), 0,
                     as_stream(stream), w, cout, cin, taps, cout_p, cin_p, mode, (bf16_t*)out);
  NSM_LAUNCH_CHECK("pack_conv_weight_s16");
  return 0;
}

static int s16_conv_fwd(const void* x, int ldx, int B, int H, int W, int cin_p, const void* wpk,
                        const float* bias, int cout_p, int ksize, void* y, int ldy,
                        const float* pro_scale, const float* pro_shift, const float* pro_mask,
                        float slope, float* stats, void* stream) {
  NSM_CHECK_ARG(x && wpk && y, "conv_fwd_s16: null pointer");
  NSM_CHECK_ARG(B > 0 && H > 0 && W > 0, "conv_fwd_s16: bad shape");
  NSM_CHECK_ARG(cin_p % 32 == 0 && cout_p % 32 == 0, "conv_fwd_s16: channels must be x32");
  NSM_CHECK_ARG(ldx >= cin_p && ldx % 8 == 0 && ldy >= cout_p, "conv_fwd_s16: bad leading dims");
  NSM_CHECK_ARG(ksize == 1 || ksize == 3, "conv_fwd_s16: ksize %d", ksize);
  NSM_CHECK_ARG(!pro_scale || pro_shift, "conv_fwd_s16: prologue needs scale and shift");
  NSM_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)wpk % 16) == 0, "conv_fwd_s16: alignment");
  long long Ml = (long long)B * H * W;
  NSM_CHECK_ARG(Ml < (1ll << 30), "conv_fwd_s16: too many pixels");
  ConvActPB ap;
  ap.x = (const bf16_t*)x;
  ap.ld = ldx;
  ap.cin = cin_p;
  ap.H = H;
  ap.W = W;
  ap.M = (int)Ml;
  ap.ksize = ksize;
  ap.K = ksize * ksize * cin_p;
  ap.fdW = make_fastdiv(W);
  ap.fdH = make_fastdiv(H);
  ap.fdC = make_fastdiv(cin_p);
  ap.scale = pro_scale;
  ap.shift = pro_shift;
  ap.mask = pro_mask ? pro_mask : pro_scale;
  ap.mask_ld = pro_mask ? cin_p : 0;
  ap.mask_on = pro_mask != nullptr;
  ap.slope = slope;
  const int K = ap.K;
  // the LDS-DMA kernels walk a 3x3 conv's K channel-major: the 9 taps of one
  // 64-channel chunk are consecutive K-tiles, so a block re-reads the same
  // activation rows 9 times within ~50 KB (L2-resident) instead of once per
  // pass over all channels (measured 13x the algorithmic bytes tap-major)
  const int cm = ksize == 3 && bf16_korder() ? 1 : 0;
  ap.cm = cm;
  RowsKPB bp{(const bf16_t*)wpk, K, cout_p, K, cin_p, cm};
  EpiStoreBP ep{(bf16_t*)y, ldy, bias, stats, bf16_epi_vec()};
  hipStream_t s = as_stream(stream);
  if (pro_scale) return dispatch_conv_fwd_b<true>(ap, bp, ep, (int)Ml, cout_p, K, s);
  return dispatch_conv_fwd_b<false>(ap, bp, ep, (int)Ml, cout_p, K, s);
}

static int s16_conv_wgrad(const void* dy, int lddy, const void* x, int ldx, int B, int H, int W,
                          int cin_p, int cout_p, int ksize, const float* pro_scale,
                          const float* pro_shift, const float* pro_mask, float slope, float* ws,
                          size_t ws_floats, int cin, int cout, float* dw, void* stream) {
  NSM_CHECK_ARG(dy && x && ws && dw, "conv_wgrad_s16: null pointer");
  NSM_CHECK_ARG(cin_p % 32 == 0 && cout_p % 32 == 0, "conv_wgrad_s16: channels must be x32");
  NSM_CHECK_ARG(ksize == 1 || ksize == 3, "conv_wgrad_s16: ksize %d", ksize);
  NSM_CHECK_ARG(lddy >= cout_p && ldx >= cin_p && lddy % 8 == 0 && ldx % 8 == 0,
                "conv_wgrad_s16: bad leading dims");
  NSM_CHECK_ARG(!pro_scale || (pro_shift && ksize == 1), "conv_wgrad_s16: prologue needs 1x1");
  NSM_CHECK_ARG(cin <= cin_p && cout <= cout_p, "conv_wgrad_s16: real dims exceed padded");
  WgradPlan pl = plan_wgrad_b(B, H, W, cin_p, cout_p, ksize, pro_scale != nullptr);
  NSM_CHECK_ARG(cin_p % pl.BN == 0 || pl.BN % cin_p == 0, "conv_wgrad_s16: N tile straddles taps");
  if (ws_floats < pl.ws_floats)
    return fail(NSM_E_WS, "conv_wgrad_s16: workspace %zu < %zu floats", ws_floats, pl.ws_floats);
  const int M = cout_p, N = ksize * ksize * cin_p;
  const long long Kl = (long long)B * H * W;
  NSM_CHECK_ARG(Kl < (1ll << 30), "conv_wgrad_s16: too many pixels");
  PixRowsPB ap{};
  ap.x = (const bf16_t*)dy;
  ap.ld = lddy;
  ap.ncols = cout_p;
  ap.cin = 0;
  ap.H = H;
  ap.W = W;
  ap.M = (int)Kl;
  ap.ksize = 1;
  ap.fdW = make_fastdiv(W);
  ap.fdH = make_fastdiv(H);
  PixRowsPB bp = ap;
  bp.x = (const bf16_t*)x;
  bp.ld = ldx;
  bp.ncols = cin_p;
  bp.cin = cin_p;
  bp.ksize = ksize;
  bp.scale = pro_scale;
  bp.shift = pro_shift;
  bp.mask = pro_mask ? pro_mask : pro_scale;
  bp.mask_ld = pro_mask ? cin_p : 0;
  bp.mask_on = pro_mask != nullptr;
  bp.slope = slope;
  EpiSlabP ep{ws};
  hipStream_t s = as_stream(stream);
  int rc;
  int dbm, dbn;
  if (wgrad_dma_tile(cin_p, cout_p, ksize, pro_scale != nullptr, dbm, dbn)) {
    if (dbm == 128 && dbn == 384)
      rc = launch_wgrad_dma<128, 384, 2, 4, 2>(ap, bp, ep, M, N, (int)Kl, pl.kchunk, pl.splits, s);
    else if (dbm == 64 && dbn == 256)
      rc = launch_wgrad_dma<64, 256, 1, 4, 2>(ap, bp, ep, M, N, (int)Kl, pl.kchunk, pl.splits, s);
    else if (dbm == 32 && dbn == 128)
      rc = launch_wgrad_dma<32, 128, 1, 4, 2>(ap, bp, ep, M, N, (int)Kl, pl.kchunk, pl.splits, s);
    else if (dbm == 256 && dbn == 256)
      rc = launch_wgrad_dma<256, 256, 2, 4, 2>(ap, bp, ep, M, N, (int)Kl, pl.kchunk, pl.splits, s);
    else if (dbm == 256)
      rc = launch_wgrad_dma<256, 128, 4, 2, 3>(ap, bp, ep, M, N, (int)Kl, pl.kchunk, pl.splits, s);
    else if (dbm == 128)
      rc = small_stages()
               ? launch_wgrad_dma<128, 128, 2, 4, 2>(ap, bp, ep, M, N, (int)Kl, pl.kchunk, pl.splits, s)
               : launch_wgrad_dma<128, 128, 2, 4, 4>(ap, bp, ep, M, N, (int)Kl, pl.kchunk, pl.splits, s);
    else
      rc = small_stages()
               ? launch_wgrad_dma<64, 64, 2, 2, 2>(ap, bp, ep, M, N, (int)Kl, pl.kchunk, pl.splits, s)
               : launch_wgrad_dma<64, 64, 2, 2, 4>(ap, bp, ep, M, N, (int)Kl, pl.kchunk, pl.splits, s);
  } else if (ksize == 3)
    rc = dispatch_wgrad_b<true, false>(pl.BM, pl.BN, ap, bp, ep, M, N, (int)Kl, pl.kchunk,
                                       pl.splits, s);
  else if (pro_scale)
    rc = dispatch_wgrad_b<false, true>(pl.BM, pl.BN, ap, bp, ep, M, N, (int)Kl, pl.kchunk,
                                       pl.splits, s);
  else
    rc = dispatch_wgrad_b<false, false>(pl.BM, pl.BN, ap, bp, ep, M, N, (int)Kl, pl.kchunk,
                                        pl.splits, s);
  if (rc) return rc;
  return wgrad_finish(ws, pl, M, N, cin_p, ksize * ksize, cin, cout, dw, s);
}

// eval-mode conv + BN + LeakyReLU (+ skip) in one pass
static int s16_conv_fwd_act(const void* x, int ldx, int B, int H, int W, int cin_p, const void* wpk,
                            const float* bias, int cout_p, int ksize, void* y, int ldy,
                            const float* act_scale, const float* act_shift, float slope,
                            const void* res, int ldres, hipStream_t s) {
  NSM_CHECK_ARG(x && wpk && y && act_scale && act_shift, "conv_fwd_act_s16: null pointer");
  NSM_CHECK_ARG(B > 0 && H > 0 && W > 0 && cin_p % 32 == 0 && cout_p % 32 == 0,
                "conv_fwd_act_s16: bad shape");
  NSM_CHECK_ARG(ldx >= cin_p && ldx % 8 == 0 && ldy >= cout_p && ldy % 8 == 0 &&
                    (!res || (ldres >= cout_p && ldres % 8 == 0)),
                "conv_fwd_act_s16: bad leading dims");
  NSM_CHECK_ARG(ksize == 1 || ksize == 3, "conv_fwd_act_s16: ksize %d", ksize);
  NSM_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)wpk % 16) == 0 &&
                    ((uintptr_t)y % 16) == 0 && ((uintptr_t)res % 16) == 0,
                "conv_fwd_act_s16: alignment");
  const long long Ml = (long long)B * H * W;
  NSM_CHECK_ARG(Ml < (1ll << 30), "conv_fwd_act_s16: too many pixels");
  ConvActPB ap{};
  ap.x = (const bf16_t*)x;
  ap.ld = ldx;
  ap.cin = cin_p;
  ap.H = H;
  ap.W = W;
  ap.M = (int)Ml;
  ap.ksize = ksize;
  ap.K = ksize * ksize * cin_p;
  ap.fdW = make_fastdiv(W);
  ap.fdH = make_fastdiv(H);
  ap.fdC = make_fastdiv(cin_p);
  ap.cm = ksize == 3 && bf16_korder() ? 1 : 0;
  RowsKPB bp{(const bf16_t*)wpk, ap.K, cout_p, ap.K, cin_p, ap.cm};
  EpiStoreBP ep{(bf16_t*)y, ldy, bias, nullptr, 1, act_scale, act_shift, slope,
                (const bf16_t*)res, ldres};
  return dispatch_conv_fwd_b<false>(ap, bp, ep, (int)Ml, cout_p, ap.K, s);
}

// 1x1 input gradient with the BN backward in its epilogue (EpiBnBwdB)
static int s16_conv1x1_dgrad_bnbwd(const void* dy2, int lddy2, int B, int H, int W, int cop,
                                   const void* w2d, int cip, const BnBwdEpiP& ep, hipStream_t s) {
  const long long Ml = (long long)B * H * W;
  ConvActPB ap{};
  ap.x = (const bf16_t*)dy2;
  ap.ld = lddy2;
  ap.cin = cop;
  ap.H = H;
  ap.W = W;
  ap.M = (int)Ml;
  ap.ksize = 1;
  ap.K = cop;
  ap.fdW = make_fastdiv(W);
  ap.fdH = make_fastdiv(H);
  ap.fdC = make_fastdiv(cop);
  ap.cm = 0;
  RowsKPB bp{(const bf16_t*)w2d, cop, cip, cop, cop, 0};
  return dispatch_conv_fwd_b<false, EpiBnBwdB>(ap, bp, ep, (int)Ml, cip, cop, s);
}
