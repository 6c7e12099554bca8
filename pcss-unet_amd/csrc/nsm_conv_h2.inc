// fp32 Winograd GEMMs on PRE-SPLIT f16x2 operands ("h2" tensors), global ->
// LDS by LDS-DMA. Included at the top of nsm_conv_h2.hip only (uses the LDS-DMA
// helpers and the f16x2 split helpers of nsm_conv.h).
//
// The f16x2 split (nsm_conv_split16.inc) writes each fp32 operand x scaled by
// s = 2^e as h + l, two fp16 terms. gemm_f32h_kernel does that split in the
// GEMM, on the way from registers to LDS: 3 VALU and two 8-B LDS writes per 4
// elements for every block that loads the element, beside an MFMA pipe it
// then shares issue slots with. Here the PRODUCER of the operand (the
// Winograd input / dual transforms, the step's weight preparation) writes the
// two terms to HBM instead of the fp32 value — same bytes (2 x 2 B per
// element) — and the GEMM is a plain f16 GEMM fed by LDS-DMA: no VALU, no
// ds_write, no loader registers, so it can run the 256-row tiles of the bf16
// DMA kernels.
//
// h2 layout: a [rows][C] fp32 matrix becomes f16 [rows][2C]; the 8 channels
// of chunk j are h at 16j .. 16j+7 and l at 16j+8 .. 16j+15. A K-tile of 64
// f16 columns (32 channels, 2 k-steps of 16) is one 128-B LDS row per M/N row,
// the MK image of the bf16 DMA kernels (nsm_conv_s16_dma.inc: 16-B chunks
// XOR-swizzled by dswz); the plane-p fragment of k-step s is chunk 4s + 2h + p
// (h = lane >> 5). KM images (weight gradient: K = Winograd tiles): K-tile of
// 32 rows x 2R f16 columns, read with ds_read_b64_tr_b16 as the bf16 KM image
// with channel chunk c at h2 chunk 2c + p.
//
// The scale must be known when the producer writes, before the operand's
// maximum is: s = 2^(15 - ceil(log2(beta * max|source|))), with max|source|
// recorded by the producer of the TRANSFORM'S INPUT (bn_act, bn_bwd_apply,
// the weights) and beta the transform's bound (max_i sum_j |T_ij|)^2, so
// |x * s| <= 2^15 < 65504 always. A bound above the true maximum only moves
// the f16x2 absolute floor (2^-25 in scaled units) up by the bound's slack
// (<= 2^8 for these transforms): still 2^-32 of the tensor maximum, far below
// fp32 rounding of the sums. Producer and GEMM compute e from the same slot
// and beta (h2_exp).

// H2Scale, h2_exp, h2_store4: nsm_common.h; h2_pair_word, h2_pair_off: nsm_conv.h

// epilogues that prefetch operands of their own before the K loop (EP::PreT)
template <class E, class = void>
struct has_pre : std::false_type {};
template <class E>
struct has_pre<E, std::void_t<typename E::template PreT<1, 1>>> : std::true_type {};
template <class E, int TM, int TN, bool = has_pre<E>::value>
struct pre_of {
  struct type {};
};
template <class E, int TM, int TN>
struct pre_of<E, TM, TN, true> {
  using type = typename E::template PreT<TM, TN>;
};

// ---- operands ------------------------------------------------------------------
struct H2RowsP {  // MK / NK: f16 rows [batch][nrows][ld], ld = 2 * channels
  const bf16_t* x;
  int ld, nrows;
  long long bstride;  // f16 elements between batch entries
};
template <int R, int NW, int KT_ = 64>
struct H2RowsDma {
  static constexpr bool KM = false;
  static constexpr int KT = KT_;  // f16 columns per K-tile (64: 2 k-steps, 32: 1)
  static constexpr int CH = KT / 8, RPI = 64 / CH;
  static constexpr int NI = R / (RPI * NW);
  static_assert(NI >= 1 && NI * RPI * NW == R, "dma shape");
  using P = H2RowsP;
  __amdgpu_buffer_rsrc_t rsrc;
  uint32_t base[NI];
  uint32_t koff;
  __device__ void init(const P& p, int r0, int, int, int wid, int lane, int batch) {
    rsrc = make_rsrc_b(p.x + (size_t)batch * p.bstride + (size_t)r0 * p.ld,
                       (long long)(p.nrows - r0) * p.ld);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int row = (wid * NI + i) * RPI + lane / CH;
      base[i] = ((uint32_t)(row * p.ld + ((lane % CH) ^ dswz<KT>(row)) * 8) * 2u) |
                (r0 + row < p.nrows ? 0u : OOB);
    }
  }
  __device__ void prep(const P&, int k0) { koff = (uint32_t)k0 * 2u; }
  __device__ void one(const P&, const bf16_t* stage, int wid, int i) const {
    dma16(rsrc, stage + (wid * NI + i) * 512, base[i] + koff);
  }
  // persistent kernels: tile-independent row offsets once, then per tile only
  // the descriptor (rows past nrows fall outside its range)
  __device__ void rows(const P& p, int wid, int lane) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int row = (wid * NI + i) * RPI + lane / CH;
      base[i] = (uint32_t)(row * p.ld + ((lane % CH) ^ dswz<KT>(row)) * 8) * 2u;
    }
  }
  __device__ void aim(const P& p, int r0, int batch) {
    rsrc = make_rsrc_b(p.x + (size_t)batch * p.bstride + (size_t)r0 * p.ld,
                       (long long)(p.nrows - r0) * p.ld);
  }
};

// 16-B chunk XOR of pixel row k of the h2 / single-plane KM images
// (H2PixDma, F16PixDma). kmswz puts the 4 rows of a fragment read's 16-lane
// group in distinct 64-B bank quarters, but an h2 row uses only half of its
// quarter (the chunks of one plane) and the other 16-lane group of the 32-lane
// bank group lands on the same half: 2-way conflicts on every
// ds_read_b64_tr_b16. The low bits here send that group to the other half (h2:
// the plane bit, by k ^ k >> 3 for both the 32x32x16 and the 16x16x32 lane
// maps; single plane: the half-quarter bit, by k >> 3 for the 16x16x32 map).
#ifndef NSM_KMSWZ2
#define NSM_KMSWZ2 1  // 0: kmswz (A/B builds)
#endif
template <int R, bool SP>
__device__ __forceinline__ int kmswz2(int k) {
  if constexpr (!NSM_KMSWZ2) return kmswz<R>(k);
  const int x = SP ? 2 * ((k >> 3) & 1) : ((k ^ (k >> 3)) & 1);
  if constexpr (2 * R >= 256) return (4 * (k & 3)) ^ x;
  else if constexpr (2 * R == 128) return (4 * ((k >> 1) & 1)) ^ x;
  else return 0;
}
// loaders that lay their KM image out by kmswz2 (SW2)
template <class L, class = void>
struct sw2_of : std::false_type {};
template <class L>
struct sw2_of<L, std::void_t<decltype(L::SW2)>> : std::bool_constant<L::SW2> {};

struct H2PixP {  // KM: f16 rows [batch][nrows][ld] whose row index is the GEMM's K
  const bf16_t* x;
  int ld, ncols, nrows;  // ncols = ld = 2 * channels
  long long bstride;
};
template <int R, int NW>  // R: f16 columns of the tile (2 x its channels)
struct H2PixDma {
  static constexpr bool KM = true, SW2 = true;
  static constexpr int KT = 32;  // K rows per K-tile
  static constexpr int RB = 2 * R;
  static constexpr int NI = KT * RB / 1024 / NW;
  static_assert(R >= 64 && NI >= 1 && NI * NW * 1024 == KT * RB, "dma shape");
  using P = H2PixP;
  __amdgpu_buffer_rsrc_t rsrc;
  int row[NI];
  uint32_t cof[NI];
  int krel, klen;
  __device__ void init(const P& p, int c0, int kbeg, int kend, int wid, int lane, int batch) {
    rsrc = make_rsrc_b(p.x + (size_t)batch * p.bstride + (size_t)kbeg * p.ld,
                       (long long)(p.nrows - kbeg) * p.ld);
    klen = kend - kbeg;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int byte = (wid * NI + i) * 1024 + lane * 16;
      const int k = byte / RB, pc = (byte % RB) / 16;
      row[i] = k;
      const int col = 2 * c0 + ((pc ^ kmswz2<R, false>(k)) << 3);
      cof[i] = ((uint32_t)col * 2u) | (col < p.ncols ? 0u : OOB);
    }
  }
  __device__ void prep(const P&, int k0) { krel = k0; }  // relative to kbeg (set by the kernel)
  __device__ void one(const P& p, const bf16_t* stage, int wid, int i) const {
    const int q = krel + row[i];
    const uint32_t off = ((uint32_t)q * (uint32_t)p.ld * 2u + cof[i]) | (q < klen ? 0u : OOB);
    dma16(rsrc, stage + (wid * NI + i) * 512, off);
  }
};

// KM single-plane f16 rows [batch][nrows][ld] (ld = ncols = channels): the
// bf16 path's Winograd weight gradient (dM, V of nsm_wino_*_f16); R: the
// tile's channels = f16 columns
template <int R, int NW, int KT_ = 32>  // KT_ 64: 4 k-steps per K-tile (gemm_h2_kernel, SP)
struct F16PixDma {
  static constexpr bool KM = true, SW2 = true;
  static constexpr int KT = KT_;
  static constexpr int RB = 2 * R;
  static constexpr int NI = KT * RB / 1024 / NW;
  static_assert(R >= 64 && NI >= 1 && NI * NW * 1024 == KT * RB, "dma shape");
  using P = H2PixP;
  __amdgpu_buffer_rsrc_t rsrc;
  int row[NI];
  uint32_t cof[NI];
  int krel, klen;
  __device__ void init(const P& p, int c0, int kbeg, int kend, int wid, int lane, int batch) {
    rsrc = make_rsrc_b(p.x + (size_t)batch * p.bstride + (size_t)kbeg * p.ld,
                       (long long)(p.nrows - kbeg) * p.ld);
    klen = kend - kbeg;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int byte = (wid * NI + i) * 1024 + lane * 16;
      const int k = byte / RB, pc = (byte % RB) / 16;
      row[i] = k;
      const int col = c0 + ((pc ^ kmswz2<R, true>(k)) << 3);
      cof[i] = ((uint32_t)col * 2u) | (col < p.ncols ? 0u : OOB);
    }
  }
  __device__ void prep(const P&, int k0) { krel = k0; }
  __device__ void one(const P& p, const bf16_t* stage, int wid, int i) const {
    const int q = krel + row[i];
    const uint32_t off = ((uint32_t)q * (uint32_t)p.ld * 2u + cof[i]) | (q < klen ? 0u : OOB);
    dma16(rsrc, stage + (wid * NI + i) * 512, off);
  }
};

// plane-p fragment of k-step s for rows rb..rb+31; R = KM image row length
// in f16, MK: the K-tile width (64: s = 0, 1; 32: s = 0)
// SP (single-plane operands, KM): channel chunk c at chunk c (the bf16 KM
// image's mapping), p unused
// SW2: the image is laid out by kmswz2 (H2PixDma, F16PixDma), else kmswz
template <bool KM, int R, bool SP = false, bool SW2 = false>
struct FragH2 {
  __device__ static int swz(int k) {
    if constexpr (SW2) return kmswz2<R, SP>(k);
    else return kmswz<R>(k);
  }
  static constexpr int NR = KM ? 2 : 1;
  u32x4 v;
  s16x4 lo, hi;
  __device__ __forceinline__ void issue(const bf16_t* S, int rb, int lane, int s, int p) {
    if constexpr (!KM) {
      constexpr int KT = R;
      const int row = rb + (lane & 31), chunk = 4 * s + 2 * (lane >> 5) + p;
      v = *(const u32x4*)&S[row * KT + ((chunk ^ dswz<KT>(row)) << 3)];
    } else {
      const int h = lane >> 5, g16 = (lane >> 4) & 1, q = (lane >> 2) & 3, pp = lane & 3;
      const int k = 16 * s + 8 * h + q;
      const int lc = SP ? (rb >> 3) + 2 * g16 + (pp >> 1) : 2 * ((rb >> 3) + 2 * g16 + (pp >> 1)) + p;
      const int sub = (pp & 1) * 4;
      typedef __attribute__((address_space(3))) bf16_t lds_bf16;
      const uint32_t a0 = (uint32_t)(uintptr_t)(lds_bf16*)(S + k * R + ((lc ^ swz(k)) << 3) + sub);
      const uint32_t a1 =
          (uint32_t)(uintptr_t)(lds_bf16*)(S + (k + 4) * R + ((lc ^ swz(k + 4)) << 3) + sub);
      asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(a0));
      asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(hi) : "v"(a1));
    }
  }
  __device__ __forceinline__ void hold() {
    if constexpr (KM) asm volatile("" : "+v"(lo), "+v"(hi));
  }
  __device__ __forceinline__ f16x8 get() const {
    if constexpr (!KM) return __builtin_bit_cast(f16x8, v);
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 w = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return __builtin_bit_cast(f16x8, w);
  }
};

// fp32 store epilogue through LDS, one 32-row slab of the wave tile at a time
// (the staging region of a whole 128x64 wave tile would not fit beside the
// 256x256 stages): out[zslab * bstride + m * ld + n], 16-B stores
struct EpiH2P {
  float* out;
  int ld;
  long long bstride;
  // O16: one scale exponent per 64 x 64 tile of M (per batch entry
  // [ceil(M/64)][N/64], int32), chosen from the tile's own max|acc|
  int* m16e = nullptr;
  int m16e_rows = 0;  // ceil(M / 64)
};

// O16: the exponent of one 64 x 64 tile of M, from the wave's max|acc| over
// it (bits of a non-negative float): |acc 2^e| <= 2^15, so the f16 value is
// normal down to 2^-29 of the tile's maximum (a static tensor-wide bound left
// channels far below it subnormal). 0 for an all-zero or non-finite tile.
__device__ __forceinline__ int m16_tile_exp(uint32_t mbits) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mbits = max(mbits, (uint32_t)__shfl_xor((int)mbits, o));
  return pow2_scale_exp(mbits);
}
struct EpiH2 {
  using P = EpiH2P;
  template <int TM, int TN, int WM, int WN>
  static constexpr int lds_bytes() { return WM * WN * 32 * (TN * 32 + 4) * 4; }
  template <int TM, int TN, int WM, int WN>
  __device__ static void apply(const P& e, f32x16 (&acc)[TM][TN], const EpiCtx& cx, int M, int N,
                               int) {
    const int col = cx.lane & 31, h = cx.lane >> 5;
    constexpr int WC = TN * 32, WCP = WC + 4, CPR = WC / 4;
    float* reg = cx.lds + (cx.wm * WN + cx.wn) * (32 * WCP);
    float* ob = e.out + (size_t)cx.zslab * e.bstride;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          reg[((i & 3) + 8 * (i >> 2) + 4 * h) * WCP + tn * 32 + col] = acc[tm][tn][i];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int it = 0; it < 32 * CPR / 64; ++it) {
        const int q = it * 64 + cx.lane, r = q / CPR, cc = q - r * CPR;
        const int m = cx.mb + tm * 32 + r, n = cx.nb + cc * 4;
        if (m < M && n < N) *(f32x4*)(ob + (size_t)m * e.ld + n) = *(const f32x4*)&reg[r * WCP + cc * 4];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
};

template <int TM, int TN, class FA, class FB>
__device__ __forceinline__ void mfma_h2(f32x16 (&acc)[TM][TN], const FA (&fa)[2][TM],
                                        const FB (&fb)[2][TN], int tm, int tn) {
  f32x16 c = acc[tm][tn];
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[1][tm].get(), fb[0][tn].get(), c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][tm].get(), fb[1][tn].get(), c, 0, 0, 0);
  acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][tm].get(), fb[0][tn].get(), c, 0, 0, 0);
}

// The h2 GEMM: C[batch][m][n] = sum_k A[batch](m, k) B[batch](n, k) over K-tiles of
// AL::KT (MK: f16 columns, KM: rows); block tile BM x BN, WM x WN waves of
// (BM/WM) x (BN/WN); grid (ceil(M/BM), ceil(N/BN), batch * zsplit), split z
// of a batch entry covers K range [z*kchunk, min(K, (z+1)*kchunk)).
// The pipeline is the bf16 DMA kernel's cross-tile form (REFILL 3) with two
// k-steps per K-tile: 2 LDS stages; the K-tile barrier sits between the reads
// and the MFMAs of the last k-step, the next tile's first fragments load under
// them, and the refill of the stage just released goes out one piece per
// MFMA group.
// SP: single-plane KM operands (F16PixDma): one product per k-step
template <int BM, int BN, int WM, int WN, class AL, class BL, class EP, bool SP = false>
__global__ void __launch_bounds__(WM * WN * 64)
    gemm_h2_kernel(typename AL::P ap, typename BL::P bp, typename EP::P ep, int M, int N, int K,
                   int kchunk, int zsplit, int remap, H2Scale sca, H2Scale scb) {
  static_assert(!SP || (AL::KM && BL::KM), "single-plane: KM operands");
  constexpr int NPL = SP ? 1 : 2;  // planes read per k-step
  constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);
  constexpr int A_EL = BM * 64, STAGE = (BM + BN) * 64;  // f16 elements (MK and KM alike)
  constexpr int KT = AL::KT;
  static_assert(KT == BL::KT, "K-tile");
  constexpr int LPT = AL::NI + BL::NI;
  constexpr int EPI = EP::template lds_bytes<TM, TN, WM, WN>() / 2;
  constexpr int LDS_EL = 2 * STAGE > EPI ? 2 * STAGE : EPI;
  __shared__ __attribute__((aligned(1024))) bf16_t lds[LDS_EL];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (remap) xcd_block_order(bx, by, bz, remap);
  const int m0 = bx * BM, n0 = by * BN;
  const int split = bz % zsplit, batch = bz / zsplit;
  const int kbeg = split * kchunk;
  const int kend = min(K, kbeg + kchunk);
  const int nk = (kend - kbeg + KT - 1) / KT;
  const int ea = h2_exp(sca), eb = h2_exp(scb);
  // MK loaders address K absolutely, KM loaders relative to their kbeg
  const int kb0 = AL::KM ? 0 : kbeg;

  AL a;
  BL b;
  a.init(ap, m0, kbeg, kend, wid, lane, batch);
  b.init(bp, n0, kbeg, kend, wid, lane, batch);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // an epilogue with operands of its own (EpiBnBwd: Y1) loads them first: they
  // are older than every DMA below, so the counted vmcnt waits stay exact
  constexpr bool PRE = has_pre<EP>::value;
  typename pre_of<EP, TM, TN>::type pre;
  if constexpr (PRE)
    EP::template prefetch<TM, TN, WM, WN>(ep, pre, m0 + (wid / WN) * TM * 32,
                                          n0 + (wid % WN) * TN * 32, lane, M, N);

  if (nk > 0) {
    a.prep(ap, kb0);
    b.prep(bp, kb0);
#pragma unroll
    for (int j = 0; j < LPT; ++j) dma_one(a, b, ap, bp, lds, A_EL, wid, j);
  }
  if (nk > 1) {
    a.prep(ap, kb0 + KT);
    b.prep(bp, kb0 + KT);
#pragma unroll
    for (int j = 0; j < LPT; ++j) dma_one(a, b, ap, bp, lds + STAGE, A_EL, wid, j);
    vm_wait<LPT>();
  } else {
    vm_wait<0>();
  }
  dma_barrier();

  constexpr bool KMR = AL::KM || BL::KM;
  using FA = FragH2<AL::KM, AL::KM ? (SP ? BM : 2 * BM) : AL::KT, SP, sw2_of<AL>::value>;
  using FB = FragH2<BL::KM, BL::KM ? (SP ? BN : 2 * BN) : BL::KT, SP, sw2_of<BL>::value>;
  constexpr int NRT = NPL * (TM * FA::NR + TN * FB::NR);
  const int arb = wm * TM * 32, brb = wn * TN * 32;
  FA fa[2][2][TM];  // [k-step buffer][plane][tm]
  FB fb[2][2][TN];
#pragma unroll
  for (int p = 0; p < NPL; ++p) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) fa[0][p][tm].issue(lds, arb + tm * 32, lane, 0, p);
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) fb[0][p][tn].issue(lds + A_EL, brb + tn * 32, lane, 0, p);
  }
  // k-steps per K-tile: 2 (MK 64 columns, KM 32 rows), or 4 (single-plane KM
  // images of 64 rows: the K-tile barrier, refill and loader bookkeeping once
  // per 4 k-steps; the stage holds the bytes of the h2 32-row one)
  constexpr int NS = AL::KM ? KT / 16 : 2;
  static_assert(NS == 2 || (NS == 4 && SP && AL::KM && BL::KM), "64-row K-tiles: single-plane KM");
  if constexpr (NS == 4) {
    for (int t = 0; t < nk; ++t) {
      const bf16_t* As = lds + (t & 1) * STAGE;
      const bf16_t* Bs = As + A_EL;
      const bool more = t + 1 < nk, refill = t + 2 < nk;
#pragma unroll
      for (int ks = 0; ks < NS; ++ks) {
        const int cur = ks & 1, nxt = cur ^ 1;
        if (ks + 1 < NS) {
          // k-step ks+1's fragments go out, then k-step ks's MFMAs
#pragma unroll
          for (int tm = 0; tm < TM; ++tm) fa[nxt][0][tm].issue(As, arb + tm * 32, lane, ks + 1, 0);
#pragma unroll
          for (int tn = 0; tn < TN; ++tn) fb[nxt][0][tn].issue(Bs, brb + tn * 32, lane, ks + 1, 0);
          lgkm_fence_n<(NRT < 15 ? NRT : 15)>();
#pragma unroll
          for (int tm = 0; tm < TM; ++tm) fa[cur][0][tm].hold();
#pragma unroll
          for (int tn = 0; tn < TN; ++tn) fb[cur][0][tn].hold();
        } else {
          if (refill) {
            a.prep(ap, kb0 + (t + 2) * KT);
            b.prep(bp, kb0 + (t + 2) * KT);
          }
          __builtin_amdgcn_s_waitcnt(0xC07F);  // this wave's reads of stage t&1 retired
          lgkm_fence();
#pragma unroll
          for (int tm = 0; tm < TM; ++tm) fa[cur][0][tm].hold();
#pragma unroll
          for (int tn = 0; tn < TN; ++tn) fb[cur][0][tn].hold();
          if (more) {
            vm_wait<0>();                  // this wave's pieces of tile t+1
            __builtin_amdgcn_s_barrier();  // everyone's reads retired, pieces landed
            const bf16_t* Ns = lds + ((t + 1) & 1) * STAGE;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) fa[nxt][0][tm].issue(Ns, arb + tm * 32, lane, 0, 0);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) fb[nxt][0][tn].issue(Ns + A_EL, brb + tn * 32, lane, 0, 0);
          }
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn) {
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[cur][0][tm].get(), fb[cur][0][tn].get(),
                                                                 acc[tm][tn], 0, 0, 0);
            if (ks + 1 == NS && refill) {
              const int q = tm * TN + tn;
#pragma unroll
              for (int i = 0; i < LPT; ++i)
                if (i * (TM * TN) / LPT == q) dma_one(a, b, ap, bp, As, A_EL, wid, i);
            }
          }
        __builtin_amdgcn_s_setprio(0);
      }
    }
  } else
  for (int t = 0; t < nk; ++t) {
    const bf16_t* As = lds + (t & 1) * STAGE;
    const bf16_t* Bs = As + A_EL;
    // k-step 0: k-step 1's fragments go out, then k-step 0's MFMAs
#pragma unroll
    for (int p = 0; p < NPL; ++p) {
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) fa[1][p][tm].issue(As, arb + tm * 32, lane, 1, p);
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) fb[1][p][tn].issue(Bs, brb + tn * 32, lane, 1, p);
    }
    if constexpr (KMR) {
      lgkm_fence_n<(NRT < 15 ? NRT : 15)>();  // (lgkmcnt counts to 15: stricter is still safe)
#pragma unroll
      for (int p = 0; p < NPL; ++p) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) fa[0][p][tm].hold();
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) fb[0][p][tn].hold();
      }
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        if constexpr (SP)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][0][tm].get(), fb[0][0][tn].get(),
                                                               acc[tm][tn], 0, 0, 0);
        else
          mfma_h2<TM, TN>(acc, fa[0], fb[0], tm, tn);
      }
    __builtin_amdgcn_s_setprio(0);
    const bool more = t + 1 < nk, refill = t + 2 < nk;
    if (refill) {
      a.prep(ap, kb0 + (t + 2) * KT);
      b.prep(bp, kb0 + (t + 2) * KT);
    }
    // this wave's reads of stage t&1 retired (compiler-visible, see REFILL 3)
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if constexpr (KMR) {
      lgkm_fence();
#pragma unroll
      for (int p = 0; p < NPL; ++p) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) fa[1][p][tm].hold();
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) fb[1][p][tn].hold();
      }
    }
    if (more) {
      vm_wait<0>();                  // this wave's pieces of tile t+1
      __builtin_amdgcn_s_barrier();  // everyone's reads retired, pieces landed
      const bf16_t* Ns = lds + ((t + 1) & 1) * STAGE;
#pragma unroll
      for (int p = 0; p < NPL; ++p) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) fa[0][p][tm].issue(Ns, arb + tm * 32, lane, 0, p);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) fb[0][p][tn].issue(Ns + A_EL, brb + tn * 32, lane, 0, p);
      }
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        if constexpr (SP)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[1][0][tm].get(), fb[1][0][tn].get(),
                                                               acc[tm][tn], 0, 0, 0);
        else
          mfma_h2<TM, TN>(acc, fa[1], fb[1], tm, tn);
        if (refill) {
          const int q = tm * TN + tn;
#pragma unroll
          for (int i = 0; i < LPT; ++i)
            if (i * (TM * TN) / LPT == q) dma_one(a, b, ap, bp, As, A_EL, wid, i);
        }
      }
    __builtin_amdgcn_s_setprio(0);
  }
  dma_barrier();  // the epilogue reuses the LDS
  const float ia = exp2i(-ea), ib = exp2i(-eb);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (acc[i][j] * ia) * ib;
  EpiCtx cx{m0, n0, m0 + arb, n0 + brb, wm, wn, lane, (float*)lds, bx, bz};
  if constexpr (PRE) EP::template apply_pre<TM, TN, WM, WN>(ep, acc, cx, M, N, pre);
  else EP::template apply<TM, TN, WM, WN>(ep, acc, cx, M, N, split);
}

// ---- the MK h2 GEMM on v_mfma_f32_16x16x32_f16 -----------------------------------
// MI355X_MICROARCH.md, DVFS (7): with LDS-fed operands the 16x16x32 shape holds
// a higher clock than 32x32x16 at equal cycles per FLOP (1.12-1.14x FLOP/s).
// A K-tile of 64 f16 columns (32 channels x 2 planes) is ONE 32-deep k-step:
// lane l supplies row (l & 15) and channels 8 (l >> 4) .. +7 of one plane, a
// 16-B chunk (h2 chunk 2 (l >> 4) + p). Wave tile TM2 x TN2 quadrants of 16x16
// (acc4, f32x4 each); per tile and wave: TN2 x 2 B fragments, then per
// row-group TM2 x 2 A fragments streamed one row-group ahead of its 3 x TN2
// MFMAs. The K-tile barrier sits before the last row-group's MFMAs (its
// fragments are in by then), the next tile's B fragments and first A
// row-group load under them, and the refill of the stage just released goes
// out between them.
// SP (single plane): A and B are plain scaled-f16 tensors [rows][C] (no l
// terms, the bf16 path's Winograd operands): a K-tile of 64 f16 columns is 64
// channels, its "plane" p = 0, 1 chunks two halves of them, and the k-step is
// the two same-plane products h_p(A) h_p(B) instead of the three f16x2 ones.
// O16 (the bf16 path's Winograd M, nsm_wino_gemm_f16m): the GEMM writes
// f16 M = acc 2^e in the operands' scaled units, e chosen per 64 x 64 tile of
// M from that tile's own max|acc| (m16_tile_exp: the tile maximum maps to
// <= 2^15, so no maximum pass over M is needed) and recorded in ep.m16e
// [batch][ceil(M/64)][N/64]; the output transform undoes 2^-(e + e_v + e_u)
// tile by tile. (pack_f16x4: nsm_common.h)

// KM (weight gradient: both operands KM images of 32-row K-tiles, H2PixDma /
// F16PixDma): the 32-deep k-step is the whole K-tile; lane l's 8 k values of
// row (l & 15) come from two ds_read_b64_tr_b16 (rows 8 (l >> 4) + q and +4 of
// the 16-lane group's 4 x 16 block, delivered transposed), the h2 plane p of
// channel chunk c at image chunk 2c + p (SP: chunk c, one product per K-tile)
template <bool KM, int R, bool SP>
__device__ __forceinline__ f16x8 rd_h2q(const bf16_t* S, int rb, int p, int lane) {
  if constexpr (!KM) {
    const int row = rb + (lane & 15), chunk = 2 * (lane >> 4) + p;
    return __builtin_bit_cast(f16x8, *(const u32x4*)&S[row * R + ((chunk ^ dswz<R>(row)) << 3)]);
  } else {
    // the XOR swizzle makes every fragment's address lane-dependent: kept
    // opaque so the compiler recomputes it (3 VALU) instead of holding one
    // register per fragment live across the K loop
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int q = (ln >> 2) & 3, pp = ln & 3, k = 8 * (ln >> 4) + q;
    const int c8 = (rb >> 3) + (pp >> 1), lc = SP ? c8 : 2 * c8 + p, sub = (pp & 1) * 4;
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (lds_s16x4*)(S + k * R + ((lc ^ kmswz2<R, SP>(k)) << 3) + sub));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (lds_s16x4*)(S + (k + 4) * R + ((lc ^ kmswz2<R, SP>(k + 4)) << 3) + sub));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return __builtin_bit_cast(f16x8, v);
  }
}

template <int BM, int BN, int WM, int WN, class AL, class BL, bool SP = false, bool O16 = false>
__global__ void __launch_bounds__(WM * WN * 64)
    gemm_h2q_kernel(typename AL::P ap, typename BL::P bp, EpiH2P ep, int M, int N, int K,
                    int kchunk, int zsplit, int remap, H2Scale sca, H2Scale scb) {
  constexpr int TM2 = BM / (WM * 16), TN2 = BN / (WN * 16);
  constexpr bool KM = AL::KM;
  static_assert(KM == BL::KM, "MK x NK or KM x KM");
  static_assert(!KM || (sw2_of<AL>::value && sw2_of<BL>::value), "KM images laid out by kmswz2");
  static_assert(KM ? (AL::KT == 32 && BL::KT == 32) : (AL::KT == 64 && BL::KT == 64),
                "MK 64-column / KM 32-row K-tiles");
  static_assert(TM2 % 2 == 0 && TN2 % 2 == 0, "whole 32x32 slabs for the epilogue");
  constexpr int KT = AL::KT;
  constexpr bool ONE = KM && SP;  // single-plane KM: one product per K-tile
  static_assert(!O16 || (SP && !KM), "f16 M: the bf16 path's single-plane MK GEMM");
  // LDS row length of a stage image (MK: the K-tile; KM: the tile's f16 columns)
  constexpr int RA = KM ? (SP ? BM : 2 * BM) : KT, RB = KM ? (SP ? BN : 2 * BN) : KT;
  constexpr int A_EL = BM * 64, STAGE = (BM + BN) * 64;  // f16 elements (MK and KM alike)
  constexpr int LPT = AL::NI + BL::NI;
  constexpr int WC = TN2 * 16, WCP = WC + 4;
  constexpr int EPI = WM * WN * 32 * WCP * 2;  // f16 elements of the epilogue's fp32 staging
  constexpr int LDS_EL = 2 * STAGE > EPI ? 2 * STAGE : EPI;
  __shared__ __attribute__((aligned(1024))) bf16_t lds[LDS_EL];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (remap) xcd_block_order(bx, by, bz, remap);
  const int m0 = bx * BM, n0 = by * BN;
  const int split = bz % zsplit, batch = bz / zsplit;
  const int kbeg = split * kchunk;
  const int kend = min(K, kbeg + kchunk);
  const int nk = (kend - kbeg + KT - 1) / KT;
  const int ea = h2_exp(sca), eb = h2_exp(scb);
  const int kb0 = KM ? 0 : kbeg;  // KM loaders address K relative to their kbeg

  AL a;
  BL b;
  a.init(ap, m0, kbeg, kend, wid, lane, batch);
  b.init(bp, n0, kbeg, kend, wid, lane, batch);

  f32x4 acc[TM2][TN2];
#pragma unroll
  for (int i = 0; i < TM2; ++i)
#pragma unroll
    for (int j = 0; j < TN2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (nk > 0) {
    a.prep(ap, kb0);
    b.prep(bp, kb0);
#pragma unroll
    for (int j = 0; j < LPT; ++j) dma_one(a, b, ap, bp, lds, A_EL, wid, j);
  }
  if (nk > 1) {
    a.prep(ap, kb0 + KT);
    b.prep(bp, kb0 + KT);
#pragma unroll
    for (int j = 0; j < LPT; ++j) dma_one(a, b, ap, bp, lds + STAGE, A_EL, wid, j);
    vm_wait<LPT>();
  } else {
    vm_wait<0>();
  }
  dma_barrier();

  const int arb = wm * TM2 * 16, brb = wn * TN2 * 16;
  // fragment of plane p for rows rb..rb+15 (lane & 15) of a stage image
  auto rda = [&](const bf16_t* S, int rb, int p) { return rd_h2q<KM, RA, SP>(S, rb, p, lane); };
  auto rdb = [&](const bf16_t* S, int rb, int p) { return rd_h2q<KM, RB, SP>(S, rb, p, lane); };
  f16x8 fb[2][2][TN2];  // [tile parity][plane][col group]
  f16x8 fa[2][2];       // [row-group parity][plane]
#pragma unroll
  for (int j = 0; j < TN2; ++j) {
    fb[0][0][j] = rdb(lds + A_EL, brb + 16 * j, 0);
    if constexpr (!ONE) fb[0][1][j] = rdb(lds + A_EL, brb + 16 * j, 1);
  }
  fa[0][0] = rda(lds, arb, 0);
  if constexpr (!ONE) fa[0][1] = rda(lds, arb, 1);
  for (int t = 0; t < nk; t += 2) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {  // two tiles per trip: B fragment buffers by parity
      const int tt = t + u;
      if (tt >= nk) break;
      const bf16_t* As = lds + u * STAGE;  // tt & 1 == u (t even)
      const bool more = tt + 1 < nk, refill = tt + 2 < nk;
      if (refill) {
        a.prep(ap, kb0 + (tt + 2) * KT);
        b.prep(bp, kb0 + (tt + 2) * KT);
      }
#pragma unroll
      for (int i = 0; i < TM2; ++i) {
        constexpr int dummy = 0;
        (void)dummy;
        const int cb = i & 1;
        if (i + 1 < TM2) {
          fa[cb ^ 1][0] = rda(As, arb + 16 * (i + 1), 0);
          if constexpr (!ONE) fa[cb ^ 1][1] = rda(As, arb + 16 * (i + 1), 1);
        } else {
          // this wave's reads of stage tt&1 retired (compiler-visible)
          __builtin_amdgcn_s_waitcnt(0xC07F);
          if (more) {
            vm_wait<0>();                  // this wave's pieces of tile tt+1
            __builtin_amdgcn_s_barrier();  // everyone's reads retired, pieces landed
            const bf16_t* Ns = lds + (u ^ 1) * STAGE;
#pragma unroll
            for (int j = 0; j < TN2; ++j) {
              fb[u ^ 1][0][j] = rdb(Ns + A_EL, brb + 16 * j, 0);
              if constexpr (!ONE) fb[u ^ 1][1][j] = rdb(Ns + A_EL, brb + 16 * j, 1);
            }
            fa[cb ^ 1][0] = rda(Ns, arb, 0);
            if constexpr (!ONE) fa[cb ^ 1][1] = rda(Ns, arb, 1);
          }
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < TN2; ++j) {
          f32x4 c = acc[i][j];
          if constexpr (ONE) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[cb][0], fb[u][0][j], c, 0, 0, 0);
          } else if constexpr (SP) {
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[cb][0], fb[u][0][j], c, 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[cb][1], fb[u][1][j], c, 0, 0, 0);
          } else {
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[cb][1], fb[u][0][j], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[cb][0], fb[u][1][j], c, 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[cb][0], fb[u][0][j], c, 0, 0, 0);
          }
          if (i + 1 == TM2 && refill) {
#pragma unroll
            for (int q = 0; q < LPT; ++q)
              if (q * TN2 / LPT == j) dma_one(a, b, ap, bp, As, A_EL, wid, q);
          }
        }
        __builtin_amdgcn_s_setprio(0);
      }
    }
  }
  dma_barrier();  // the epilogue reuses the LDS
  const float ia = exp2i(-ea), ib = exp2i(-eb);
  // O16: a scale per 64-row group of the wave tile (64 columns wide), from its
  // own maximum (m16_tile_exp), recorded in ep.m16e for the output transform
  constexpr int NG = TM2 >= 4 ? TM2 / 4 : 1;
  float osc[NG];
  if constexpr (O16) {
    static_assert(TN2 * 16 == 64 && TM2 % 4 == 0, "O16: 64 x 64 exponent tiles");
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      uint32_t mb = 0;
#pragma unroll
      for (int i = 4 * g; i < 4 * g + 4; ++i)
#pragma unroll
        for (int j = 0; j < TN2; ++j) amax_fold(mb, acc[i][j]);
      const int e = m16_tile_exp(mb);
      osc[g] = exp2i(e);
      const int r64 = (m0 + arb) / 64 + g, c64 = (n0 + brb) / 64;
      if (lane == 0 && r64 < ep.m16e_rows)
        ep.m16e[((size_t)bz * ep.m16e_rows + r64) * (N / 64) + c64] = e;
    }
  }
  // epilogue: 32-row slabs (two 16-row groups) staged in LDS, 16-B stores
  float* reg = (float*)lds + (wm * WN + wn) * (32 * WCP);
  float* ob = ep.out + (size_t)bz * ep.bstride;
  bf16_t* ob16 = (bf16_t*)ep.out + (size_t)bz * ep.bstride;
  constexpr int CPR = WC / 4;
#pragma unroll
  for (int s2 = 0; s2 < TM2 / 2; ++s2) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < TN2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          reg[(16 * h + 4 * (lane >> 4) + e) * WCP + 16 * j + (lane & 15)] =
              O16 ? acc[2 * s2 + h][j][e] * osc[(2 * s2 + h) / 4 < NG ? (2 * s2 + h) / 4 : 0]
                  : (acc[2 * s2 + h][j][e] * ia) * ib;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int it = 0; it < 32 * CPR / 64; ++it) {
      const int q = it * 64 + lane, r = q / CPR, cc = q - r * CPR;
      const int m = m0 + arb + 32 * s2 + r, n = n0 + brb + cc * 4;
      if (m < M && n < N) {
        const f32x4 v = *(const f32x4*)&reg[r * WCP + cc * 4];
        if constexpr (O16) *(u32x2*)(ob16 + (size_t)m * ep.ld + n) = pack_f16x4(v);
        else *(f32x4*)(ob + (size_t)m * ep.ld + n) = v;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// ---- persistent form: the epilogue under the next tile's loads ----------------------
// gemm_h2q_kernel runs one output tile per block at one block per CU; its
// epilogue (256 KB of fp32 per 256x256 tile) and the next block's prologue
// (descriptor setup, the first two K-tiles' DMA latency, a barrier) stall the
// matrix cores once per tile, in step on every CU, while all of them store at
// once. Here a grid of one block per CU walks the tiles L = blockIdx.x + r *
// gridDim.x (XCD-contiguous order as xcd_block_order), and the K-tile stream
// runs on ACROSS tiles: the last two K-tiles of a tile refill their stages
// with the next tile's first two (the loaders re-aimed at the next tile), the
// next tile's first fragments load under the last MFMAs, and the epilogue
// stages its fp32 rows through an LDS region of its own (16 rows x 64 columns
// per wave, 16-float blocks XOR-swizzled by row quad) and stores with buffer
// stores (rows past M fall outside the descriptor: a constant store count per
// lane, which the next counted vmcnt wait skips over). zsplit 1, K % 128 == 0
// (an even number of K-tiles keeps the stage parity), 64-column wave tiles.
template <int BM, int BN, int WM, int WN, class AL, class BL, bool SP = false, bool O16 = false>
__global__ void __launch_bounds__(WM * WN * 64)
    gemm_h2p_kernel(typename AL::P ap, typename BL::P bp, EpiH2P ep, int M, int N, int K, int gx,
                    int gy, int total, H2Scale sca, H2Scale scb, int nfast) {
  constexpr int TM2 = BM / (WM * 16), TN2 = BN / (WN * 16);
  static_assert(!AL::KM && !BL::KM && AL::KT == 64 && BL::KT == 64, "MK 64-column K-tiles");
  static_assert(TN2 == 4, "64-column wave tiles: one 256-B staging row");
  constexpr int KT = 64;
  constexpr int A_EL = BM * KT, STAGE = (BM + BN) * KT;
  constexpr int LPT = AL::NI + BL::NI;
  constexpr int SPL = TM2 * 4;  // epilogue stores per lane and tile
  static_assert(SPL <= 63 && LPT <= 63, "vmcnt range");
  constexpr int STG = WM * WN * 16 * 64;  // fp32 staging
  __shared__ __attribute__((aligned(1024))) bf16_t lds[2 * STAGE + 2 * STG];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int nk = K / KT;
  static_assert(!O16 || SP, "f16 M: single-plane operands");
  static_assert(!O16 || TM2 % 4 == 0, "O16: 64 x 64 exponent tiles");
  const float ia = exp2i(-h2_exp(sca)), ib = exp2i(-h2_exp(scb));
  const bool remap = (total & 7) == 0;
  auto decode = [&](int L, int& m0, int& n0, int& bz) {
    const int lg = remap ? (L & 7) * (total >> 3) + (L >> 3) : L;
    // nfast: the N tiles of one M block consecutive (they share its A rows:
    // with many M blocks, M-fastest runs them far apart and re-fetches A)
    m0 = (nfast ? (lg / gy) % gx : lg % gx) * BM;
    n0 = (nfast ? lg % gy : (lg / gx) % gy) * BN;
    bz = lg / (gx * gy);
  };
  int L = blockIdx.x;
  int m0, n0, bz;
  decode(L, m0, n0, bz);

  AL a;
  BL b;
  a.rows(ap, wid, lane);
  b.rows(bp, wid, lane);
  a.aim(ap, m0, bz);
  b.aim(bp, n0, bz);
  a.prep(ap, 0);
  b.prep(bp, 0);
#pragma unroll
  for (int j = 0; j < LPT; ++j) dma_one(a, b, ap, bp, lds, A_EL, wid, j);
  a.prep(ap, KT);
  b.prep(bp, KT);
#pragma unroll
  for (int j = 0; j < LPT; ++j) dma_one(a, b, ap, bp, lds + STAGE, A_EL, wid, j);
  vm_wait<0>();  // both K-tiles: the first tile's K-tile-1 wait then counts like every other tile's
  dma_barrier();

  const int arb = wm * TM2 * 16, brb = wn * TN2 * 16;
  auto rd = [&](const bf16_t* S, int rb, int p) {
    const int row = rb + (lane & 15), chunk = 2 * (lane >> 4) + p;
    return __builtin_bit_cast(f16x8, *(const u32x4*)&S[row * KT + ((chunk ^ dswz<KT>(row)) << 3)]);
  };
  f16x8 fb[2][2][TN2];
  f16x8 fa[2][2];
#pragma unroll
  for (int j = 0; j < TN2; ++j) {
    fb[0][0][j] = rd(lds + A_EL, brb + 16 * j, 0);
    fb[0][1][j] = rd(lds + A_EL, brb + 16 * j, 1);
  }
  fa[0][0] = rd(lds, arb, 0);
  fa[0][1] = rd(lds, arb, 1);
  for (; L < total; L += gridDim.x) {
    const bool has_next = L + (int)gridDim.x < total;
    int m0n = 0, n0n = 0, bzn = 0;
    if (has_next) decode(L + gridDim.x, m0n, n0n, bzn);
    f32x4 acc[TM2][TN2];
#pragma unroll
    for (int i = 0; i < TM2; ++i)
#pragma unroll
      for (int j = 0; j < TN2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < nk; t += 2) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int tt = t + u;
        const bf16_t* As = lds + u * STAGE;
        const bool more = tt + 1 < nk || has_next;
        const int tgt = tt + 2;  // the K-tile refilled into this stage (>= nk: the next tile's)
        const bool refill = tgt < nk || has_next;
        if (refill) {
          if (tgt < nk) {
            a.prep(ap, tgt * KT);
            b.prep(bp, tgt * KT);
          } else {
            if (tgt == nk) {
              a.aim(ap, m0n, bzn);
              b.aim(bp, n0n, bzn);
            }
            a.prep(ap, (tgt - nk) * KT);
            b.prep(bp, (tgt - nk) * KT);
          }
        }
#pragma unroll
        for (int i = 0; i < TM2; ++i) {
          const int cb = i & 1;
          if (i + 1 < TM2) {
            fa[cb ^ 1][0] = rd(As, arb + 16 * (i + 1), 0);
            fa[cb ^ 1][1] = rd(As, arb + 16 * (i + 1), 1);
          } else {
            __builtin_amdgcn_s_waitcnt(0xC07F);
            if (more) {
              // this wave's pieces of the next K-tile; in a tile's first K-tile
              // the previous tile's SPL epilogue stores are younger than them
              // (the first tile's K-tile 1 was waited for in the prologue)
              // (tt made opaque: a visible tt == 0 test makes hipcc peel the
              // first K-trip, a second copy of the loop that spills)
              int tq = tt;
              asm volatile("" : "+s"(tq));
              if (tq == 0) vm_wait<SPL>();
              else vm_wait<0>();
              __builtin_amdgcn_s_barrier();
              const bf16_t* Ns = lds + (u ^ 1) * STAGE;
#pragma unroll
              for (int j = 0; j < TN2; ++j) {
                fb[u ^ 1][0][j] = rd(Ns + A_EL, brb + 16 * j, 0);
                fb[u ^ 1][1][j] = rd(Ns + A_EL, brb + 16 * j, 1);
              }
              fa[cb ^ 1][0] = rd(Ns, arb, 0);
              fa[cb ^ 1][1] = rd(Ns, arb, 1);
            }
          }
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int j = 0; j < TN2; ++j) {
            f32x4 c = acc[i][j];
            if constexpr (SP) {  // single-plane operands (gemm_h2q_kernel)
              c = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[cb][0], fb[u][0][j], c, 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[cb][1], fb[u][1][j], c, 0, 0, 0);
            } else {
              c = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[cb][1], fb[u][0][j], c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[cb][0], fb[u][1][j], c, 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[cb][0], fb[u][0][j], c, 0, 0, 0);
            }
            if (i + 1 == TM2 && refill) {
#pragma unroll
              for (int q = 0; q < LPT; ++q)
                if (q * TN2 / LPT == j) dma_one(a, b, ap, bp, As, A_EL, wid, q);
            }
          }
          __builtin_amdgcn_s_setprio(0);
        }
      }
    }
    // epilogue: 16-row groups through this wave's staging rows. Its lane
    // offsets are derived from an opaque copy of the lane index so that they
    // are formed here, not hoisted out of the tile loop into registers that
    // would stay live across the K-loop.
    int el = lane;
    asm volatile("" : "+v"(el));
    // O16: a scale per 64-row group of the wave tile from its own maximum
    // (m16_tile_exp), recorded in ep.m16e for the output transform
    constexpr int NG = TM2 / 4 > 0 ? TM2 / 4 : 1;
    float osc[NG];
    if constexpr (O16) {
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        uint32_t mb = 0;
#pragma unroll
        for (int i = 4 * g; i < 4 * g + 4; ++i)
#pragma unroll
          for (int j = 0; j < TN2; ++j) amax_fold(mb, acc[i][j]);
        const int e = m16_tile_exp(mb);
        osc[g] = exp2i(e);
        const int r64 = (m0 + arb) / 64 + g, c64 = (n0 + brb) / 64;
        if (el == 0 && r64 < ep.m16e_rows)
          ep.m16e[((size_t)bz * ep.m16e_rows + r64) * (N / 64) + c64] = e;
      }
    }
    float* stg = (float*)(lds + 2 * STAGE) + wid * (16 * 64);
    const __amdgpu_buffer_rsrc_t orsrc =
        O16 ? __builtin_amdgcn_make_buffer_rsrc((void*)((bf16_t*)ep.out + (size_t)bz * ep.bstride),
                                                (short)0, M * ep.ld * 2, 0x00020000)
            : __builtin_amdgcn_make_buffer_rsrc((void*)(ep.out + (size_t)bz * ep.bstride), (short)0,
                                                M * ep.ld * 4, 0x00020000);
#pragma unroll
    for (int i = 0; i < TM2; ++i) {
#pragma unroll
      for (int j = 0; j < TN2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          stg[(4 * (el >> 4) + e) * 64 + ((16 * j) ^ ((el >> 4) << 4)) + (el & 15)] =
              O16 ? acc[i][j][e] * osc[i / 4 < NG ? i / 4 : 0] : (acc[i][j][e] * ia) * ib;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int r = it * 4 + (el >> 4), cc = el & 15;
        const f32x4 v = *(const f32x4*)&stg[r * 64 + ((4 * cc) ^ ((r >> 2) << 4))];
        const int m = m0 + arb + 16 * i + r, n = n0 + brb + 4 * cc;
        if constexpr (O16)
          __builtin_amdgcn_raw_buffer_store_b64(pack_f16x4(v), orsrc, (uint32_t)(m * ep.ld + n) * 2u,
                                                0, 0);
        else
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), orsrc,
                                                 (uint32_t)(m * ep.ld + n) * 4u, 0, 0);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    m0 = m0n;
    n0 = n0n;
    bz = bzn;
  }
}

// ---- fp32 -> h2 conversion (test / benchmark helper; the product path's
// operands come from their producers) -------------------------------------------
__global__ void __launch_bounds__(256) to_h2_kernel(const float* __restrict__ x, long long rows,
                                                   int C, H2Scale sc, bf16_t* __restrict__ out) {
  const float s = exp2i(h2_exp(sc));
  const int C4 = C / 4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < rows * C4;
       i += (long long)gridDim.x * 256) {
    const long long r = i / C4;
    const int c = (int)(i - r * C4) * 4;
    h2_store4(out + (size_t)r * 2 * C, c, *(const f32x4*)(x + (size_t)r * C + c), s);
  }
}

// ---- host ----------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, class AL, class BL>
static int launch_h2(dim3 grid, hipStream_t s, const typename AL::P& ap, const typename BL::P& bp,
                     const EpiH2P& ep, int M, int N, int K, int kchunk, int zsplit, H2Scale sa,
                     H2Scale sb) {
  constexpr int NT = WM * WN * 64;
  const long long total = (long long)grid.x * grid.y * grid.z;
  const int remap = split_xcd() && total % 8 == 0 && grid.z > 1 ? 1 : 0;
  hipLaunchKernelGGL((gemm_h2_kernel<BM, BN, WM, WN, AL, BL, EpiH2>), grid, dim3(NT), 0, s, ap, bp,
                     ep, M, N, K, kchunk, zsplit, remap, sa, sb);
  NSM_LAUNCH_CHECK("gemm_h2");
  return 0;
}

// NSM_H2_MF16=0: the forward / dgrad 256x256 tiles on v_mfma_f32_32x32x16_f16
// (gemm_h2_kernel) instead of 16x16x32 (gemm_h2q_kernel)
static bool h2_mf16() { static const bool v = env_flag("NSM_H2_MF16", true); return v; }

template <int BM, int BN, int WM, int WN, class AL, class BL, bool SP = false, bool O16 = false>
static int launch_h2q(dim3 grid, hipStream_t s, const typename AL::P& ap, const typename BL::P& bp,
                      const EpiH2P& ep, int M, int N, int K, H2Scale sa, H2Scale sb) {
  constexpr int NT = WM * WN * 64;
  const long long total = (long long)grid.x * grid.y * grid.z;
  const int remap = split_xcd() && total % 8 == 0 && grid.z > 1 ? 1 : 0;
  hipLaunchKernelGGL((gemm_h2q_kernel<BM, BN, WM, WN, AL, BL, SP, O16>), grid, dim3(NT), 0, s, ap, bp, ep,
                     M, N, K, K, 1, remap, sa, sb);
  NSM_LAUNCH_CHECK("gemm_h2q");
  return 0;
}

// NSM_H2P_NFAST=0: the persistent GEMM walks a batch entry's tiles M-fastest
// instead of N-fastest
static bool h2p_nfast() { static const bool v = env_flag("NSM_H2P_NFAST", true); return v; }

// NSM_H2_PERSIST=0: one tile per block (gemm_h2q_kernel) instead of the
// persistent grid (gemm_h2p_kernel)
static bool h2_persist() { static const bool v = env_flag("NSM_H2_PERSIST", true); return v; }

// whether a 256-row GEMM of `total` tiles over K f16 columns runs on the
// persistent grid (gemm_h2p_kernel) rather than one tile per block
static bool h2_persistent(long long total, int K) {
  return h2_persist() && K % 128 == 0 && total > cu_count() && total < (1ll << 30);
}

template <int BM, int BN, int WM, int WN, class AL, class BL, bool SP = false, bool O16 = false>
static int launch_h2p(dim3 grid, hipStream_t s, const typename AL::P& ap, const typename BL::P& bp,
                      const EpiH2P& ep, int M, int N, int K, H2Scale sa, H2Scale sb) {
  constexpr int NT = WM * WN * 64;
  const long long total = (long long)grid.x * grid.y * grid.z;
  hipLaunchKernelGGL((gemm_h2p_kernel<BM, BN, WM, WN, AL, BL, SP, O16>), dim3(cu_count()), dim3(NT), 0, s,
                     ap, bp, ep, M, N, K, (int)grid.x, (int)grid.y, (int)total, sa, sb,
                     h2p_nfast() ? 1 : 0);
  NSM_LAUNCH_CHECK("gemm_h2p");
  return 0;
}

// gemm_h2p_kernel (persistent) or gemm_h2q_kernel (one tile per block), as the
// caller's plan decided
template <int BM, int BN, int WM, int WN, class AL, class BL, bool SP = false, bool O16 = false>
static int launch_h2q_or_p(bool persistent, dim3 grid, hipStream_t s, const typename AL::P& ap,
                           const typename BL::P& bp, const EpiH2P& ep, int M, int N, int K,
                           H2Scale sa, H2Scale sb) {
  if (persistent)
    return launch_h2p<BM, BN, WM, WN, AL, BL, SP, O16>(grid, s, ap, bp, ep, M, N, K, sa, sb);
  return launch_h2q<BM, BN, WM, WN, AL, BL, SP, O16>(grid, s, ap, bp, ep, M, N, K, sa, sb);
}

// NSM_H2_TILE: force the forward / dgrad tile (0 = policy, 1 = 256x256,
// 2 = 256x128, 3 = 128x128)
static int h2_tile_env() { static const int v = (int)env_int("NSM_H2_TILE", 0); return v; }

// The single-plane GEMM's decision, shared by the launch below and the query
// entry nsm_wino_gemm_f16_plan: tile 1 = 256x256 (cout_p % 256 == 0), 2 =
// 256x128; form 1 = gemm_h2q_kernel, 2 = gemm_h2p_kernel. The same for fp32
// and f16 M.
struct WinoGemmF16Plan {
  int tile, form;
};
static WinoGemmF16Plan plan_wino_gemm_f16(long long T, int cin_p, int cout_p, int nb) {
  const int tile = cout_p % 256 == 0 ? 1 : 2;
  const long long total = (long long)ceil_div((int)T, 256) * (cout_p / (tile == 1 ? 256 : 128)) * nb;
  return WinoGemmF16Plan{tile, h2_persistent(total, cin_p) ? 2 : 1};
}

// batched M = T x N = cout GEMMs over K = cin channels of single-plane scaled
// f16 operands (the bf16 path's Winograd forward: V [nb][T][cin_p], U
// [nb][cout_p][cin_p]); 256-row tiles, N % 128 == 0 (host-checked)
// o16: M written as f16 (O16 above) into Mb's first half
// (called from nsm_conv_bf16.hip; declared in nsm_conv.h)
int nsm::wino_gemm_f16(const bf16_t* V, const bf16_t* U, long long T, int cin_p, int cout_p,
                       int nb, float* Mb, H2Scale sv, H2Scale su, hipStream_t s, bool o16,
                       int* m16e) {
  const int M = (int)T, N = cout_p, K = cin_p;
  H2RowsP ap{V, cin_p, M, (long long)T * cin_p};
  H2RowsP bp{U, cin_p, N, (long long)cout_p * cin_p};
  EpiH2P ep{Mb, cout_p, (long long)T * cout_p, m16e, (int)((T + 63) / 64)};
  const dim3 g256(ceil_div(M, 256), N / 256, nb), g128(ceil_div(M, 256), N / 128, nb);
  using R256 = H2RowsDma<256, 8>;
  using R128 = H2RowsDma<128, 8>;
  const WinoGemmF16Plan pl = plan_wino_gemm_f16(T, cin_p, cout_p, nb);
  const bool pers = pl.form == 2;
  if (o16)
    return pl.tile == 1
               ? launch_h2q_or_p<256, 256, 2, 4, R256, R256, true, true>(pers, g256, s, ap, bp, ep, M, N, K, sv, su)
               : launch_h2q_or_p<256, 128, 4, 2, R256, R128, true, true>(pers, g128, s, ap, bp, ep, M, N, K, sv, su);
  return pl.tile == 1
             ? launch_h2q_or_p<256, 256, 2, 4, R256, R256, true>(pers, g256, s, ap, bp, ep, M, N, K, sv, su)
             : launch_h2q_or_p<256, 128, 4, 2, R256, R128, true>(pers, g128, s, ap, bp, ep, M, N, K, sv, su);
}

// The forward / dgrad GEMM's decision, shared by the launch below and the
// query entry nsm_wino_gemm_h2_plan: tile 1 = 256x256, 2 = 256x128, 3 = 128x128,
// 4 = 256x64, 5 = 128x32 (a forced tile that cout_p does not divide falls to the
// next one that fits); form 0 = gemm_h2_kernel, 1 = gemm_h2q_kernel, 2 =
// gemm_h2p_kernel (the 256-row tiles only)
struct WinoGemmH2Plan {
  int tile, form;
};
static WinoGemmH2Plan plan_wino_gemm_h2(long long T, int cin_p, int cout_p, int nb) {
  const int M = (int)T, N = cout_p, K = 2 * cin_p;
  int tile = h2_tile_env();
  if (!tile) {
    if (N % 256 == 0 && (long long)ceil_div(M, 256) * (N / 256) * nb >= 768) tile = 1;
    else if (N % 128 == 0 && (long long)ceil_div(M, 256) * (N / 128) * nb >= 768) tile = 2;
    else if (N % 128 == 0) tile = 3;
    else tile = N % 64 == 0 ? 4 : 5;
  }
  if (tile < 1 || tile > 5) tile = 5;
  if (tile == 1 && N % 256) tile = 2;
  if (tile == 2 && N % 128) tile = 3;
  if (tile == 3 && N % 128) tile = 4;
  if (tile == 4 && N % 64) tile = 5;
  int form = 0;
  if (tile <= 2 && h2_mf16()) {
    const long long total = (long long)ceil_div(M, 256) * (N / (tile == 1 ? 256 : 128)) * nb;
    form = h2_persistent(total, K) ? 2 : 1;
  }
  return WinoGemmH2Plan{tile, form};
}

// batched M = T x N = cout GEMMs over K = cin channels (2 cin f16 columns)
static int wino_gemm_h2(const bf16_t* V, const bf16_t* U, long long T, int cin_p, int cout_p,
                        int nb, float* Mb, H2Scale sv, H2Scale su, hipStream_t s) {
  const int M = (int)T, N = cout_p, K = 2 * cin_p;
  H2RowsP ap{V, 2 * cin_p, M, (long long)T * 2 * cin_p};
  H2RowsP bp{U, 2 * cin_p, N, (long long)cout_p * 2 * cin_p};
  EpiH2P ep{Mb, cout_p, (long long)T * cout_p};
  const WinoGemmH2Plan pl = plan_wino_gemm_h2(T, cin_p, cout_p, nb);
  switch (pl.tile) {
    case 1: {
      const dim3 g(ceil_div(M, 256), N / 256, nb);
      using R = H2RowsDma<256, 8>;
      if (pl.form == 2) return launch_h2p<256, 256, 2, 4, R, R>(g, s, ap, bp, ep, M, N, K, sv, su);
      if (pl.form == 1) return launch_h2q<256, 256, 2, 4, R, R>(g, s, ap, bp, ep, M, N, K, sv, su);
      return launch_h2<256, 256, 2, 4, R, R>(g, s, ap, bp, ep, M, N, K, K, 1, sv, su);
    }
    case 2: {
      const dim3 g(ceil_div(M, 256), N / 128, nb);
      using RA = H2RowsDma<256, 8>;
      using RB = H2RowsDma<128, 8>;
      if (pl.form == 2) return launch_h2p<256, 128, 4, 2, RA, RB>(g, s, ap, bp, ep, M, N, K, sv, su);
      if (pl.form == 1) return launch_h2q<256, 128, 4, 2, RA, RB>(g, s, ap, bp, ep, M, N, K, sv, su);
      return launch_h2<256, 128, 4, 2, RA, RB>(g, s, ap, bp, ep, M, N, K, K, 1, sv, su);
    }
    case 3:
      return launch_h2<128, 128, 2, 2, H2RowsDma<128, 4>, H2RowsDma<128, 4>>(
          dim3(ceil_div(M, 128), N / 128, nb), s, ap, bp, ep, M, N, K, K, 1, sv, su);
    case 4:
      return launch_h2<256, 64, 4, 1, H2RowsDma<256, 4>, H2RowsDma<64, 4>>(
          dim3(ceil_div(M, 256), N / 64, nb), s, ap, bp, ep, M, N, K, K, 1, sv, su);
    default:
      return launch_h2<128, 32, 4, 1, H2RowsDma<128, 4>, H2RowsDma<32, 4>>(
          dim3(ceil_div(M, 128), ceil_div(N, 32), nb), s, ap, bp, ep, M, N, K, K, 1, sv, su);
  }
}

// NSM_WGRAD_Q=1: the KM weight-gradient GEMMs on v_mfma_f32_16x16x32_f16
// (gemm_h2q_kernel's KM form) instead of 32x32x16 (gemm_h2_kernel). Measured
// slower (B=8 step: conv6's 3x3 weight gradient 384 -> 468-478 us, 742.7 ->
// 723.1 frames/s A/B): each 16x16x32 fragment takes two transposing reads
// whose addresses depend on the lane through the XOR swizzle, one row-group
// ahead of its MFMAs, where the 32x32x16 form loads a whole k-step ahead.
static bool wgrad_q() { static const bool v = env_flag("NSM_WGRAD_Q", false); return v; }

// split-K launch of gemm_h2q_kernel (the KM weight-gradient form)
template <int BM, int BN, int WM, int WN, class AL, class BL, bool SP = false>
static int launch_h2qk(dim3 grid, hipStream_t s, const typename AL::P& ap, const typename BL::P& bp,
                       const EpiH2P& ep, int M, int N, int K, int kchunk, int zsplit, H2Scale sa,
                       H2Scale sb) {
  constexpr int NT = WM * WN * 64;
  const long long total = (long long)grid.x * grid.y * grid.z;
  const int remap = split_xcd() && total % 8 == 0 && grid.z > 1 ? 1 : 0;
  hipLaunchKernelGGL((gemm_h2q_kernel<BM, BN, WM, WN, AL, BL, SP>), grid, dim3(NT), 0, s, ap, bp, ep,
                     M, N, K, kchunk, zsplit, remap, sa, sb);
  NSM_LAUNCH_CHECK("gemm_h2q (KM)");
  return 0;
}

// NSM_F16_WG_KT64=0: the bf16 path's 256x256 Winograd weight-gradient GEMMs on
// 32-row K-tiles instead of 64-row ones (4 k-steps per barrier)
static bool f16_wg_kt64() { static const bool v = env_flag("NSM_F16_WG_KT64", true); return v; }

// weight-gradient GEMMs dU[xi][split] = dM[xi]^T V[xi] over the split's
// Winograd tiles (K): M = cout_p, N = cin_p, KM images of both h2 operands
// the bf16 path's Winograd weight gradient on single-plane f16 dM / V
// (F16PixDma, one product per k-step): dU[xi][split] = dM[xi]^T V[xi]
// (called from nsm_conv_bf16.hip; declared in nsm_conv.h)
int nsm::wino_wgrad_gemm_f16(const bf16_t* dM, const bf16_t* V, long long T, int cin_p,
                             int cout_p, int nb, int BM, int BN, int kchunk, int splits,
                             float* slab, H2Scale sdm, H2Scale sv, hipStream_t s) {
  const int M = cout_p, N = cin_p, K = (int)T;
  H2PixP ap{dM, cout_p, cout_p, (int)T, T * cout_p};
  H2PixP bp{V, cin_p, cin_p, (int)T, T * cin_p};
  EpiH2P ep{slab, N, (long long)M * N};
  const dim3 grid(ceil_div(M, BM), ceil_div(N, BN), nb * splits);
  const long long total = (long long)grid.x * grid.y * grid.z;
  const int remap = split_xcd() && total % 8 == 0 && grid.z > 1 ? 1 : 0;
  if (wgrad_q()) {
    if (BM == 256 && BN == 256)
      return launch_h2qk<256, 256, 2, 4, F16PixDma<256, 8>, F16PixDma<256, 8>, true>(
          grid, s, ap, bp, ep, M, N, K, kchunk, splits, sdm, sv);
    if (BM == 128 && BN == 128)
      return launch_h2qk<128, 128, 2, 2, F16PixDma<128, 4>, F16PixDma<128, 4>, true>(
          grid, s, ap, bp, ep, M, N, K, kchunk, splits, sdm, sv);
    return fail(NSM_E_ARG, "wino_wgrad_gemm_f16: tile %dx%d", BM, BN);
  }
  if (BM == 256 && BN == 256 && f16_wg_kt64())
    hipLaunchKernelGGL((gemm_h2_kernel<256, 256, 2, 4, F16PixDma<256, 8, 64>, F16PixDma<256, 8, 64>, EpiH2,
                                       true>),
                       grid, dim3(512), 0, s, ap, bp, ep, M, N, K, kchunk, splits, remap, sdm, sv);
  else if (BM == 256 && BN == 256)
    hipLaunchKernelGGL((gemm_h2_kernel<256, 256, 2, 4, F16PixDma<256, 8>, F16PixDma<256, 8>, EpiH2, true>),
                       grid, dim3(512), 0, s, ap, bp, ep, M, N, K, kchunk, splits, remap, sdm, sv);
  else if (BM == 128 && BN == 128)
    hipLaunchKernelGGL((gemm_h2_kernel<128, 128, 2, 2, F16PixDma<128, 4>, F16PixDma<128, 4>, EpiH2, true>),
                       grid, dim3(256), 0, s, ap, bp, ep, M, N, K, kchunk, splits, remap, sdm, sv);
  else
    return fail(NSM_E_ARG, "wino_wgrad_gemm_f16: tile %dx%d", BM, BN);
  NSM_LAUNCH_CHECK("wino_wgrad_gemm_f16");
  return 0;
}

static int wino_wgrad_gemm_h2(const bf16_t* dM, const bf16_t* V, long long T, int cin_p,
                              int cout_p, int nb, int BM, int BN, int kchunk, int splits,
                              float* slab, H2Scale sdm, H2Scale sv, hipStream_t s) {
  const int M = cout_p, N = cin_p, K = (int)T;
  H2PixP ap{dM, 2 * cout_p, 2 * cout_p, (int)T, T * 2 * cout_p};
  H2PixP bp{V, 2 * cin_p, 2 * cin_p, (int)T, T * 2 * cin_p};
  EpiH2P ep{slab, N, (long long)M * N};
  const dim3 grid(ceil_div(M, BM), ceil_div(N, BN), nb * splits);
#define NSM_WH(bm, bn, wm, wn)                                                                   \
  if (BM == bm && BN == bn)                                                                      \
    return wgrad_q() ? launch_h2qk<bm, bn, wm, wn, H2PixDma<2 * bm, wm * wn>,                    \
                                   H2PixDma<2 * bn, wm * wn>>(grid, s, ap, bp, ep, M, N, K,      \
                                                              kchunk, splits, sdm, sv)           \
                     : launch_h2<bm, bn, wm, wn, H2PixDma<2 * bm, wm * wn>,                      \
                                 H2PixDma<2 * bn, wm * wn>>(grid, s, ap, bp, ep, M, N, K, kchunk, \
                                                            splits, sdm, sv);
  NSM_WH(256, 256, 2, 4)
  NSM_WH(128, 128, 2, 2)
  NSM_WH(128, 64, 2, 2)
  NSM_WH(64, 128, 2, 2)
  NSM_WH(64, 64, 2, 2)
  NSM_WH(128, 32, 4, 1)
  NSM_WH(32, 128, 1, 4)
  NSM_WH(64, 32, 2, 1)
  NSM_WH(32, 64, 1, 2)
#undef NSM_WH
  if (wgrad_q())
    return launch_h2qk<32, 32, 1, 1, H2PixDma<64, 1>, H2PixDma<64, 1>>(grid, s, ap, bp, ep, M, N, K,
                                                                     kchunk, splits, sdm, sv);
  return launch_h2<32, 32, 1, 1, H2PixDma<64, 1>, H2PixDma<64, 1>>(grid, s, ap, bp, ep, M, N, K,
                                                                   kchunk, splits, sdm, sv);
}
