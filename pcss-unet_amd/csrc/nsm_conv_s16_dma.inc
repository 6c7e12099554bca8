// LDS-DMA pipelined bf16 implicit-GEMM convolutions (BASELINE config 3).
// Included from nsm_conv_s16.inc only (shares its loaders' parameter blocks and
// epilogues), so once per 16-bit format. The format-independent LDS-DMA
// helpers (dswz, kmswz, dma16, vm_wait, dma_barrier, wait_retire, dma_one,
// lgkm_fence), which the h2 GEMMs use too, are in nsm_conv.h.
//
// For the large prologue-free convolutions: 3x3 forward and input-gradient
// with Cin % 64 == 0 (conv4..conv8), and the 3x3 weight gradient.
//   * Operands go global -> LDS by `buffer_load_dwordx4 ... lds` (no VGPR
//     round trip, no ds_write; OOB lanes are still zero-filled by the buffer
//     descriptor), through a STAGES-deep ring of K-tiles (BK = 64).
//   * Each K-tile is retired by a counted `s_waitcnt vmcnt(N)` and ONE raw
//     `s_barrier`: STAGES-2 younger tiles stay in flight across it, and the
//     DMA of tile t+STAGES-1 is issued right after it, into the stage every
//     wave finished reading before the barrier.
//   * A DMA instruction writes 64 lanes x 16 B = 1 KiB contiguously, so LDS
//     images are unpadded; bank conflicts are removed by XOR-swizzling 16-B
//     chunks, applied on the GLOBAL side (lane l of an instruction fetches the
//     logical chunk that belongs at its physical slot) and on the read side.
//
// MK image (forward / dgrad; K = (tap, channel)): [rows][64] bf16, 128-B rows.
//   Chunk c of row r sits at physical chunk c ^ ((r >> 1) & 7); the ds_read_b128
//   lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} (MI355X_MICROARCH.md §LDS)
//   of a fragment read (32 consecutive rows, one chunk) then hit 16 distinct
//   16-B bank slots each.
// KM image (weight gradient; K = pixels): [64 pixels][R channels], 2R-B rows,
//   read with two ds_read_b64_tr_b16 per fragment (4 pixel rows x 16 channels
//   per 16-lane group, delivered transposed). The 16-B chunk c of pixel row k
//   sits at c ^ kmswz(k): the 4 rows of a 32-lane group land in distinct 64-B
//   bank quarters.

// Fragment of k-step s (0..3), rows rb..rb+31 of the tile (lane & 31 selects
// the row). MK: one plain ds_read_b128 (counted by hipcc). KM: two
// ds_read_b64_tr_b16 in inline asm: hipcc's waitcnt pass cannot tell the
// transposed-read builtin from a read of the stages still being filled and
// drains every DMA (vmcnt(0)) before it, which serialises the pipeline. The
// asm reads are invisible to it, so the kernel waits for them itself
// (lgkm_fence: s_waitcnt lgkmcnt(0), then hold() pins the destinations).
template <bool KM, int R, int BK = DBK>
struct FragRd {
  static constexpr int NR = KM ? 2 : 1;  // LDS reads per fragment
  bf16x8 v;
  s16x4 lo, hi;
  __device__ __forceinline__ void issue(const bf16_t* S, int rb, int lane, int s) {
    if constexpr (!KM) {
      const int row = rb + (lane & 31), chunk = 2 * s + (lane >> 5);
      v = __builtin_bit_cast(bf16x8, *(const u32x4*)&S[row * BK + ((chunk ^ dswz<BK>(row)) << 3)]);
    } else {
      const int h = lane >> 5, g16 = (lane >> 4) & 1, q = (lane >> 2) & 3, p = lane & 3;
      const int k = 16 * s + 8 * h + q;                    // pixel row (second read: k + 4)
      const int lc = (rb >> 3) + 2 * g16 + (p >> 1);       // logical 16-B chunk
      const int sub = (p & 1) * 4;                         // bf16 offset inside the chunk
      typedef __attribute__((address_space(3))) bf16_t lds_bf16;
      const uint32_t a0 = (uint32_t)(uintptr_t)(lds_bf16*)(S + k * R + ((lc ^ kmswz<R>(k)) << 3) + sub);
      const uint32_t a1 =
          (uint32_t)(uintptr_t)(lds_bf16*)(S + (k + 4) * R + ((lc ^ kmswz<R>(k + 4)) << 3) + sub);
      asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(a0));
      asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(hi) : "v"(a1));
    }
  }
  __device__ __forceinline__ void hold() {
    if constexpr (KM) asm volatile("" : "+v"(lo), "+v"(hi));
  }
  __device__ __forceinline__ bf16x8 get() const {
    if constexpr (!KM) return v;
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 w = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return __builtin_bit_cast(bf16x8, w);
  }
};
// 16x16x32 accumulators -> the 32x32 MFMA layout every epilogue reads.
// 16x16 quadrant (a, b) lane l reg j holds C[16a + 4 (l >> 4) + j][16b + (l & 15)];
// the 32x32 layout wants, at lane l reg i, C[(i & 3) + 8 (i >> 2) + 4 (l >> 5)][l & 31]:
// quadrant (i >> 3, (l >> 4) & 1), source lane (l & 15) + 16 (2 ((i >> 2) & 1) + (l >> 5)),
// source reg i & 3
template <int TM, int TN>
__device__ __forceinline__ void acc16_to_32(const f32x4 (&acc4)[2 * TM][2 * TN],
                                            f32x16 (&acc)[TM][TN], int lane) {
  const bool hib = (lane >> 4) & 1;
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int src = ((lane & 15) + 16 * (2 * ((i >> 2) & 1) + (lane >> 5))) << 2;
        const int qa = 2 * tm + (i >> 3);
        const float v0 = __int_as_float(
            __builtin_amdgcn_ds_bpermute(src, __float_as_int(acc4[qa][2 * tn][i & 3])));
        const float v1 = __int_as_float(
            __builtin_amdgcn_ds_bpermute(src, __float_as_int(acc4[qa][2 * tn + 1][i & 3])));
        acc[tm][tn][i] = hib ? v1 : v0;
      }
}

// The pipelined GEMM: block tile BM x BN, WM x WN waves of (BM/WM) x (BN/WN),
// grid (ceil(N/BN), ceil(M/BM), splits); split z covers K range
// [z*kchunk, min(K,(z+1)*kchunk)), kchunk % 64 == 0.
template <int BM, int BN, int WM, int WN, int STAGES, int BK, int REFILL, bool PF, class AL,
          class BL, class EP>
__global__ void __launch_bounds__(WM * WN * 64)
    gemm_bf16_dma_kernel(typename AL::P ap, typename BL::P bp, typename EP::P ep, int M, int N,
                         int K, int kchunk, int xcd_remap) {
  constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);
  constexpr int A_EL = BM * BK, STAGE = (BM + BN) * BK;
  constexpr int KS = BK / 16;  // 16-deep MFMA k-steps per K-tile
  constexpr int LPT = AL::NI + BL::NI;
  static_assert(STAGES >= 2 && STAGES <= 8 && (BK == 32 || BK == 64), "stages");
  // ONE __shared__ object: a second one beside the DMA target can make hipcc
  // drain vmcnt before LDS reads (cdna_hip_programming.md §5, trap 4(a))
  __shared__ __attribute__((aligned(1024))) bf16_t lds[STAGES * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  // xcd_remap (grid size % 8 == 0): blocks are dispatched round-robin over the
  // 8 XCDs; renumber so each XCD owns a contiguous range of tiles (N fastest,
  // then M, then split), i.e. neighbouring tiles that share operand rows in
  // its own L2
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (xcd_remap) {
    const uint32_t G = gridDim.x * gridDim.y * gridDim.z;
    const uint32_t bid = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const uint32_t L = (bid & 7u) * (G >> 3) + (bid >> 3);
    bx = (int)(L % gridDim.x);
    by = (int)((L / gridDim.x) % gridDim.y);
    bz = (int)(L / (gridDim.x * gridDim.y));
  }
  const int m0 = by * BM, n0 = bx * BN;
  const int split = bz;
  const int kbeg = split * kchunk;
  const int kend = min(K, kbeg + kchunk);
  const int nk = (kend - kbeg + BK - 1) / BK;

  AL a;
  BL b;
  a.init(ap, m0, kbeg, kend, wid, lane);
  b.init(bp, n0, kbeg, kend, wid, lane);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // an epilogue with operands of its own (EpiBnBwdB: Y1) loads them first:
  // older than every DMA below, they retire before the first counted
  // vmcnt wait returns, which then stays exact for the DMA pieces
  constexpr bool PRE = s16_has_pre<EP>::value;
  typename s16_pre_of<EP, TM, TN>::type pre;
  if constexpr (PRE)
    EP::template prefetch<TM, TN, WM, WN>(ep, pre, m0 + wm * TM * 32, n0 + wn * TN * 32, lane, M, N);

  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nk) {
      a.prep(ap, kbeg + s * BK);
      b.prep(bp, kbeg + s * BK);
#pragma unroll
      for (int j = 0; j < LPT; ++j) dma_one(a, b, ap, bp, lds + s * STAGE, A_EL, wid, j);
    }

  const int arb = wm * TM * 32, brb = wn * TN * 32;
  if constexpr (REFILL == 3) {
    // Cross-tile pipeline (2 stages, MK operands): the K-tile barrier sits
    // between the fragment reads and the MFMAs of the LAST k-step, so the
    // first fragments of the next tile are read under those 8 MFMAs instead
    // of after a drained barrier; the refill of the stage just released goes
    // out after the barrier, one piece between consecutive MFMAs.
    static_assert(STAGES == 2 && KS >= 2, "cross-tile pipeline");
    constexpr bool KMR = AL::KM || BL::KM;  // asm transposed reads: fenced by hand
    constexpr int NRT = TM * FragRd<AL::KM, BM, BK>::NR + TN * FragRd<BL::KM, BN, BK>::NR;
    if (nk > 1) {  // both stages start free: tile 1 goes out with tile 0
      a.prep(ap, kbeg + BK);
      b.prep(bp, kbeg + BK);
#pragma unroll
      for (int j = 0; j < LPT; ++j) dma_one(a, b, ap, bp, lds + STAGE, A_EL, wid, j);
      vm_wait<LPT>();
    } else {
      vm_wait<0>();
    }
    dma_barrier();
    FragRd<AL::KM, BM, BK> fa[2][TM];
    FragRd<BL::KM, BN, BK> fb[2][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) fa[0][tm].issue(lds, arb + tm * 32, lane, 0);
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) fb[0][tn].issue(lds + A_EL, brb + tn * 32, lane, 0);
    for (int t = 0; t < nk; ++t) {
      const bf16_t* As = lds + (t & 1) * STAGE;
      const bf16_t* Bs = As + A_EL;
#pragma unroll
      for (int s = 0; s < KS - 1; ++s) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) fa[(s + 1) & 1][tm].issue(As, arb + tm * 32, lane, s + 1);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) fb[(s + 1) & 1][tn].issue(Bs, brb + tn * 32, lane, s + 1);
        if constexpr (KMR) {  // k-step s's reads in, s+1's still in flight
          lgkm_fence_n<NRT>();
#pragma unroll
          for (int tm = 0; tm < TM; ++tm) fa[s & 1][tm].hold();
#pragma unroll
          for (int tn = 0; tn < TN; ++tn) fb[s & 1][tn].hold();
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = mfma_s16_32(
                fa[s & 1][tm].get(), fb[s & 1][tn].get(), acc[tm][tn], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
      const bool more = t + 1 < nk, refill = t + 2 < nk;
      // the scalar offsets of tile t+2 before the reads below: prep may
      // reload kernel arguments (SMEM shares lgkmcnt with the LDS reads)
      if (refill) {
        a.prep(ap, kbeg + (t + 2) * BK);
        b.prep(bp, kbeg + (t + 2) * BK);
      }
      // this wave's reads of stage t&1 retired. The lgkmcnt(0) is the
      // compiler's own s_waitcnt, on every path (also the last tile's), so its
      // scoreboard knows the last k-step's fragments are in and the MFMAs
      // below do not wait for the next tile's reads issued after it
      __builtin_amdgcn_s_waitcnt(0xC07F);  // vmcnt 63, expcnt 7, lgkmcnt 0
      constexpr int L = (KS - 1) & 1;
      if constexpr (KMR) {
        lgkm_fence();
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) fa[L][tm].hold();
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) fb[L][tn].hold();
      }
      if (more) {
        vm_wait<0>();  // this wave's pieces of tile t+1
        __builtin_amdgcn_s_barrier();  // everyone's reads retired, pieces landed
        const bf16_t* Ns = lds + ((t + 1) & 1) * STAGE;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) fa[0][tm].issue(Ns, arb + tm * 32, lane, 0);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) fb[0][tn].issue(Ns + A_EL, brb + tn * 32, lane, 0);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
          acc[tm][tn] = mfma_s16_32(fa[L][tm].get(), fb[L][tn].get(),
                                                                acc[tm][tn], 0, 0, 0);
          if (refill) {
            const int q = tm * TN + tn;
#pragma unroll
            for (int i = 0; i < LPT; ++i)
              if (i * (TM * TN) / LPT == q) dma_one(a, b, ap, bp, As, A_EL, wid, i);
          }
        }
      __builtin_amdgcn_s_setprio(0);
    }
  } else if constexpr (REFILL == 4) {
    // The cross-tile pipeline of REFILL 3 on v_mfma_f32_16x16x32_bf16: the
    // same K-tiles, LDS images, DMA pieces and fragment bytes, but each 32x32
    // tile is computed as four 16x16 quadrants with a 32-deep k-step (2 per
    // K-tile). Equal cycles per FLOP; MI355X_MICROARCH.md §DVFS (7): the
    // 16x16x32 shape holds a higher clock under load (1.12-1.15x FLOP/s with
    // LDS-fed operands). The accumulators are permuted into the 32x32 layout
    // at the end so every epilogue is shared.
    static_assert(STAGES == 2 && BK == 64 && !AL::KM && !BL::KM, "16x16x32 pipeline");
    constexpr int KS2 = BK / 32, TM2 = 2 * TM, TN2 = 2 * TN;
    f32x4 acc4[TM2][TN2];
#pragma unroll
    for (int i = 0; i < TM2; ++i)
#pragma unroll
      for (int j = 0; j < TN2; ++j) acc4[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // fragment of k-step s (32 deep) for rows rb..rb+15: lane supplies row
    // lane & 15, k = 32 s + 8 (lane >> 4) .. +7 (one 16-B chunk)
    auto rd = [&](const bf16_t* S, int rb, int s) {
      const int row = rb + (lane & 15), chunk = 4 * s + (lane >> 4);
      return __builtin_bit_cast(bf16x8, *(const u32x4*)&S[row * BK + ((chunk ^ dswz<BK>(row)) << 3)]);
    };
    if (nk > 1) {
      a.prep(ap, kbeg + BK);
      b.prep(bp, kbeg + BK);
#pragma unroll
      for (int j = 0; j < LPT; ++j) dma_one(a, b, ap, bp, lds + STAGE, A_EL, wid, j);
      vm_wait<LPT>();
    } else {
      vm_wait<0>();
    }
    dma_barrier();
    // A fragments single-buffered and refilled right behind the 4 MFMAs that
    // consume them (fits 2 waves per SIMD without spills); B double-buffered
    static_assert(KS2 == 2, "two 32-deep k-steps per K-tile");
    bf16x8 fa[TM2], fb[2][TN2];
#pragma unroll
    for (int i = 0; i < TM2; ++i) fa[i] = rd(lds, arb + 16 * i, 0);
#pragma unroll
    for (int j = 0; j < TN2; ++j) fb[0][j] = rd(lds + A_EL, brb + 16 * j, 0);
    for (int t = 0; t < nk; ++t) {
      const bf16_t* As = lds + (t & 1) * STAGE;
      const bf16_t* Bs = As + A_EL;
#pragma unroll
      for (int j = 0; j < TN2; ++j) fb[1][j] = rd(Bs, brb + 16 * j, 1);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < TM2; ++i) {
#pragma unroll
        for (int j = 0; j < TN2; ++j)
          acc4[i][j] = mfma_s16_16(fa[i], fb[0][j], acc4[i][j], 0, 0, 0);
        fa[i] = rd(As, arb + 16 * i, 1);
      }
      __builtin_amdgcn_s_setprio(0);
      const bool more = t + 1 < nk, refill = t + 2 < nk;
      if (refill) {
        a.prep(ap, kbeg + (t + 2) * BK);
        b.prep(bp, kbeg + (t + 2) * BK);
      }
      __builtin_amdgcn_s_waitcnt(0xC07F);  // vmcnt 63, expcnt 7, lgkmcnt 0 (see REFILL 3)
      const bf16_t* Ns = lds + ((t + 1) & 1) * STAGE;
      if (more) {
        vm_wait<0>();
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int j = 0; j < TN2; ++j) fb[0][j] = rd(Ns + A_EL, brb + 16 * j, 0);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < TM2; ++i) {
#pragma unroll
        for (int j = 0; j < TN2; ++j) {
          acc4[i][j] = mfma_s16_16(fa[i], fb[1][j], acc4[i][j], 0, 0, 0);
          if (refill) {
            const int q = i * TN2 + j;
#pragma unroll
            for (int p = 0; p < LPT; ++p)
              if (p * (TM2 * TN2) / LPT == q) dma_one(a, b, ap, bp, As, A_EL, wid, p);
          }
        }
        if (more) fa[i] = rd(Ns, arb + 16 * i, 0);
      }
      __builtin_amdgcn_s_setprio(0);
    }
    acc16_to_32<TM, TN>(acc4, acc, lane);
  } else {
  int cur = 0, nxt = STAGES - 1;
  for (int t = 0; t < nk; ++t) {
    wait_retire<LPT, STAGES - 2>(min(STAGES - 2, nk - 1 - t));
    dma_barrier();
    const bool refill = t + STAGES - 1 < nk;
    if (refill) {
      a.prep(ap, kbeg + (t + STAGES - 1) * BK);
      b.prep(bp, kbeg + (t + STAGES - 1) * BK);
      // REFILL 1: the whole refill goes out before this tile's first LDS read
      // (the longest time in flight); 0: spread over the k-steps, behind each
      // k-step's fragment reads; 2: spread over the k-steps, each piece placed
      // between two of the k-step's MFMAs
      if constexpr (REFILL == 1) {
#pragma unroll
        for (int j = 0; j < LPT; ++j) dma_one(a, b, ap, bp, lds + nxt * STAGE, A_EL, wid, j);
      }
    }
    const bf16_t* As = lds + cur * STAGE;
    const bf16_t* Bs = As + A_EL;
    const bf16_t* Ns = lds + nxt * STAGE;
    // PF: fragments double-buffered, the reads of k-step s+1 issued ahead of
    // the MFMAs of k-step s (within the K-tile: the next tile needs the barrier)
    FragRd<AL::KM, BM, BK> fa[PF ? 2 : 1][TM];
    FragRd<BL::KM, BN, BK> fb[PF ? 2 : 1][TN];
    if constexpr (PF) {
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) fa[0][tm].issue(As, arb + tm * 32, lane, 0);
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) fb[0][tn].issue(Bs, brb + tn * 32, lane, 0);
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      constexpr int NB = PF ? 2 : 1;
      const int cb = PF ? (s & 1) : 0;
      const int rs = PF ? s + 1 : s;  // k-step whose fragments are read now
      if (rs < KS) {
        const int rb = PF ? (rs & 1) : 0;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) fa[rb % NB][tm].issue(As, arb + tm * 32, lane, rs);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) fb[rb % NB][tn].issue(Bs, brb + tn * 32, lane, rs);
      }
      // the refill DMAs are spread over the k-steps, issued behind this
      // k-step's fragment reads and ahead of its MFMAs
      const int j0 = (s * LPT + KS - 1) / KS, j1 = ((s + 1) * LPT + KS - 1) / KS;
      if (REFILL == 0 && refill) {
#pragma unroll
        for (int j = j0; j < j1; ++j) dma_one(a, b, ap, bp, Ns, A_EL, wid, j);
      }
      if constexpr (AL::KM || BL::KM) {
        // wait for this k-step's reads only (the prefetched ones stay in flight)
        if (PF && s + 1 < KS) lgkm_fence_n<TM * FragRd<AL::KM, BM, BK>::NR + TN * FragRd<BL::KM, BN, BK>::NR>();
        else lgkm_fence();
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) fa[cb][tm].hold();
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) fb[cb][tn].hold();
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
          acc[tm][tn] = mfma_s16_32(fa[cb][tm].get(), fb[cb][tn].get(),
                                                                acc[tm][tn], 0, 0, 0);
          if constexpr (REFILL == 2) {
            // piece j0 + i of this k-step after MFMA i * TM*TN / (j1 - j0)
            const int q = tm * TN + tn, n = j1 - j0;
            if (refill) {
#pragma unroll
              for (int i = 0; i < LPT; ++i)
                if (i < n && i * (TM * TN) / n == q) dma_one(a, b, ap, bp, Ns, A_EL, wid, j0 + i);
            }
          }
        }
      __builtin_amdgcn_s_setprio(0);
    }
    cur = cur + 1 == STAGES ? 0 : cur + 1;
    nxt = nxt + 1 == STAGES ? 0 : nxt + 1;
  }
  }
  dma_barrier();  // the epilogue reuses the LDS as scratch
  EpiCtx cx{m0, n0, m0 + arb, n0 + brb, wm, wn, lane, (float*)lds, by, bz};
  if constexpr (PRE) EP::template apply_pre<TM, TN, WM, WN>(ep, acc, cx, M, N, pre);
  else EP::template apply<TM, TN, WM, WN>(ep, acc, cx, M, N, split);
}

// ---- halo-tiled direct 3x3 convolution (stride 1, pad 1) -------------------------
// The forward / input-gradient 3x3 of the narrow layers (64 or 128 output
// channels, images 64..256 pixels wide: conv3, conv4, conv8, conv9 and their
// dgrads) as a direct convolution over a halo tile held in LDS. The im2col
// GEMM above fetches every activation row once per tap into LDS (9x per
// channel chunk: 64 KB of A per 8.4 MFLOP K-tile at 512x128); here a chunk's
// activations enter LDS once, with a 1-row / 1-pixel border, and the 9 taps
// read them shifted.
//   * Block tile: 512 output pixels = RT = 512 / WD whole image rows (GEMM rows
//     stay contiguous, so the GEMM epilogues apply unchanged) x BN output
//     channels; 8 waves of 128x64 (BN 128) or 64x64 (BN 64) on 16x16x32 MFMAs.
//   * K walk: 32-channel chunks, the 9 taps of a chunk consecutive (K-tile =
//     one tap of one chunk). The chunk's halo, (RT + 2) rows x (WD + 2) pixels
//     x 32 channels at 64 B per pixel, sits in one of two LDS buffers; tap
//     (dy, dx) reads it shifted by dy (WD + 2) + dx pixels. The next chunk's
//     halo streams into the other buffer one 1-KiB DMA piece per wave per tap
//     (taps 0..HPW-1). Its two pad columns are zeroed once and never DMA'd; its
//     rows outside the image arrive as zeros (out-of-range descriptor offsets).
//   * B (packed weights [N][9 cin], the K-tile's 32 columns): a 3-stage ring
//     refilled two K-tiles ahead, one 1-KiB piece per wave (BN 128).
//   * One barrier per K-tile, after the first half of its MFMAs; the next
//     K-tile's fragments load under the second half.
//   * 16-B chunk c of LDS pixel p (or B row p) sits at c ^ ((p >> 1) & 2): the
//     16 consecutive pixels of a 16x16x32 fragment read then hit 16 distinct
//     16-B bank slots in every ds_read_b128 lane group (MI355X_MICROARCH.md
//     §LDS: groups {0-3,12-15,20-27}, ...; rows r, r+4, r+8, r+12 of one residue
//     read chunks c, c^1, c^1, c).
struct HaloPB {
  const bf16_t* x;  // NHWC activations, row stride ld elements
  const bf16_t* w;  // packed weights [nrows][ldw = 9 cin]
  int ld, cin, H, W, ldw, nrows;
};

__device__ __forceinline__ int halo_swz(int p) { return (p >> 1) & 2; }

template <int WD, int BN, int SB, class EP>
__global__ void __launch_bounds__(512)
    conv3x3_halo_kernel(HaloPB p, typename EP::P ep, int M, int N, int xcd_remap) {
  constexpr int WM = BN == 128 ? 4 : 8, WN = 8 / WM;
  constexpr int BM = 512, TM2 = BM / (WM * 16), TN2 = BN / (WN * 16);
  static_assert(TN2 == 4 && (TM2 == 8 || TM2 == 4), "wave tiles 128x64 / 64x64");
  // LDS row stride WD + 8 pixels (== 0 mod 8): a fragment's first pixel then
  // sits at 1 + dx (mod 8) for every row group and tap row, so its swizzle
  // phase, and with it each lane's offset, is one of three registers
  constexpr int RT = BM / WD, HW2 = WD + 8, HROWS = RT + 2;
  constexpr int HBUF = HROWS * HW2 * 32;  // elements per halo buffer
  constexpr int SEGS = WD / 16;           // 1-KiB pieces per halo row
  constexpr int NH = HROWS * SEGS, HPW = NH / 8;
  static_assert(NH % 8 == 0 && HPW >= 1 && HPW <= 8, "halo: at most one piece per wave and tap");
  // B ring: SB stages refilled D = SB - 1 K-tiles ahead
  constexpr int D = SB - 1, BST = BN * 32, NBP = BN / 16;  // refill distance, stage elements, pieces
  static_assert(SB >= 3 && SB <= 5, "B ring");
  // At a chunk boundary's barrier the wait leaves the last D - 1 K-tiles'
  // pieces in flight; the next chunk's halo pieces go out at taps 0..HPW-1, so
  // every one of them must be at least D - 1 taps older than tap 9 (ADVICE r05)
  static_assert(HPW <= 10 - D, "halo pieces still in flight when the next chunk reads the halo");
  static_assert(NBP <= 8, "B pieces");
  // (at least the 512 x BN bf16 tile EpiStoreB stages through the LDS)
  constexpr int LDS_EL = 2 * HBUF + SB * BST > BM * BN ? 2 * HBUF + SB * BST : BM * BN;
  __shared__ __attribute__((aligned(1024))) bf16_t lds[LDS_EL];
  bf16_t* const hb = lds;
  bf16_t* const bs = lds + 2 * HBUF;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  int by = blockIdx.x, bx = blockIdx.y;
  if (xcd_remap) {  // XCD-contiguous M tiles: neighbours share halo rows in one L2
    const uint32_t G = gridDim.x * gridDim.y;
    const uint32_t bid = blockIdx.x + gridDim.x * blockIdx.y;
    const uint32_t L = (bid & 7u) * (G >> 3) + (bid >> 3);
    by = (int)(L % gridDim.x);
    bx = (int)(L / gridDim.x);
  }
  const int m0 = by * BM, n0 = bx * BN;
  const int yg0 = m0 / WD;  // b * H + y0: the tile's first image row
  const int y0 = yg0 % p.H;
  const int base_row = max(0, yg0 - 1);
  const __amdgpu_buffer_rsrc_t ar =
      make_rsrc_b(p.x + (size_t)base_row * WD * p.ld, (long long)(M - base_row * WD) * p.ld);
  const __amdgpu_buffer_rsrc_t wr =
      make_rsrc_b(p.w + (size_t)n0 * p.ldw, (long long)(p.nrows - n0) * p.ldw);

  // halo piece k of this wave (q = wid * HPW + k) at channel c0 into buffer buf:
  // offsets formed at issue (once per K-tile), not held in registers across
  // the K loop
  auto issue_h = [&](int k, int buf, int c0) {
    const int q = wid * HPW + k, hy = q / SEGS, seg = q - hy * SEGS;
    const int pix = hy * HW2 + 1 + seg * 16;  // LDS pixel of the piece's first lane quad
    const int x = seg * 16 + (lane >> 2);
    const int c = (lane & 3) ^ halo_swz(pix + (lane >> 2));
    const bool ok = (unsigned)(y0 - 1 + hy) < (unsigned)p.H;
    const uint32_t off =
        ((uint32_t)(((yg0 - 1 + hy - base_row) * WD + x) * p.ld + c0 + c * 8) * 2u) | (ok ? 0u : OOB);
    dma16(ar, hb + buf * HBUF + pix * 32, off);
  };
  const bool bmine = wid < NBP;  // BN 64: waves 4..7 load no B
  uint32_t woff;
  {
    const int row = wid * 16 + (lane >> 2);
    const int c = (lane & 3) ^ halo_swz(row);
    woff = ((uint32_t)(row * p.ldw + c * 8) * 2u) | (n0 + row < p.nrows ? 0u : OOB);
  }
  auto issue_b = [&](int kt) {  // K-tile kt = (chunk j, tap t): columns t cin + 32 j
    const int j = kt / 9, t = kt - 9 * j;
    dma16(wr, bs + (kt % SB) * BST + wid * 512, woff + (uint32_t)(t * p.cin + 32 * j) * 2u);
  };

  // the pad columns of both halo buffers: zero for the whole kernel
  for (int e = tid; e < 2 * HROWS * 8; e += 512) {
    const int q4 = e & 3, side = (e >> 2) & 1, r = (e >> 3) % HROWS, buf = (e >> 3) / HROWS;
    *(u32x4*)&hb[buf * HBUF + (r * HW2 + (side ? WD + 1 : 0)) * 32 + q4 * 8] = u32x4{0u, 0u, 0u, 0u};
  }
  const int nch = p.cin / 32, nkt = 9 * nch;  // nkt >= 9
  for (int k = 0; k < HPW; ++k) issue_h(k, 0, 0);
  if (bmine) {
    for (int u = 0; u < D; ++u) issue_b(u);
    vm_wait<D - 1>();  // halo 0 and B(0) in; B(1..D-1) may fly
  } else {
    vm_wait<0>();
  }
  dma_barrier();

  const int l15 = lane & 15, kc = lane >> 4;
  // A fragment (row group i, tap (dy, dx)): LDS pixels a0 + dy HW2 + dx +
  // delta(i) + l15. a0 (the wave's first row, tap (0,0)) is uniform; delta(i)
  // is a compile-time pixel step (a wave's rows start an image row or lie in
  // one); the lane's byte offset depends on the phase 1 + dx alone.
  const int r0 = wm * TM2 * 16;
  const int a0 = (r0 / WD + 1) * HW2 + r0 % WD + 1;
  auto lane_off = [&](int ph) { return l15 * 64 + ((kc ^ halo_swz(ph + l15)) << 4); };
  const int ox0 = lane_off(0), ox1 = lane_off(1), ox2 = lane_off(2);
  // byte offset of row group 0 at tap tn (vector: one add and a select per K-tile)
  auto abase = [&](int tn) {
    const int dy = tn / 3 - 1, dx = tn % 3 - 1;
    const int ox = dx < 0 ? ox0 : (dx == 0 ? ox1 : ox2);
    return (a0 + dy * HW2 + dx) * 64 + ox;
  };
  auto rda = [&](const bf16_t* h, int i, int vb) {
    const int delta = ((16 * i) / WD) * HW2 + (16 * i) % WD;
    return __builtin_bit_cast(bf16x8, *(const u32x4*)((const char*)h + vb + delta * 64));
  };
  // B fragment jj: rows n = wn TN2 16 + 16 jj + l15, one phase for all jj
  const int bo = (wn * TN2 * 16 + l15) * 64 + ((kc ^ halo_swz(wn * TN2 * 16 + l15)) << 4);
  auto rdb = [&](const bf16_t* st, int jj) {
    return __builtin_bit_cast(bf16x8, *(const u32x4*)((const char*)st + bo + jj * 1024));
  };

  f32x4 acc4[TM2][TN2];
#pragma unroll
  for (int i = 0; i < TM2; ++i)
#pragma unroll
    for (int jj = 0; jj < TN2; ++jj) acc4[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
  // fragments single-buffered, each refilled right behind its last MFMA of the
  // K-tile (2 waves per SIMD: 128 accumulators + 48 fragment registers)
  bf16x8 fa[TM2], fb[TN2];
#pragma unroll
  for (int jj = 0; jj < TN2; ++jj) fb[jj] = rdb(bs, jj);
#pragma unroll
  for (int i = 0; i < TM2; ++i) fa[i] = rda(hb, i, abase(0));
  int j = 0, t = 0;
  // pieces this wave issued in each of the last D - 1 K-tiles (2-bit fields,
  // newest lowest; the prologue's B(1..D-1) count as K-tiles -(D-1)..-1): at
  // K-tile kt's barrier exactly those, and kt's own, were issued after B(kt+1)
  uint32_t hist = 0;
  if (bmine)
    for (int u = 0; u < D - 1; ++u) hist |= 1u << (2 * u);
  for (int kt = 0; kt < nkt; ++kt) {
    const bool hiss = t < HPW && j + 1 < nch;
    const bool biss = bmine && kt + D < nkt;
    if (hiss) issue_h(t, (j + 1) & 1, 32 * (j + 1));
    if (biss) issue_b(kt + D);
    hist = ((hist << 2) | (uint32_t)((int)hiss + (int)biss)) & ((1u << (2 * (D - 1))) - 1u);
    int jn = j, tn = t + 1;
    if (tn == 9) {
      tn = 0;
      ++jn;
    }
    // first half: rows 0 .. TM2/2-1
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < TM2 / 2; ++i)
#pragma unroll
      for (int jj = 0; jj < TN2; ++jj)
        acc4[i][jj] = mfma_s16_16(fa[i], fb[jj], acc4[i][jj], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    const bool more = kt + 1 < nkt;
    const bf16_t* nb = bs + ((kt + 1) % SB) * BST;
    const bf16_t* nh = hb + (jn & 1) * HBUF;
    const int vb = abase(tn);
    if (more) {
      // this wave's pieces of K-tile kt+1 (and, entering a chunk, its halo)
      // landed: only the pieces issued above may still fly
      const uint32_t fly = (hist & 3u) + ((hist >> 2) & 3u) + ((hist >> 4) & 3u) + ((hist >> 6) & 3u);
      switch (fly) {
        case 0: vm_wait<0>(); break;
        case 1: vm_wait<1>(); break;
        case 2: vm_wait<2>(); break;
        case 3: vm_wait<3>(); break;
        case 4: vm_wait<4>(); break;
        case 5: vm_wait<5>(); break;
        case 6: vm_wait<6>(); break;
        case 7: vm_wait<7>(); break;
        default: vm_wait<8>(); break;
      }
      dma_barrier();
#pragma unroll
      for (int i = 0; i < TM2 / 2; ++i) fa[i] = rda(nh, i, vb);
    }
    // second half: rows TM2/2 .. TM2-1, column-major so each B fragment is
    // free (and refilled) after its last use
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int jj = 0; jj < TN2; ++jj) {
#pragma unroll
      for (int i = TM2 / 2; i < TM2; ++i)
        acc4[i][jj] = mfma_s16_16(fa[i], fb[jj], acc4[i][jj], 0, 0, 0);
      if (more) fb[jj] = rdb(nb, jj);
    }
    __builtin_amdgcn_s_setprio(0);
    if (more) {
#pragma unroll
      for (int i = TM2 / 2; i < TM2; ++i) fa[i] = rda(nh, i, vb);
    }
    j = jn;
    t = tn;
  }
  f32x16 acc[TM2 / 2][TN2 / 2];
  acc16_to_32<TM2 / 2, TN2 / 2>(acc4, acc, lane);
  dma_barrier();  // the epilogue reuses the LDS
  EpiCtx cx{m0, n0, m0 + wm * TM2 * 16, n0 + wn * TN2 * 16, wm, wn, lane, (float*)lds, by, 0};
  EP::template apply<TM2 / 2, TN2 / 2, WM, WN>(ep, acc, cx, M, N, 0);
}

// NSM_BF16_HALO (opt-in, read at every dispatch): 1 = the narrow 3x3 layers
// on the halo kernel, 2 = as 1 with 64-channel N tiles for the 256-wide
// 128-channel layers. Measured slower than the im2col DMA GEMMs on every
// layer of the B=64 step but conv4 (DESIGN.md, round 5), so off by default
static int bf16_halo() { return (int)env_int("NSM_BF16_HALO", 0); }

// NSM_BF16_DMA selects the pipelined kernels: 0 = off (register-staged
// kernels only), 1 = 256x128 forward tiles only, 2 = 256x256 forward tiles
// where Cout % 256 == 0 (default; measured 1142 vs 924 TFLOP/s on conv6)
static int bf16_dma_mode() { static const int v = (int)env_int("NSM_BF16_DMA", 2); return v; }
// NSM_BF16_XCD: bit 0 = XCD-contiguous tile order for the forward/dgrad DMA
// GEMMs, bit 1 = for the weight-gradient DMA GEMMs
// measured: fwd +-0 %, wgrad +0.4 % (r02); both, r04: B=64 step 1226 -> 1232
// frames/s, and the 4 N-tiles of an M block share one XCD's L2 (A fetched once)
static int bf16_xcd() { static const int v = (int)env_int("NSM_BF16_XCD", 3); return v; }
// NSM_BF16_PF: bit 0 = fragment reads one k-step ahead (PF) in the forward /
// dgrad DMA GEMMs, bit 1 = in the weight-gradient DMA GEMMs. Measured (B=64
// bf16 train step, A/B in one box): off 1110-1113 frames/s, fwd+wgrad 1105-1106,
// fwd 1104, wgrad 1110: two waves per SIMD already hide the LDS read latency,
// so it stays off by default
static int bf16_pf() { static const int v = (int)env_int("NSM_BF16_PF", 0); return v; }
// NSM_BF16_DMA_PIPE: K-tile ring of the 256x256 forward / dgrad GEMMs:
// 0 = BK 64 x 2 stages, 1 = BK 32 x 5 stages (all 160 KiB), 2 = BK 32 x 4,
// 3 = BK 64 x 2 with the refill issued before the first LDS read. Measured
// (conv6 fwd GEMM / train step, B=64 bf16): 0 = 1168-1184 TFLOP/s, 1113-1123
// frames/s; 1 = 1059-1061, 1072; 2 = 1052, 1066; 3 = 1134, 1099. A deeper
// ring does not pay: the per-K-tile barrier and the LDS-DMA issue cost (eight
// 1-KiB pieces per wave per K-tile beside 32 MFMAs), not the DMA latency,
// bound this loop
static int bf16_dma_pipe() { static const int v = (int)env_int("NSM_BF16_DMA_PIPE", 0); return v; }
// NSM_BF16_ILV: refill pieces placed between the MFMAs of each k-step
// (REFILL 2) instead of behind its fragment reads: bit 0 forward / dgrad,
// bit 1 weight gradient. Measured (B=64 bf16 train step, A/B in one box):
// off 1101-1109 frames/s, both 1062-1076, forward only 1099, weight gradient
// only 1081: off by default
static int bf16_ilv() { static const int v = (int)env_int("NSM_BF16_ILV", 0); return v; }
// NSM_BF16_XT=0: the 2-stage forward / dgrad DMA GEMMs on the per-tile
// barrier loop instead of the cross-tile pipeline (REFILL 3). Measured (B=64
// bf16, A/B in one box): conv6 fwd GEMM 1200 -> 1226 TFLOP/s, train step
// 1166-1170 -> 1173-1175 frames/s
static bool bf16_xt() { static const bool v = env_flag("NSM_BF16_XT", true); return v; }
// NSM_BF16_XT_WG: the 2-stage weight-gradient DMA GEMMs on the cross-tile
// pipeline. Measured (B=64 bf16, A/B in one box): 1181-1185 off vs 1176-1184
// frames/s on (conv8/conv9 -1 %, conv6/conv7 +1 %): off by default
static bool bf16_xt_wg() { static const bool v = env_flag("NSM_BF16_XT_WG", false); return v; }
// NSM_BF16_KORDER=0: tap-major K walk for the DMA 3x3 convolutions
static bool bf16_korder() { static const bool v = env_flag("NSM_BF16_KORDER", true); return v; }
// NSM_BF16_MF16=1: the 2-stage forward / dgrad DMA GEMMs on
// v_mfma_f32_16x16x32_bf16 (REFILL 4) instead of 32x32x16 (REFILL 3);
// =2: only the 256x256 tiles with K >= 4096 (conv6 / conv7 3x3)
// measured: 0 1193-1201, 2 1202-1205 frames/s (B=64 step)
static int bf16_mf16() { static const int v = (int)env_int("NSM_BF16_MF16", 2); return v; }
template <int BM, int BN, int WM, int WN, int STAGES, int BK, int REFILL, class EP = EpiStoreB>
static int launch_conv_fwd_dma_v(const ConvActPB& ap, const RowsKPB& bp, const typename EP::P& ep,
                                 int M, int N, int K, hipStream_t s) {
  constexpr int NW = WM * WN;
  using AL = ConvActDma<BM, NW, BK>;
  using BL = RowsKDma<BN, NW, BK>;
  dim3 grid(ceil_div(N, BN), ceil_div(M, BM), 1);
  const int remap = (bf16_xcd() & 1) && (grid.x * grid.y) % 8 == 0;
  bool pf = false;
  if constexpr (std::is_same<EP, EpiStoreB>::value) pf = bf16_pf() & 1;
  if (pf)
    hipLaunchKernelGGL((gemm_bf16_dma_kernel<BM, BN, WM, WN, STAGES, BK, REFILL, true, AL, BL, EP>),
                       grid, dim3(NW * 64), 0, s, ap, bp, ep, M, N, K, K, remap);
  else
    hipLaunchKernelGGL((gemm_bf16_dma_kernel<BM, BN, WM, WN, STAGES, BK, REFILL, false, AL, BL, EP>),
                       grid, dim3(NW * 64), 0, s, ap, bp, ep, M, N, K, K, remap);
  NSM_LAUNCH_CHECK("conv_fwd_bf16_dma");
  return 0;
}

// Measured alternatives (conv6-class launches, B=64): refill issued before
// the first LDS read (EARLY) -2 %; BK = 32 K-tiles with twice the stages -5 %;
// both -7 %. The defaults: BK = 64, refill spread over the 4 k-steps.
template <int BM, int BN, int WM, int WN, int STAGES, class EP = EpiStoreB>
static int launch_conv_fwd_dma(const ConvActPB& ap, const RowsKPB& bp, const typename EP::P& ep,
                               int M, int N, int K, hipStream_t s) {
  constexpr bool STD = std::is_same<EP, EpiStoreB>::value;  // the A/B knobs: store epilogue only
  if constexpr (STAGES == 2) {
    if constexpr (STD) {
      const int mf = bf16_mf16();
      if (mf == 1 || (mf == 2 && BM == 256 && BN == 256 && K >= 4096))
        return launch_conv_fwd_dma_v<BM, BN, WM, WN, STAGES, DBK, 4>(ap, bp, ep, M, N, K, s);
    }
    if (bf16_xt())
      return launch_conv_fwd_dma_v<BM, BN, WM, WN, STAGES, DBK, 3, EP>(ap, bp, ep, M, N, K, s);
  }
  if constexpr (STD)
    if (bf16_ilv() & 1) return launch_conv_fwd_dma_v<BM, BN, WM, WN, STAGES, DBK, 2>(ap, bp, ep, M, N, K, s);
  return launch_conv_fwd_dma_v<BM, BN, WM, WN, STAGES, DBK, 0, EP>(ap, bp, ep, M, N, K, s);
}

// the shapes conv3x3_halo_kernel takes: whole 512-pixel row groups of one
// image, 32-channel chunks, one 64 / 128-wide N tile, >= one block per CU
static bool halo_fits(const ConvActPB& ap, const RowsKPB& bp, int M, int N) {
  if (!bf16_halo() || ap.ksize != 3 || ap.cin % 32 != 0) return false;
  if (ap.W != 64 && ap.W != 128 && ap.W != 256) return false;
  if (ap.H % (512 / ap.W) != 0 || M % 512 != 0) return false;
  if (N != 64 && N != 128) return false;
  if (bp.ldw != 9 * ap.cin || bp.nrows < N) return false;
  return (long long)(M / 512) >= 256;
}

template <int WD, int BN, class EP>
static int launch_conv3x3_halo(const ConvActPB& ap, const RowsKPB& bp, const typename EP::P& ep,
                               int M, int N, hipStream_t s) {
  const HaloPB hp{ap.x, bp.w, ap.ld, ap.cin, ap.H, ap.W, bp.ldw, bp.nrows};
  dim3 grid(M / 512, N / BN, 1);
  const int remap = (bf16_xcd() & 1) && (grid.x * grid.y) % 8 == 0;
  // a 3-stage B ring (5 stages, where the LDS holds them, measured slower:
  // conv9 forward 675 -> 712 us, conv3 185 -> 196 us)
  constexpr int SB = 3;
  hipLaunchKernelGGL((conv3x3_halo_kernel<WD, BN, SB, EP>), grid, dim3(512), 0, s, hp, ep, M, N, remap);
  NSM_LAUNCH_CHECK("conv3x3_halo");
  return 0;
}

template <class EP>
static int dispatch_conv3x3_halo(const ConvActPB& ap, const RowsKPB& bp, const typename EP::P& ep,
                                 int M, int N, hipStream_t s) {
  if (N == 128) {
    if (ap.W == 256)
      return bf16_halo() == 2 ? launch_conv3x3_halo<256, 64, EP>(ap, bp, ep, M, N, s)
                              : launch_conv3x3_halo<256, 128, EP>(ap, bp, ep, M, N, s);
    if (ap.W == 128) return launch_conv3x3_halo<128, 128, EP>(ap, bp, ep, M, N, s);
    return launch_conv3x3_halo<64, 128, EP>(ap, bp, ep, M, N, s);
  }
  if (ap.W == 256) return launch_conv3x3_halo<256, 64, EP>(ap, bp, ep, M, N, s);
  if (ap.W == 128) return launch_conv3x3_halo<128, 64, EP>(ap, bp, ep, M, N, s);
  return launch_conv3x3_halo<64, 64, EP>(ap, bp, ep, M, N, s);
}

template <int BM, int BN, int WM, int WN, int STAGES, int BK, int REFILL>
static int launch_wgrad_dma_v(const PixRowsPB& ap, const PixRowsPB& bp, const EpiSlabP& ep, int M,
                              int N, int K, int kchunk, int splits, hipStream_t s) {
  constexpr int NW = WM * WN;
  using AL = PixRowsDma<BM, NW, false, BK>;
  using BL = PixRowsDma<BN, NW, true, BK>;
  dim3 grid(ceil_div(N, BN), ceil_div(M, BM), splits);
  const int remap = (bf16_xcd() & 2) && (grid.x * grid.y * grid.z) % 8 == 0;
  if (bf16_pf() & 2)
    hipLaunchKernelGGL((gemm_bf16_dma_kernel<BM, BN, WM, WN, STAGES, BK, REFILL, true, AL, BL, EpiSlab>),
                       grid, dim3(NW * 64), 0, s, ap, bp, ep, M, N, K, kchunk, remap);
  else
    hipLaunchKernelGGL((gemm_bf16_dma_kernel<BM, BN, WM, WN, STAGES, BK, REFILL, false, AL, BL, EpiSlab>),
                       grid, dim3(NW * 64), 0, s, ap, bp, ep, M, N, K, kchunk, remap);
  NSM_LAUNCH_CHECK("conv_wgrad_bf16_dma");
  return 0;
}

template <int BM, int BN, int WM, int WN, int STAGES>
static int launch_wgrad_dma(const PixRowsPB& ap, const PixRowsPB& bp, const EpiSlabP& ep, int M,
                            int N, int K, int kchunk, int splits, hipStream_t s) {
  if constexpr (STAGES == 2)
    if (bf16_xt_wg())
      return launch_wgrad_dma_v<BM, BN, WM, WN, STAGES, DBK, 3>(ap, bp, ep, M, N, K, kchunk, splits, s);
  if (bf16_ilv() & 2)
    return launch_wgrad_dma_v<BM, BN, WM, WN, STAGES, DBK, 2>(ap, bp, ep, M, N, K, kchunk, splits, s);
  return launch_wgrad_dma_v<BM, BN, WM, WN, STAGES, DBK, 0>(ap, bp, ep, M, N, K, kchunk, splits, s);
}
