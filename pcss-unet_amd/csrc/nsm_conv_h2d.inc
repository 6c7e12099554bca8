// The 1x1 convolutions of the DoubleConv (Unetmodel.py:26) on PRE-SPLIT f16x2
// operands (h2 tensors, nsm_conv_h2.inc). Included at the top of
// nsm_conv_h2.hip only, after nsm_conv_h2.inc.
//
// gemm_f32h_kernel (nsm_conv_split16.inc) runs the fp32 1x1 convolutions with
// the f16x2 split done in its operand loaders: every block that loads an
// element splits it again (3 VALU + two LDS writes per 4 elements beside the
// MFMAs), and the loader registers keep the tile at 128 x 128 (21 % of the
// B=8 fp32 step, profiles/r03). Here the operands' PRODUCERS write the two
// fp16 terms (same bytes as fp32):
//   A1  = lrelu(BN1(Y1)) * mask   nsm_bn_act_h2, scale from the bound its BN
//                                 finalize recorded (nsm_bn_finalize_train:
//                                 |gamma| sqrt(n-1) + |beta|, times the mask's
//                                 maximum — train-mode BN of n values)
//   dY2 (the output BN's backward) nsm_bn_bwd_apply_h2, scale from the bound
//                                 nsm_bn_bwd_finalize derives: max|k1 dz|
//                                 (recorded by the BN-backward reduction) +
//                                 |k2| sqrt(n-1)/invstd + |k3| (Samuelson)
//   W2 packed fwd / dgrad         the step's weight preparation (prep kind 5)
// and the forward, the input gradient (with the first BN's backward in its
// epilogue, EpiBnBwd) and the weight gradient run on the LDS-DMA f16 GEMMs of
// nsm_conv_h2.inc: no VALU, no ds_write, no loader registers in the K loop.

// fp32 store epilogue of the h2 GEMMs: bias, one 32-row slab of the wave tile
// at a time through LDS (EpiH2's staging: the whole 128 x 64 wave tile of a
// 256 x 256 block would not fit beside the stages), 16-B stores, then the BN
// batch-statistics partials of the block's rows (EpiStore::stats_only, from
// the accumulators).
struct EpiStoreH {
  using P = EpiStoreP;
  template <int TM, int TN, int WM, int WN>
  static constexpr int lds_bytes() {
    constexpr int a = WM * WN * 32 * (TN * 32 + 4) * 4, b = WM * WN * TN * 32 * 4;
    return a > b ? a : b;
  }
  template <int TM, int TN, int WM, int WN>
  __device__ static void apply(const P& e, f32x16 (&acc)[TM][TN], const EpiCtx& cx, int M, int N,
                               int) {
    const int col = cx.lane & 31, h = cx.lane >> 5;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int n = cx.nb + tn * 32 + col;
      const float bv = (e.bias && n < N) ? e.bias[n] : 0.f;
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[tm][tn][i] += bv;
    }
    constexpr int WC = TN * 32, WCP = WC + 4, CPR = WC / 4;
    float* reg = cx.lds + (cx.wm * WN + cx.wn) * (32 * WCP);
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
        if (m < M && n < N)
          *(f32x4*)(e.y + (size_t)m * e.ldy + n) = *(const f32x4*)&reg[r * WCP + cc * 4];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (!e.stats) return;
    __syncthreads();  // stats_only reuses the LDS
    EpiStore::stats_only<TM, TN, WM, WN>(e, acc, cx, M, N);
  }
};

// Block tiles of the 1x1 h2 GEMMs (M = pixels, N = output channels of the
// GEMM). NSM_H2D_TILE forces one: 1 = 256x256, 2 = 256x128, 3 = 128x128,
// 4 = 256x64, 5 = 128x64, 6 = 128x32 (falling back to the next that divides N).
static int h2d_tile_env() { static const int v = (int)env_int("NSM_H2D_TILE", 0); return v; }
// bnbwd: EpiBnBwd stages the whole wave tile in LDS, which a 256x256 block's
// 128x64 wave tiles do not fit; with a short K (<= 256 channels) its epilogue
// (the Y1 read) dominates, so it takes the 128x128 tile that runs two blocks
// per CU (69.6 KB of LDS) instead of 256x128 at one
// NSM_H2D_BNB_K: the longest K (f16 columns) for which the BN-backward GEMM
// takes the two-blocks-per-CU 128x128 tile
static int h2d_bnb_k() { static const int v = (int)env_int("NSM_H2D_BNB_K", 512); return v; }
static int h2d_tile(long long M, int N, int K, bool bnbwd) {
  int t = h2d_tile_env();
  const long long mb = ceil_div(M, 256);
  if (!t) {
    if (bnbwd && N % 128 == 0 && K <= h2d_bnb_k()) t = 3;
    else if (!bnbwd && N % 256 == 0 && mb * (N / 256) >= 256) t = 1;
    else if (N % 128 == 0 && mb * (N / 128) >= 256) t = 2;
    else if (N % 128 == 0) t = 3;
    else if (N % 64 == 0 && mb * (N / 64) >= 512) t = 4;
    else if (N % 64 == 0) t = 5;
    else t = 6;
  }
  if (t == 1 && (bnbwd || N % 256)) t = 2;
  if ((t == 2 || t == 3) && N % 128) t = 4;
  if ((t == 4 || t == 5) && N % 64) t = 6;
  return t;
}
static int h2d_tile_bm(int t) { return t == 1 || t == 2 || t == 4 ? 256 : 128; }

// NSM_H2D_NFAST=0: the 1x1 GEMMs' blocks in launch order (M fastest) instead
// of N-fastest in XCD-contiguous runs (xcd_block_order mode 2): with several N
// tiles (conv5 / conv6 / conv7: 2-8) the blocks sharing one M tile's A rows run
// back to back on one XCD, so A comes from HBM once instead of once per N tile
// (conv6's input gradient: 8 x 67 MB of dY2 re-read)
static bool h2d_nfast() { static const bool v = env_flag("NSM_H2D_NFAST", true); return v; }

template <int BM, int BN, int WM, int WN, class EP>
static int launch_h2d(const H2RowsP& ap, const H2RowsP& bp, const typename EP::P& ep, int M, int N,
                      int K, H2Scale sa, H2Scale sb, hipStream_t s) {
  constexpr int NW = WM * WN;
  const dim3 grid(ceil_div(M, BM), ceil_div(N, BN), 1);
  const long long total = (long long)grid.x * grid.y;
  const int remap = h2d_nfast() && grid.y > 1 && total % 8 == 0 ? 2 : 0;
  hipLaunchKernelGGL((gemm_h2_kernel<BM, BN, WM, WN, H2RowsDma<BM, NW>, H2RowsDma<BN, NW>, EP>), grid,
                     dim3(NW * 64), 0, s, ap, bp, ep, M, N, K, K, 1, remap, sa, sb);
  NSM_LAUNCH_CHECK("conv1x1_h2");
  return 0;
}

// C[m][n] = sum_k A[m][k] B[n][k] over h2 rows (K = 2 x channels f16 columns)
template <class EP>
static int gemm_h2d(int tile, const H2RowsP& ap, const H2RowsP& bp, const typename EP::P& ep, int M,
                    int N, int K, H2Scale sa, H2Scale sb, hipStream_t s) {
  switch (tile) {
    case 1:
      if constexpr (!std::is_same<EP, EpiBnBwd>::value)
        return launch_h2d<256, 256, 2, 4, EP>(ap, bp, ep, M, N, K, sa, sb, s);
      return fail(NSM_E_ARG, "conv1x1_h2: tile");
    case 2: return launch_h2d<256, 128, 4, 2, EP>(ap, bp, ep, M, N, K, sa, sb, s);
    case 3: return launch_h2d<128, 128, 2, 2, EP>(ap, bp, ep, M, N, K, sa, sb, s);
    case 4: return launch_h2d<256, 64, 4, 1, EP>(ap, bp, ep, M, N, K, sa, sb, s);
    case 5: return launch_h2d<128, 64, 2, 2, EP>(ap, bp, ep, M, N, K, sa, sb, s);
    default: return launch_h2d<128, 32, 4, 1, EP>(ap, bp, ep, M, N, K, sa, sb, s);
  }
}

// weight-gradient plan of a 1x1 conv on h2 operands: M = cout_p, N = cin_p,
// K = pixels split into ~512 blocks (one round of two blocks per CU), every
// split >= 256 pixels, the partial slabs <= 128 MB (plan_wgrad's policy)
static WgradPlan plan_wgrad_h2(long long px, int cin_p, int cout_p) {
  WgradPlan pl;
  pl.BM = cout_p >= 128 ? 128 : (cout_p >= 64 ? 64 : 32);
  pl.BN = cin_p >= 128 ? 128 : (cin_p >= 64 ? 64 : 32);
  const long long tiles = (long long)ceil_div(cout_p, pl.BM) * ceil_div(cin_p, pl.BN);
  static const long long target = env_int("NSM_H2D_WG_BLOCKS", 512);
  long long sp = target / tiles;
  const long long maxs = (px + 255) / 256;
  long long slab_cap = (128ll << 20) / ((long long)cout_p * cin_p);
  if (slab_cap < 1) slab_cap = 1;
  if (sp > maxs) sp = maxs;
  if (sp > slab_cap) sp = slab_cap;
  if (sp > 512) sp = 512;
  if (sp < 1) sp = 1;
  long long kc = (px + sp - 1) / sp;
  kc = (kc + 31) / 32 * 32;  // whole K-tiles of the KM loader
  sp = (px + kc - 1) / kc;
  pl.splits = (int)sp;
  pl.kchunk = (int)kc;
  pl.ws_floats = (size_t)sp * cout_p * cin_p;
  if (sp > 16) pl.ws_floats += (size_t)((sp + 15) / 16) * cout_p * cin_p;
  return pl;
}

// ---- persistent form of the BN-backward input-gradient GEMM ---------------------
// gemm_h2_kernel runs one output tile per block. With the short K of most 1x1
// input gradients (2-4 K-tiles) every block pays descriptor setup, the Y1
// prefetch, two K-tiles of DMA latency and a barrier before a handful of
// MFMAs, then stages its whole wave tile through the LDS the stages used.
// gemm_h2bp_kernel is gemm_h2p_kernel's scheme for this GEMM: a fixed grid
// walks the tiles L = blockIdx.x, + gridDim.x, ... in the order of
// h2d_tile_decode, the K-tile stream runs on ACROSS tiles (the last two
// K-tiles of a tile refill their stages with the next tile's first two, the
// loaders re-aimed), the next tile's first fragments load under the last
// MFMAs, and the epilogue works from a staging region of its own, one 16-row
// slab of the 64 x 64 wave tile at a time, so the next tile's DMA lands while
// it runs. The Y1 rows of the NEXT tile are fetched slab by slab into the
// registers the current slab has just consumed. MFMA shape, product order,
// K order, epilogue arithmetic, per-lane row order, merge order and the
// partial-row format are gemm_h2_kernel<..., EpiBnBwd>'s: the results are
// bitwise those of the one-tile-per-block kernel at the same tile.
//
// The tile walk: logical index lg -> M block lg / gy, N block lg % gy (the N
// tiles of one M block share its dY2 rows and its partial row, so they are
// consecutive); with several N tiles and total % 8 == 0 the dispatch slot L
// maps to lg XCD-contiguously (xcd_block_order mode 2, what launch_h2d uses).
__host__ __device__ inline int h2d_tile_decode(int L, int gx, int gy, int& m, int& n) {
  const int total = gx * gy;
  const int lg = (gy > 1 && (total & 7) == 0) ? (L & 7) * (total >> 3) + (L >> 3) : L;
  m = lg / gy;
  n = lg - m * gy;
  return lg;
}

// two waves per SIMD (two 4-wave blocks or one 8-wave block per CU): 256 registers
template <int BM, int BN, int WM, int WN>
__global__ void __launch_bounds__(WM * WN * 64) __attribute__((amdgpu_waves_per_eu(2, 2)))
    gemm_h2bp_kernel(H2RowsP ap, H2RowsP bp, BnBwdEpiP ep, int M, int N, int K, int gx, int gy,
                     H2Scale sca, H2Scale scb) {
  constexpr int NW = WM * WN, TM = BM / (WM * 32), TN = BN / (WN * 32);
  static_assert(TM == 2 && TN == 2, "64 x 64 wave tiles");
  using AL = H2RowsDma<BM, NW>;
  using BL = H2RowsDma<BN, NW>;
  constexpr int KT = 64;
  constexpr int A_EL = BM * KT, STAGE = (BM + BN) * KT;
  constexpr int LPT = AL::NI + BL::NI;
  constexpr int CPR = 16, NIT = 16;  // EpiBnBwd's lane layout of a 64 x 64 wave tile
  constexpr int SLAB = 16 * 64;      // fp32 staging per wave: 16 rows of the wave tile
  static_assert(LPT <= 63 && 2 * NIT <= 63, "vmcnt range");
  __shared__ __attribute__((aligned(1024))) bf16_t lds[2 * STAGE + 2 * NW * SLAB];

  const int total = gx * gy;
  int L = blockIdx.x;
  if (L >= total) return;  // no tile: out before the first barrier
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int nk = K / KT;  // >= 2 (h2d_bnb_covered)
  const float ia = exp2i(-h2_exp(sca)), ib = exp2i(-h2_exp(scb));
  int bm, bn;
  h2d_tile_decode(L, gx, gy, bm, bn);

  const int arb = wm * TM * 32, brb = wn * TN * 32;
  const int cc = lane % CPR, rq = lane / CPR;
  const float* __restrict__ Y = (const float*)ep.y;
  // Y1 rows of the first tile (EpiBnBwd::prefetch's layout), older than every DMA
  f32x4 yv[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int m = min(bm * BM + arb + it * 4 + rq, M - 1);
    yv[it] = *(const f32x4*)(Y + (size_t)m * ep.ldy + bn * BN + brb + cc * 4);
  }

  AL a;
  BL b;
  a.rows(ap, wid, lane);
  b.rows(bp, wid, lane);
  a.aim(ap, bm * BM, 0);
  b.aim(bp, bn * BN, 0);
  a.prep(ap, 0);
  b.prep(bp, 0);
#pragma unroll
  for (int j = 0; j < LPT; ++j) dma_one(a, b, ap, bp, lds, A_EL, wid, j);
  a.prep(ap, KT);
  b.prep(bp, KT);
#pragma unroll
  for (int j = 0; j < LPT; ++j) dma_one(a, b, ap, bp, lds + STAGE, A_EL, wid, j);
  vm_wait<0>();  // both K-tiles (and Y1): the first tile's K-tile-1 wait then counts like every tile's
  dma_barrier();

  using FR = FragH2<false, KT>;
  FR fa[2][2][TM];  // [k-step][plane][tm]
  FR fb[2][2][TN];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) fa[0][p][tm].issue(lds, arb + tm * 32, lane, 0, p);
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) fb[0][p][tn].issue(lds + A_EL, brb + tn * 32, lane, 0, p);
  }
  const __amdgpu_buffer_rsrc_t orsrc =
      __builtin_amdgcn_make_buffer_rsrc(ep.out, (short)0, ep.out ? M * ep.ldo * 4 : 0, 0x00020000);
  float* const stg = (float*)(lds + 2 * STAGE) + wid * SLAB;
  const float* const stg0 = (const float*)(lds + 2 * STAGE);
  const bool red = ep.mode != 2;
  int st = 0;  // the stage of the K-tile at hand (an odd K-tile count flips it per tile)
  for (; L < total; L += (int)gridDim.x) {
    const bool has_next = L + (int)gridDim.x < total;
    int bmn = 0, bnn = 0;
    if (has_next) h2d_tile_decode(L + (int)gridDim.x, gx, gy, bmn, bnn);
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    for (int t = 0; t < nk; ++t) {
      const bf16_t* As = lds + st * STAGE;
      const bf16_t* Bs = As + A_EL;
      // k-step 0: k-step 1's fragments go out, then k-step 0's MFMAs
#pragma unroll
      for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) fa[1][p][tm].issue(As, arb + tm * 32, lane, 1, p);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) fb[1][p][tn].issue(Bs, brb + tn * 32, lane, 1, p);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) mfma_h2<TM, TN>(acc, fa[0], fb[0], tm, tn);
      __builtin_amdgcn_s_setprio(0);
      const int tgt = t + 2;  // the K-tile refilled into this stage (>= nk: the next tile's)
      const bool more = t + 1 < nk || has_next, refill = tgt < nk || has_next;
      if (refill) {
        if (tgt < nk) {
          a.prep(ap, tgt * KT);
          b.prep(bp, tgt * KT);
        } else {
          if (tgt == nk) {
            a.aim(ap, bmn * BM, 0);
            b.aim(bp, bnn * BN, 0);
          }
          a.prep(ap, (tgt - nk) * KT);
          b.prep(bp, (tgt - nk) * KT);
        }
      }
      __builtin_amdgcn_s_waitcnt(0xC07F);  // this wave's reads of the stage retired
      if (more) {
        // this wave's pieces of the next K-tile. In a tile's first K-tile the
        // previous tile's epilogue is younger than them: NIT Y1 loads, and NIT
        // stores unless mode 0 (anything else it issued only makes the wait
        // stricter). The first tile's K-tile 1 was waited for in the prologue.
        // (t made opaque: a visible t == 0 test makes hipcc peel the first K-trip)
        int tq = t;
        asm volatile("" : "+s"(tq));
        if (tq == 0) {
          if (ep.mode == 0) vm_wait<NIT>();
          else vm_wait<2 * NIT>();
        } else {
          vm_wait<0>();
        }
        __builtin_amdgcn_s_barrier();  // everyone's reads retired, pieces landed
        const bf16_t* Ns = lds + (st ^ 1) * STAGE;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
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
          mfma_h2<TM, TN>(acc, fa[1], fb[1], tm, tn);
          if (refill) {
            const int q = tm * TN + tn;
#pragma unroll
            for (int i = 0; i < LPT; ++i)
              if (i * (TM * TN) / LPT == q) dma_one(a, b, ap, bp, As, A_EL, wid, i);
          }
        }
      __builtin_amdgcn_s_setprio(0);
      st ^= 1;
    }

    // ---- EpiBnBwd::apply_impl on 16-row slabs (same arithmetic, same order) ----
    // lane offsets from an opaque copy of the lane index: formed here, not
    // hoisted into registers that stay live across the K loop
    int el = lane;
    asm volatile("" : "+v"(el));
    const int col = el & 31, h = el >> 5;
    const int ec = el % CPR, er = el / CPR;
    const int mb = bm * BM + arb, n = bn * BN + brb + ec * 4;
    const int mbn = bmn * BM + arb, nn = bnn * BN + brb + ec * 4;
    const float* __restrict__ mk = ep.mask;
    const f32x4 sc = *(const f32x4*)(ep.scale + n), sh = *(const f32x4*)(ep.shift + n),
                mu = *(const f32x4*)(ep.mean + n);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 is = red ? *(const f32x4*)(ep.invstd + n) : zero;
    const f32x4 k1 = red ? zero : *(const f32x4*)(ep.coef + n),
                k2 = red ? zero : *(const f32x4*)(ep.coef + N + n),
                k3 = red ? zero : *(const f32x4*)(ep.coef + 2 * N + n);
    // the Dropout2d mask rows of the wave tile's 64 pixels: with HW >= 64 they
    // lie in at most two images, whose rows are fetched here with the column
    // vectors (a load per pixel row would drain the whole memory stream, the
    // next tile's DMA and Y1 included, 16 times per tile); shorter images
    // keep the load per row
    const bool mrow = mk && ep.fdHW.d < 64u;
    f32x4 mk0 = zero, mk1 = zero;
    int mth = 0;
    if (mk && !mrow) {
      const uint32_t b0 = fdiv((uint32_t)min(mb, M - 1), ep.fdHW),
                     b1 = fdiv((uint32_t)min(mb + 63, M - 1), ep.fdHW);
      mk0 = *(const f32x4*)(mk + (size_t)b0 * N + n);
      mk1 = *(const f32x4*)(mk + (size_t)b1 * N + n);
      mth = (int)((b0 + 1u) * ep.fdHW.d);
    }
    // Every load of the epilogue but the next tile's Y1 is complete before the
    // first slab: a register the compiler believes a load may still be writing
    // on some path would cost a vmcnt(0) wherever the K loop reuses it, once
    // per K-tile, and that wait would drain the DMA stream.
    asm volatile("" ::"v"(sc), "v"(sh), "v"(mu), "v"(is), "v"(k1), "v"(k2), "v"(k3), "v"(mk0), "v"(mk1));
    f32x4 s1 = zero, s2 = zero;
    uint32_t am = 0;
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) {
      const int tm = sl >> 1, hf = sl & 1;
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          stg[((j & 3) + 8 * (j >> 2) + 4 * h) * 64 + tn * 32 + col] = (acc[tm][tn][8 * hf + j] * ia) * ib;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int it = sl * 4 + q;
        const int m = mb + it * 4 + er;
        const bool ok = m < M;
        const uint32_t ooff = ok ? (uint32_t)(m * ep.ldo + n) * 4u : OOB;
        const f32x4 g = *(const f32x4*)&stg[(q * 4 + er) * 64 + ec * 4], v = yv[it];
        f32x4 dz = g * lrelu_grad_v4(v * sc + sh, ep.slope);
        if (mrow) dz = dz * *(const f32x4*)(mk + (size_t)fdiv((uint32_t)min(m, M - 1), ep.fdHW) * N + n);
        else if (mk) dz = dz * (m < mth ? mk0 : mk1);
        // rows past M by select, not by branch: every loaded register is
        // consumed on every path (see the note at the column vectors)
        if (!red) {
          const f32x4 d = k1 * dz + k2 * (v - mu) + k3;
          uint32_t a2 = am;
          amax_fold(a2, d);
          am = ok ? a2 : am;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, d), orsrc, ooff, 0, 0);
        } else {
          const f32x4 t1 = s1 + dz, t2 = s2 + dz * ((v - mu) * is);
          s1 = ok ? t1 : s1;
          s2 = ok ? t2 : s2;
          if (ep.k1dz) {
            uint32_t a2 = am;
            amax_fold(a2, sc * dz);
            am = ok ? a2 : am;
          }
          if (ep.mode == 1)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, g), orsrc, ooff, 0, 0);
        }
      }
      // the next tile's Y1 rows into the registers this slab has consumed
      if (has_next) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int it = sl * 4 + q;
          const int m = min(mbn + it * 4 + er, M - 1);
          yv[it] = *(const f32x4*)(Y + (size_t)m * ep.ldy + nn);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // the maxima go to a line chosen by the tile, not by the block that ran it
    uint32_t* const aslot = red ? ep.k1dz : ep.amax;
    if (aslot) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o));
      const uint32_t line = ((uint32_t)bm + 7u * (uint32_t)bn) & (AMAX_LINES - 1);
      if (el == 0 && am) atomicMax(aslot + line * AMAX_STRIDE, am);
    }
    if (red) {
#pragma unroll
      for (int o = CPR; o < 64; o <<= 1) {
        s1 += shfl_xor_v4(s1, o);
        s2 += shfl_xor_v4(s2, o);
      }
      // one partial row per BM rows: every wave leaves its sums in its own
      // staging rows, the waves of one column range meet after a barrier,
      // fixed order. The rows are next written in the next tile's epilogue,
      // past a K-tile barrier that the reading waves reach after reading.
      if (el < CPR) {
        *(f32x4*)(stg + ec * 4) = s1;
        *(f32x4*)(stg + 64 + ec * 4) = s2;
      }
      dma_barrier();
      if (wm == 0) {
        float* pr = ep.partial + (size_t)bm * 2 * N;
        for (int j = el; j < 2 * 64; j += 64) {
          const int k = j / 64, c = j - k * 64;
          float t = 0.f;
#pragma unroll
          for (int w = 0; w < WM; ++w) t += stg0[(w * WN + wn) * SLAB + k * 64 + c];
          pr[k * N + bn * BN + brb + c] = t;
        }
      }
    }
    bm = bmn;
    bn = bnn;
  }
}

// NSM_H2D_BNB_PERSIST: 0 = the one-tile-per-block kernel everywhere, 1 (default)
// = the policy below, 2 = the persistent form wherever it covers the shape.
// nsm_set_h2d_bnb_persist overrides (form 0 = policy, 1 = old, 2 = persistent;
// grid = blocks of the persistent form, 0 = as many as are resident at once).
static int g_h2d_bnb_form = [] {
  const long long v = env_int("NSM_H2D_BNB_PERSIST", 1);
  return v == 0 ? 1 : v == 2 ? 2 : 0;
}();
static int g_h2d_bnb_grid = 0;

// shapes the persistent form takes: the 128-column tiles of 64 x 64 wave tiles,
// whole N tiles, at least two K-tiles (a single K-tile, conv9's K = 64, would
// need the DMA stream to run two TILES ahead: it stays on the old kernel),
// 32-bit byte offsets into the output
static bool h2d_bnb_covered(int tile, long long M, int N, int K, int ldo) {
  return (tile == 2 || tile == 3) && N % 128 == 0 && K % 64 == 0 && K >= 128 &&
         M * (long long)std::max(ldo, N) * 4 < (1ll << 31) &&
         ceil_div(M, h2d_tile_bm(tile)) * (N / 128) < (1ll << 30);
}
// policy: more tiles than one round of resident blocks (two per CU of the
// 128-row tile, one of the 256-row tile); otherwise every block has one tile
// and the walk buys nothing
static bool h2d_bnb_persistent(int tile, long long M, int N, int K, int ldo) {
  if (g_h2d_bnb_form == 1 || !h2d_bnb_covered(tile, M, N, K, ldo)) return false;
  if (g_h2d_bnb_form == 2) return true;
  const long long tiles = ceil_div(M, h2d_tile_bm(tile)) * (N / 128);
  return tiles > (long long)cu_count() * (tile == 3 ? 2 : 1);
}

template <int BM, int BN, int WM, int WN>
static int h2bp_grid(long long total) {
  static const int resident = [] {
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, gemm_h2bp_kernel<BM, BN, WM, WN>,
                                                     WM * WN * 64, 0) != hipSuccess || occ < 1)
      occ = 1;
    return std::min(occ, 2) * cu_count();
  }();
  const long long g = g_h2d_bnb_grid > 0 ? g_h2d_bnb_grid : resident;
  return (int)std::min<long long>(g, total);
}

template <int BM, int BN, int WM, int WN>
static int launch_h2bp(const H2RowsP& ap, const H2RowsP& bp, const BnBwdEpiP& ep, int M, int N, int K,
                       H2Scale sa, H2Scale sb, hipStream_t s) {
  const int gx = ceil_div(M, BM), gy = N / BN;
  const int grid = h2bp_grid<BM, BN, WM, WN>((long long)gx * gy);
  hipLaunchKernelGGL((gemm_h2bp_kernel<BM, BN, WM, WN>), dim3(grid), dim3(WM * WN * 64), 0, s, ap, bp,
                     ep, M, N, K, gx, gy, sa, sb);
  NSM_LAUNCH_CHECK("conv1x1_h2 (persistent)");
  return 0;
}

extern "C" int nsm_conv1x1_h2_rows(int M, int N, int K, int bnbwd) {
  return h2d_tile_bm(h2d_tile(M, N, K, bnbwd != 0));
}

extern "C" int nsm_conv1x1_h2(const void* xh, int M, int cin_p, const void* wh, const float* bias,
                              int cout_p, float* y, int ldy, float* stats, const uint32_t* amax_x,
                              const uint32_t* amax_w, void* stream) {
  NSM_CHECK_ARG(xh && wh && y && amax_x && amax_w, "conv1x1_h2: null pointer");
  NSM_CHECK_ARG(M > 0 && cin_p % 32 == 0 && cout_p % 32 == 0 && ldy >= cout_p && ldy % 4 == 0,
                "conv1x1_h2: bad shape");
  NSM_CHECK_ARG(((uintptr_t)xh % 16) == 0 && ((uintptr_t)wh % 16) == 0 && ((uintptr_t)y % 16) == 0,
                "conv1x1_h2: 16-B alignment");
  NSM_CHECK_ARG((long long)M * 2 * cin_p < (1ll << 30), "conv1x1_h2: operand too large");
  const int K = 2 * cin_p;
  H2RowsP ap{(const bf16_t*)xh, K, M, 0};
  H2RowsP bp{(const bf16_t*)wh, K, cout_p, 0};
  EpiStoreP ep{y, ldy, bias, stats, 0, nullptr, nullptr, 0.f, nullptr, 0, 1};
  return gemm_h2d<EpiStoreH>(h2d_tile(M, cout_p, K, false), ap, bp, ep, M, cout_p, K,
                             H2Scale{amax_x, 1.f}, H2Scale{amax_w, 1.f}, as_stream(stream));
}

// nsm_conv1x1_dgrad_bnbwd on h2 operands (dY2 rows, the DGRAD-packed h2
// weight [cip][2 cop]); partial rows: one per block of nsm_conv1x1_h2_rows(M,
// cip, 2 cop, 1) pixels
extern "C" int nsm_conv1x1_dgrad_bnbwd_h2(const void* dy2h, int M, int cop, const void* w2dh,
                                          int cip, const float* y1, int ldy1, const float* scale,
                                          const float* shift, const float* mean,
                                          const float* invstd, const float* mask, int HW,
                                          float slope, int mode, float* partial, const float* coef,
                                          float* out, int ldo, const uint32_t* amax_dy2,
                                          const uint32_t* amax_w, uint32_t* amax_out,
                                          uint32_t* amax_k1dz, void* stream) {
  NSM_CHECK_ARG(dy2h && w2dh && y1 && scale && shift && mean && amax_dy2 && amax_w,
                "conv1x1_dgrad_bnbwd_h2: null pointer");
  NSM_CHECK_ARG(mode >= 0 && mode <= 2, "conv1x1_dgrad_bnbwd_h2: mode %d", mode);
  NSM_CHECK_ARG(mode == 2 || (partial && invstd), "conv1x1_dgrad_bnbwd_h2: modes 0/1 need partials");
  NSM_CHECK_ARG(mode == 0 || out, "conv1x1_dgrad_bnbwd_h2: modes 1/2 need an output");
  NSM_CHECK_ARG(mode != 2 || coef, "conv1x1_dgrad_bnbwd_h2: mode 2 needs coef");
  NSM_CHECK_ARG(M > 0 && HW > 0 && cop % 32 == 0 && cip % 32 == 0 && ldy1 >= cip && ldy1 % 4 == 0 &&
                    (mode == 0 || (ldo >= cip && ldo % 4 == 0)),
                "conv1x1_dgrad_bnbwd_h2: bad shape");
  NSM_CHECK_ARG(((uintptr_t)dy2h % 16) == 0 && ((uintptr_t)w2dh % 16) == 0 &&
                    ((uintptr_t)y1 % 16) == 0 && ((uintptr_t)out % 16) == 0,
                "conv1x1_dgrad_bnbwd_h2: 16-B alignment");
  NSM_CHECK_ARG((long long)M * 2 * cop < (1ll << 30), "conv1x1_dgrad_bnbwd_h2: operand too large");
  BnBwdEpiP ep{out, ldo, y1, ldy1, scale, shift, mean, invstd, coef, mask,
               make_fastdiv((uint32_t)HW), slope, partial, mode};
  if (mode == 2) ep.amax = amax_out;
  else ep.k1dz = amax_k1dz;
  const int K = 2 * cop;
  H2RowsP ap{(const bf16_t*)dy2h, K, M, 0};
  H2RowsP bp{(const bf16_t*)w2dh, K, cip, 0};
  const int tile = h2d_tile(M, cip, K, true);
  if (h2d_bnb_persistent(tile, M, cip, K, mode == 0 ? cip : ldo)) {
    if (tile == 2)
      return launch_h2bp<256, 128, 4, 2>(ap, bp, ep, M, cip, K, H2Scale{amax_dy2, 1.f},
                                         H2Scale{amax_w, 1.f}, as_stream(stream));
    return launch_h2bp<128, 128, 2, 2>(ap, bp, ep, M, cip, K, H2Scale{amax_dy2, 1.f},
                                       H2Scale{amax_w, 1.f}, as_stream(stream));
  }
  return gemm_h2d<EpiBnBwd>(tile, ap, bp, ep, M, cip, K, H2Scale{amax_dy2, 1.f},
                            H2Scale{amax_w, 1.f}, as_stream(stream));
}

// the kernel form of nsm_conv1x1_dgrad_bnbwd_h2: form 0 = policy, 1 = one tile
// per block, 2 = persistent wherever covered, < 0 = unchanged; grid = blocks
// of the persistent form (0 = default, < 0 = unchanged). prev (optional)
// receives the previous {form, grid}.
extern "C" int nsm_set_h2d_bnb_persist(int form, int grid, int* prev) {
  NSM_CHECK_ARG(form <= 2, "set_h2d_bnb_persist: form %d", form);
  if (prev) {
    prev[0] = g_h2d_bnb_form;
    prev[1] = g_h2d_bnb_grid;
  }
  if (form >= 0) g_h2d_bnb_form = form;
  if (grid >= 0) g_h2d_bnb_grid = grid;
  return 0;
}

// what nsm_conv1x1_dgrad_bnbwd_h2 launches for (M, cip, cop) with a contiguous
// output: plan[0] = tile (h2d_tile's numbering), plan[1] = form (0 = one tile
// per block, 1 = persistent), plan[2] = blocks of the persistent form (0 for
// form 0), plan[3] = rows per partial row
extern "C" int nsm_conv1x1_dgrad_bnbwd_h2_plan(int M, int cip, int cop, int* plan) {
  NSM_CHECK_ARG(plan && M > 0 && cip > 0 && cop > 0 && cip % 32 == 0 && cop % 32 == 0,
                "conv1x1_dgrad_bnbwd_h2_plan: bad args");
  const int K = 2 * cop, tile = h2d_tile(M, cip, K, true), bm = h2d_tile_bm(tile);
  const bool p = h2d_bnb_persistent(tile, M, cip, K, cip);
  const long long total = (long long)ceil_div(M, bm) * ceil_div(cip, 128);
  plan[0] = tile;
  plan[1] = p ? 1 : 0;
  plan[2] = !p ? 0 : tile == 2 ? h2bp_grid<256, 128, 4, 2>(total) : h2bp_grid<128, 128, 2, 2>(total);
  plan[3] = bm;
  return 0;
}

// the tiles block `block` of a persistent grid of `grid` blocks walks over a
// gx x gy tile space, in order: out[3 i] = M block, [3 i + 1] = N block,
// [3 i + 2] = logical index (h2d_tile_decode). *count = their number (at most
// cap are written). Host only: no device is touched.
extern "C" int nsm_h2d_tile_walk(int gx, int gy, int grid, int block, int* out, int cap,
                                 int* count) {
  NSM_CHECK_ARG(out && count && gx > 0 && gy > 0 && grid > 0 && block >= 0 && block < grid &&
                    cap >= 0 && (long long)gx * gy < (1ll << 30),
                "h2d_tile_walk: bad args");
  int cnt = 0;
  for (int L = block; L < gx * gy; L += grid, ++cnt) {
    if (cnt >= cap) continue;
    int m, n;
    out[3 * cnt + 2] = h2d_tile_decode(L, gx, gy, m, n);
    out[3 * cnt] = m;
    out[3 * cnt + 1] = n;
  }
  *count = cnt;
  return 0;
}

// ---- the fused BN-act 1x1 forward ------------------------------------------------
// nsm_bn_act_h2 writes A1 = lrelu(BN1(Y1)) * mask as an h2 tensor and
// nsm_conv1x1_h2 reads it straight back by LDS-DMA. Where N fits one block
// tile, one block owns whole rows of A1, so gemm_h2a_kernel PRODUCES the A
// stage instead of fetching it: every thread loads 8-channel units of Y1
// (fp32, two 16-B loads), applies bn_act_h2_8 (nsm_elem.h, the arithmetic
// bn_act_h2_kernel calls), stores the h2 words to A1 in global memory (the
// weight gradient reads A1 later) and into the LDS A stage at the place
// H2RowsDma would have put them: one 128-B row per M row and 64-column
// K-tile, 16-B chunk c at (c ^ dswz<64>(row)); rows past M are zero, as the
// DMA's out-of-range reads are. W2 streams into the B stage by LDS-DMA as in
// gemm_h2_kernel. Fragments, mfma_h2's product order, the K order, the
// epilogue (EpiStoreH) and BM are gemm_h2_kernel's, so Y2, the BN2 partials
// and A1 are bitwise what the two kernels give.
//
// Schedule, per tile (a block walks tiles bm = blockIdx.x, + gridDim.x, ...):
//   issue(t):  scale/shift (and mask) vectors, the Y1 units of K-tile t into
//              registers, then W2's DMA pieces into stage t & 1
//   commit(t): vmcnt(0); bn-act + split; ds_write the A stage; A1 stores
//   prologue:  issue(0) commit(0) issue(1) barrier
//   K-tile t:  k-step 0, k-step 1 | commit(t+1) barrier | issue(t+2)
// Every vector-memory wait is a full one and each is meant: at commit(t+1)
// the wave's counter holds, oldest first, the A1 stores of commit(t) and
// issue(t+1)'s loads and DMA; the loads are the youngest and the counter is
// in order, so waiting for them is waiting for all. Nothing else is in
// flight in the K loop (a tile spanning images adds a drained mask load per
// unit, see mrow). The next tile's first loads are younger than the
// epilogue's Y2 stores and wait for them the same way.
//
// Budget per block (LDS: NSTG stages of (BM + BN) x 128 B, reused by
// EpiStoreH; registers: accumulators + one k-step of fragments + NU units
// of 8 fp32 + scale/shift + a mask row, capped at 256 by two waves per SIMD):
//   256 x 128, 8 waves: 96 KB, NU = 2, 188 VGPRs -> one block per CU
//   256 x 64,  4 waves: 80 KB, NU = 4, 207 VGPRs -> two
//              (K = 64: one stage, 40 KB, 155 VGPRs -> three)
//   128 x 128, 4 waves: 64 KB, NU = 2, 192 VGPRs -> two
//   128 x 64,  4 waves: 48 KB, 180 VGPRs -> two (one stage: 24 KB, 143 -> three)
//   128 x 32,  4 waves: 40 KB, NU = 2, 125 VGPRs -> four
// No scratch in any of them (-Rpass-analysis=kernel-resource-usage); each
// spills 8-49 SGPRs, which go to VGPR lanes and are inside the counts above.
struct BnActH2P {
  const float* y;  // Y1 [M][ldy]
  int ldy;
  const float* scale;
  const float* shift;
  float slope;
  const float* mask;  // [B][cin_p] or NULL
  FastDiv fdHW;
  bf16_t* a1;  // [M][2 cin_p]
};

template <int BM, int BN, int WM, int WN, int NSTG>
__global__ void __launch_bounds__(WM * WN * 64) __attribute__((amdgpu_waves_per_eu(2)))
    gemm_h2a_kernel(BnActH2P ap, H2RowsP bp, EpiStoreP ep, int M, int N, int K, int gx, H2Scale sca,
                    H2Scale scb) {
  constexpr int NW = WM * WN, NT = NW * 64, TM = BM / (WM * 32), TN = BN / (WN * 32);
  using BL = H2RowsDma<BN, NW>;
  constexpr int KT = 64;
  constexpr int A_EL = BM * KT, STAGE = (BM + BN) * KT;
  constexpr int NU = BM * 4 / NT, RSTEP = NT / 4;  // 8-channel units per thread and K-tile
  static_assert(NU >= 1 && NU * NT == BM * 4, "unit shape");
  constexpr int EPI = EpiStoreH::template lds_bytes<TM, TN, WM, WN>() / 2;
  constexpr int LDS_EL = NSTG * STAGE > EPI ? NSTG * STAGE : EPI;
  __shared__ __attribute__((aligned(1024))) bf16_t lds[LDS_EL];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int nk = K / KT;  // NSTG == 1: nk == 1
  const int cin = K >> 1;
  const int ea = h2_exp(sca), eb = h2_exp(scb);
  const float s = exp2i(ea);
  // unit i of a thread: row (tid >> 2) + i * RSTEP, channels 8 (tid & 3) .. + 7 of the K-tile
  const bool masked = ap.mask != nullptr;

  BL b;
  b.init(bp, 0, 0, K, wid, lane, 0);
  using FR = FragH2<false, KT>;
  const int arb = wm * TM * 32, brb = wn * TN * 32;

  for (int bm = blockIdx.x; bm < gx; bm += (int)gridDim.x) {
    const int m0 = bm * BM;
    if (bm != (int)blockIdx.x) __syncthreads();  // the previous tile's epilogue is done with the LDS
    // Dropout2d mask rows: a tile inside one image (every tile of the step's
    // shapes: BM divides H W) takes that image's vector per K-tile with the
    // Y1 loads; a tile spanning images (HW % BM != 0) loads one vector per
    // unit when it commits
    const uint32_t b0 = masked ? fdiv((uint32_t)m0, ap.fdHW) : 0u;
    const bool mrow = masked && fdiv((uint32_t)min(m0 + BM - 1, M - 1), ap.fdHW) != b0;

    F8 yv[NU], sc, sh;
    F8 mk0 = f8zero();
    // (unit offsets from an opaque copy of the thread index, formed where they
    // are used: hoisted, they would stay live across the K loop and the tiles)
    auto issue = [&](int t) {
      int tq = tid;
      asm volatile("" : "+v"(tq));
      const int c8 = tq & 3, r0 = tq >> 2;
      const int c = t * 32 + c8 * 8;
      sc = ldf8(ap.scale + c);
      sh = ldf8(ap.shift + c);
      if (masked && !mrow) mk0 = ld8(ap.mask + (size_t)b0 * cin + c);
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        const int m = min(m0 + r0 + i * RSTEP, M - 1);  // rows past M: a valid row, not used
        yv[i] = ld8(ap.y + (size_t)m * ap.ldy + c);
      }
      b.prep(bp, t * KT);
      const bf16_t* Bs = lds + (NSTG > 1 ? (t & 1) * STAGE : 0) + A_EL;
#pragma unroll
      for (int j = 0; j < BL::NI; ++j) b.one(bp, Bs, wid, j);
    };
    auto commit = [&](int t) {
      vm_wait<0>();
      int tq = tid;
      asm volatile("" : "+v"(tq));
      const int c8 = tq & 3, r0 = tq >> 2;
      bf16_t* As = lds + (NSTG > 1 ? (t & 1) * STAGE : 0);
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        const int row = r0 + i * RSTEP, m = m0 + row;
        const bool ok = m < M;
        F8 mk = mk0;
        if (mrow) {
          F8 g = ld8(ap.mask + (size_t)fdiv((uint32_t)min(m, M - 1), ap.fdHW) * cin + t * 32 + c8 * 8);
          // (consumed here: merged with the read of mk0, the load would become
          // a flat load from a selected address and mk0 live in scratch)
          asm volatile("" : "+v"(g.a), "+v"(g.b));
          mk = g;
        }
        u32x4 h, l;
        bn_act_h2_8(yv[i], sc, sh, ap.slope, masked, mk, s, h, l);
        const u32x4 z = {0u, 0u, 0u, 0u};
        h = ok ? h : z;
        l = ok ? l : z;
        const int sw = dswz<KT>(row);
        *(u32x4*)&As[row * KT + (((2 * c8) ^ sw) << 3)] = h;
        *(u32x4*)&As[row * KT + (((2 * c8 + 1) ^ sw) << 3)] = l;
        if (ok) {
          bf16_t* g = ap.a1 + (size_t)m * K + t * KT + c8 * 16;
          *(u32x4*)g = h;
          *(u32x4*)(g + 8) = l;
        }
      }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    issue(0);
    commit(0);
    if (NSTG > 1 && nk > 1) issue(1);
    dma_barrier();

    // one k-step of fragments at a time: the kernel is bound by the Y1 / A1 /
    // Y2 streams, and the registers go to the Y1 units in flight instead
    FR fa[2][TM], fb[2][TN];  // [plane][tm]
    for (int t = 0; t < nk; ++t) {
      const bf16_t* As = lds + (NSTG > 1 ? (t & 1) * STAGE : 0);
      const bf16_t* Bs = As + A_EL;
      int lq = lane;
      asm volatile("" : "+v"(lq));
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
          for (int tm = 0; tm < TM; ++tm) fa[p][tm].issue(As, arb + tm * 32, lq, ks, p);
#pragma unroll
          for (int tn = 0; tn < TN; ++tn) fb[p][tn].issue(Bs, brb + tn * 32, lq, ks, p);
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn) mfma_h2<TM, TN>(acc, fa, fb, tm, tn);
        __builtin_amdgcn_s_setprio(0);
      }
      if constexpr (NSTG > 1) {
        if (t + 1 < nk) {
          // stage (t+1) & 1 was last read in K-tile t-1, before the barrier
          // that ended it; this barrier: everyone's reads of stage t & 1
          // retired (it is refilled next), everyone's part of K-tile t+1 landed
          commit(t + 1);
          dma_barrier();
          if (t + 2 < nk) issue(t + 2);
        }
      }
    }
    dma_barrier();  // the epilogue reuses the LDS
    const float ia = exp2i(-ea), ib = exp2i(-eb);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = (acc[i][j] * ia) * ib;
    int le = lane;  // (opaque: the epilogue's lane offsets are formed here, not kept across the tiles)
    asm volatile("" : "+v"(le));
    EpiCtx cx{m0, 0, m0 + arb, brb, wm, wn, le, (float*)lds, bm, 0};
    EpiStoreH::template apply<TM, TN, WM, WN>(ep, acc, cx, M, N, 0);
  }
}

// NSM_H2D_ACT_FUSE: 0 (default) = the policy below, 1 = nsm_bn_act_h2 +
// nsm_conv1x1_h2 everywhere, 2 = the fused kernel wherever it covers the
// shape. nsm_set_h2d_act_fuse overrides (form 0 = policy, 1 = two kernels, 2 =
// fused; grid = blocks of the fused kernel, 0 = one per tile).
static int g_h2d_act_form = [] {
  const long long v = env_int("NSM_H2D_ACT_FUSE", 0);
  return v == 1 ? 1 : v == 2 ? 2 : 0;
}();
static int g_h2d_act_grid = 0;

// shapes the fused kernel takes: N is exactly one block tile of h2d_tile (one
// block then owns whole rows of A1 and produces each element once), whole
// 64-column K-tiles (cin_p % 32 == 0)
static int h2d_tile_bn(int t) { return t == 1 ? 256 : t == 2 || t == 3 ? 128 : t == 6 ? 32 : 64; }
static bool h2d_act_covered(int tile, long long M, int N, int K) {
  return tile >= 2 && tile <= 6 && h2d_tile_bn(tile) == N && K % 64 == 0 && K >= 64 &&
         M * K < (1ll << 30);
}
// policy: every covered shape (the measurement kept all five of the fp32
// step's, DESIGN.md "The fused BN-act 1x1 forward"; below them a launch less
// is the whole difference)
static bool h2d_act_fused(int tile, long long M, int N, int K) {
  if (g_h2d_act_form == 1 || !h2d_act_covered(tile, M, N, K)) return false;
  return true;
}
static int h2a_grid(int gx) { return g_h2d_act_grid > 0 ? std::min(g_h2d_act_grid, gx) : gx; }

template <int BM, int BN, int WM, int WN>
static int launch_h2a(const BnActH2P& ap, const H2RowsP& bp, const EpiStoreP& ep, int M, int N, int K,
                      H2Scale sa, H2Scale sb, hipStream_t s) {
  const int gx = ceil_div(M, BM), grid = h2a_grid(gx);
  // a single K-tile needs one stage only (a second block per CU fits instead)
  if (K == 64 && BN == 64)
    hipLaunchKernelGGL((gemm_h2a_kernel<BM, BN, WM, WN, (BN == 64 ? 1 : 2)>), dim3(grid),
                       dim3(WM * WN * 64), 0, s, ap, bp, ep, M, N, K, gx, sa, sb);
  else
    hipLaunchKernelGGL((gemm_h2a_kernel<BM, BN, WM, WN, 2>), dim3(grid), dim3(WM * WN * 64), 0, s, ap,
                       bp, ep, M, N, K, gx, sa, sb);
  NSM_LAUNCH_CHECK("bn_act_conv1x1_h2");
  return 0;
}

// A1 [M][2 cin_p] h2 = lrelu(y1 * scale + shift) (* mask[row / HW]) at the
// scale of `bound` (nsm_bn_act_h2) and y2 [M][ldy2] fp32 = A1 W^T + bias with
// the BN partials `stats` (nsm_conv1x1_h2), in one kernel; the shape must be
// one nsm_bn_act_conv1x1_h2_plan covers
extern "C" int nsm_bn_act_conv1x1_h2(const float* y1, int ldy1, int M, int cin_p, const float* scale,
                                     const float* shift, float slope, const float* mask, int HW,
                                     void* a1, const void* wh, const float* bias, int cout_p,
                                     float* y2, int ldy2, float* stats, const uint32_t* bound,
                                     const uint32_t* amax_w, void* stream) {
  NSM_CHECK_ARG(y1 && scale && shift && a1 && wh && y2 && bound && amax_w,
                "bn_act_conv1x1_h2: null pointer");
  NSM_CHECK_ARG(M > 0 && cin_p > 0 && cout_p > 0 && cin_p % 32 == 0 && cout_p % 32 == 0 &&
                    ldy1 >= cin_p && ldy1 % 4 == 0 && ldy2 >= cout_p && ldy2 % 4 == 0 &&
                    (!mask || HW > 0),
                "bn_act_conv1x1_h2: bad shape");
  NSM_CHECK_ARG(((uintptr_t)y1 % 16) == 0 && ((uintptr_t)a1 % 16) == 0 && ((uintptr_t)wh % 16) == 0 &&
                    ((uintptr_t)y2 % 16) == 0 && ((uintptr_t)scale % 16) == 0 &&
                    ((uintptr_t)shift % 16) == 0 && ((uintptr_t)mask % 16) == 0,
                "bn_act_conv1x1_h2: 16-B alignment");
  NSM_CHECK_ARG((long long)M * 2 * cin_p < (1ll << 30), "bn_act_conv1x1_h2: operand too large");
  const int K = 2 * cin_p, tile = h2d_tile(M, cout_p, K, false);
  if (!h2d_act_covered(tile, M, cout_p, K))
    return fail(NSM_E_ARG, "bn_act_conv1x1_h2: shape not covered (cout_p %d, tile %d)", cout_p, tile);
  BnActH2P ap{y1, ldy1, scale, shift, slope, mask, make_fastdiv(mask ? HW : 1), (bf16_t*)a1};
  H2RowsP bp{(const bf16_t*)wh, K, cout_p, 0};
  EpiStoreP ep{y2, ldy2, bias, stats, 0, nullptr, nullptr, 0.f, nullptr, 0, 1};
  const H2Scale sa{bound, 1.f}, sb{amax_w, 1.f};
  hipStream_t s = as_stream(stream);
  switch (tile) {
    case 2: return launch_h2a<256, 128, 4, 2>(ap, bp, ep, M, cout_p, K, sa, sb, s);
    case 3: return launch_h2a<128, 128, 2, 2>(ap, bp, ep, M, cout_p, K, sa, sb, s);
    case 4: return launch_h2a<256, 64, 4, 1>(ap, bp, ep, M, cout_p, K, sa, sb, s);
    case 5: return launch_h2a<128, 64, 2, 2>(ap, bp, ep, M, cout_p, K, sa, sb, s);
    default: return launch_h2a<128, 32, 4, 1>(ap, bp, ep, M, cout_p, K, sa, sb, s);
  }
}

// form 0 = policy, 1 = two kernels, 2 = fused wherever covered, < 0 =
// unchanged; grid = blocks of the fused kernel (0 = one per tile, < 0 =
// unchanged). prev (optional) receives the previous {form, grid}.
extern "C" int nsm_set_h2d_act_fuse(int form, int grid, int* prev) {
  NSM_CHECK_ARG(form <= 2, "set_h2d_act_fuse: form %d", form);
  if (prev) {
    prev[0] = g_h2d_act_form;
    prev[1] = g_h2d_act_grid;
  }
  if (form >= 0) g_h2d_act_form = form;
  if (grid >= 0) g_h2d_act_grid = grid;
  return 0;
}

// what ops.bn_act_conv1x1_h2 runs for (M, cin_p, cout_p): plan[0] = tile
// (h2d_tile's numbering), plan[1] = form (0 = two kernels, 1 = fused), plan[2]
// = blocks of the fused kernel (0 for form 0), plan[3] = rows per partial row
extern "C" int nsm_bn_act_conv1x1_h2_plan(int M, int cin_p, int cout_p, int* plan) {
  NSM_CHECK_ARG(plan && M > 0 && cin_p > 0 && cout_p > 0 && cin_p % 32 == 0 && cout_p % 32 == 0,
                "bn_act_conv1x1_h2_plan: bad args");
  const int K = 2 * cin_p, tile = h2d_tile(M, cout_p, K, false), bm = h2d_tile_bm(tile);
  const bool f = h2d_act_fused(tile, M, cout_p, K);
  plan[0] = tile;
  plan[1] = f ? 1 : 0;
  plan[2] = f ? h2a_grid(ceil_div(M, bm)) : 0;
  plan[3] = bm;
  return 0;
}

extern "C" size_t nsm_conv1x1_wgrad_h2_ws(int M, int cin_p, int cout_p) {
  return plan_wgrad_h2(M, cin_p, cout_p).ws_floats;
}

// dw[co][ci] (reference layout, 1x1) = sum_p dY[p][co] X[p][ci] over h2 pixel
// rows: split-K KM x KM h2 GEMM (wino_wgrad_gemm_h2 with one batch entry),
// fixed-order slab reduction (wgrad_finish)
extern "C" int nsm_conv1x1_wgrad_h2(const void* dyh, const void* xh, int M, int cin_p, int cout_p,
                                    int cin, int cout, float* dw, float* ws, size_t ws_floats,
                                    const uint32_t* amax_dy, const uint32_t* amax_x, void* stream) {
  NSM_CHECK_ARG(dyh && xh && dw && ws && amax_dy && amax_x, "conv1x1_wgrad_h2: null pointer");
  NSM_CHECK_ARG(M > 0 && cin_p % 32 == 0 && cout_p % 32 == 0 && cin <= cin_p && cout <= cout_p,
                "conv1x1_wgrad_h2: bad shape");
  NSM_CHECK_ARG(((uintptr_t)dyh % 16) == 0 && ((uintptr_t)xh % 16) == 0 && ((uintptr_t)ws % 16) == 0,
                "conv1x1_wgrad_h2: 16-B alignment");
  NSM_CHECK_ARG((long long)M * 2 * std::max(cin_p, cout_p) < (1ll << 30),
                "conv1x1_wgrad_h2: operand too large");
  const WgradPlan pl = plan_wgrad_h2(M, cin_p, cout_p);
  if (ws_floats < pl.ws_floats)
    return fail(NSM_E_WS, "conv1x1_wgrad_h2: workspace %zu < %zu floats", ws_floats, pl.ws_floats);
  hipStream_t s = as_stream(stream);
  const int rc = wino_wgrad_gemm_h2((const bf16_t*)dyh, (const bf16_t*)xh, M, cin_p, cout_p, 1,
                                    pl.BM, pl.BN, pl.kchunk, pl.splits, ws, H2Scale{amax_dy, 1.f},
                                    H2Scale{amax_x, 1.f}, s);
  if (rc) return rc;
  return wgrad_finish(ws, pl, cout_p, cin_p, cin_p, 1, cin, cout, dw, s);
}

// ---- the direct 3x3 convolution (conv2, Cin < 64) on h2 operands ---------------
// The bf16 LDS-DMA loaders (nsm_conv_s16_loaders.inc) move 16-bit columns: an h2
// tensor [pixels][2 C] is read by them as a 16-bit tensor of 2 C columns, one
// K-tile of 64 columns = 32 channels x 2 planes, the MK image FragH2 expects.
// These adapters give them gemm_h2_kernel's interface (K-tile size, batch
// argument; KM loaders address K relative to the split start).
template <int R, int NW>
struct H2ConvDma : ConvActDma<R, NW, 64> {
  static constexpr int KT = 64;
  __device__ void init(const ConvActPB& p, int m0, int kb, int ke, int wid, int lane, int) {
    ConvActDma<R, NW, 64>::init(p, m0, kb, ke, wid, lane);
  }
};
template <int R, int NW>
struct H2RowsKDma : RowsKDma<R, NW, 64> {
  static constexpr int KT = 64;
  __device__ void init(const RowsKPB& p, int n0, int kb, int ke, int wid, int lane, int) {
    RowsKDma<R, NW, 64>::init(p, n0, kb, ke, wid, lane);
  }
};
// the shifted (tap) operand of the 3x3 weight gradient, K = pixels, 32-row K-tiles
template <int R, int NW>
struct H2ShiftDma : PixRowsDma<R, NW, true, 32> {
  static constexpr int KT = 32;
  int kb0;
  __device__ void init(const PixRowsPB& p, int off, int kb, int ke, int wid, int lane, int) {
    kb0 = kb;  // off: the tile's first GEMM column (channel units) -> f16 column 2 off
    PixRowsDma<R, NW, true, 32>::init(p, 2 * off, kb, ke, wid, lane);
  }
  __device__ void prep(const PixRowsPB& p, int krel) { PixRowsDma<R, NW, true, 32>::prep(p, kb0 + krel); }
};

static ConvActPB h2_conv_operand(const void* xh, int B, int H, int W, int cin_p) {
  ConvActPB ap{};
  ap.x = (const bf16_t*)xh;
  ap.ld = 2 * cin_p;
  ap.cin = 2 * cin_p;  // 16-bit columns per tap
  ap.H = H;
  ap.W = W;
  ap.M = B * H * W;
  ap.ksize = 3;
  ap.K = 9 * 2 * cin_p;
  ap.fdW = make_fastdiv(W);
  ap.fdH = make_fastdiv(H);
  ap.fdC = make_fastdiv(2 * cin_p);
  ap.cm = 1;  // K-tile t = (64-column chunk j, tap): the 9 taps of a chunk back to back
  return ap;
}

template <int BM, int BN, int WM, int WN>
static int launch_h2c(const ConvActPB& ap, const RowsKPB& bp, const EpiStoreP& ep, int M, int N,
                      int K, H2Scale sa, H2Scale sb, hipStream_t s) {
  constexpr int NW = WM * WN;
  const dim3 grid(ceil_div(M, BM), ceil_div(N, BN), 1);
  hipLaunchKernelGGL((gemm_h2_kernel<BM, BN, WM, WN, H2ConvDma<BM, NW>, H2RowsKDma<BN, NW>, EpiStoreH>),
                     grid, dim3(NW * 64), 0, s, ap, bp, ep, M, N, K, K, 1, 0, sa, sb);
  NSM_LAUNCH_CHECK("conv3x3_h2");
  return 0;
}

extern "C" int nsm_conv3x3_h2_rows(int M, int N) {
  return N % 64 == 0 ? 256 : 128;
}

// y [M][ldy] fp32 = conv3x3(x, W) + bias over h2 operands: xh [B*H*W][2 cin_p]
// (nsm_input_prep_h2, or nsm_bn_bwd_apply_h2's dY for the input gradient), wh
// the prep-kind-5 pack [cout_p][9][2 cin_p] (FWD, or DGRAD for the input
// gradient); stats (may be NULL): BN partials of nsm_conv3x3_h2_rows(M, cout_p) rows
extern "C" int nsm_conv3x3_h2(const void* xh, int B, int H, int W, int cin_p, const void* wh,
                              const float* bias, int cout_p, float* y, int ldy, float* stats,
                              const uint32_t* amax_x, const uint32_t* amax_w, void* stream) {
  NSM_CHECK_ARG(xh && wh && y && amax_x && amax_w, "conv3x3_h2: null pointer");
  NSM_CHECK_ARG(B > 0 && H > 0 && W > 0 && cin_p % 32 == 0 && cout_p % 32 == 0 && ldy >= cout_p &&
                    ldy % 4 == 0,
                "conv3x3_h2: bad shape");
  NSM_CHECK_ARG(((uintptr_t)xh % 16) == 0 && ((uintptr_t)wh % 16) == 0 && ((uintptr_t)y % 16) == 0,
                "conv3x3_h2: 16-B alignment");
  const long long Ml = (long long)B * H * W;
  NSM_CHECK_ARG(Ml * 2 * cin_p < (1ll << 30), "conv3x3_h2: operand too large");
  const int M = (int)Ml, K = 9 * 2 * cin_p;
  const ConvActPB ap = h2_conv_operand(xh, B, H, W, cin_p);
  const RowsKPB bp{(const bf16_t*)wh, K, cout_p, K, 2 * cin_p, 1};
  EpiStoreP ep{y, ldy, bias, stats, 0, nullptr, nullptr, 0.f, nullptr, 0, 1};
  const H2Scale sa{amax_x, 1.f}, sb{amax_w, 1.f};
  hipStream_t s = as_stream(stream);
  if (cout_p % 64 == 0) return launch_h2c<256, 64, 4, 1>(ap, bp, ep, M, cout_p, K, sa, sb, s);
  return launch_h2c<128, 32, 4, 1>(ap, bp, ep, M, cout_p, K, sa, sb, s);
}

// weight-gradient plan of the direct 3x3 on h2 operands: M = cout_p rows, N =
// 9 cin_p columns in 128-column tiles spanning taps (PixRowsDma: one tap per
// lane), K = pixels split into ~512 blocks
static WgradPlan plan_wgrad3_h2(long long px, int cin_p, int cout_p) {
  WgradPlan pl = plan_wgrad_h2(px, 128, cout_p);
  pl.BM = 32;
  pl.BN = 128;
  const long long tiles = (long long)ceil_div(cout_p, 32) * ceil_div(9 * cin_p, 128);
  long long sp = 512 / tiles;
  const long long maxs = (px + 255) / 256;
  if (sp > maxs) sp = maxs;
  if (sp > 512) sp = 512;
  if (sp < 1) sp = 1;
  long long kc = (px + sp - 1) / sp;
  kc = (kc + 31) / 32 * 32;
  sp = (px + kc - 1) / kc;
  pl.splits = (int)sp;
  pl.kchunk = (int)kc;
  const size_t MN = (size_t)cout_p * 9 * cin_p;
  pl.ws_floats = (size_t)sp * MN;
  if (sp > 16) pl.ws_floats += (size_t)((sp + 15) / 16) * MN;
  return pl;
}

extern "C" size_t nsm_conv3x3_wgrad_h2_ws(int B, int H, int W, int cin_p, int cout_p) {
  return plan_wgrad3_h2((long long)B * H * W, cin_p, cout_p).ws_floats;
}

// dw[co][ci][3][3] (reference layout) = sum_p dY[p][co] X[p + tap][ci] over h2
// pixel rows (dyh [M][2 cout_p], xh [M][2 cin_p]); cout_p == 32 (the 32-row
// tile covers the block's 3x3 conv, Cout = Cin < 64)
extern "C" int nsm_conv3x3_wgrad_h2(const void* dyh, const void* xh, int B, int H, int W, int cin_p,
                                    int cout_p, int cin, int cout, float* dw, float* ws,
                                    size_t ws_floats, const uint32_t* amax_dy,
                                    const uint32_t* amax_x, void* stream) {
  NSM_CHECK_ARG(dyh && xh && dw && ws && amax_dy && amax_x, "conv3x3_wgrad_h2: null pointer");
  NSM_CHECK_ARG(cout_p == 32 && cin_p % 32 == 0 && cin <= cin_p && cout <= cout_p,
                "conv3x3_wgrad_h2: cout_p must be 32, cin_p a multiple of 32");
  NSM_CHECK_ARG(((uintptr_t)dyh % 16) == 0 && ((uintptr_t)xh % 16) == 0 && ((uintptr_t)ws % 16) == 0,
                "conv3x3_wgrad_h2: 16-B alignment");
  const long long Ml = (long long)B * H * W;
  NSM_CHECK_ARG(Ml * 2 * cin_p < (1ll << 30) && Ml < (1ll << 30), "conv3x3_wgrad_h2: too large");
  const WgradPlan pl = plan_wgrad3_h2(Ml, cin_p, cout_p);
  if (ws_floats < pl.ws_floats)
    return fail(NSM_E_WS, "conv3x3_wgrad_h2: workspace %zu < %zu floats", ws_floats, pl.ws_floats);
  const int M = cout_p, N = 9 * cin_p, K = (int)Ml;
  H2PixP ap{(const bf16_t*)dyh, 2 * cout_p, 2 * cout_p, K, 0};
  PixRowsPB bp{};
  bp.x = (const bf16_t*)xh;
  bp.ld = 2 * cin_p;
  bp.ncols = 2 * cin_p;
  bp.cin = 2 * cin_p;  // 16-bit columns per tap: the tile's GEMM column -> (tap, column)
  bp.H = H;
  bp.W = W;
  bp.M = K;
  bp.ksize = 3;
  bp.fdW = make_fastdiv(W);
  bp.fdH = make_fastdiv(H);
  EpiH2P ep{ws, N, (long long)M * N};
  const dim3 grid(ceil_div(M, 32), ceil_div(N, 128), pl.splits);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL((gemm_h2_kernel<32, 128, 1, 4, H2PixDma<64, 4>, H2ShiftDma<256, 4>, EpiH2>), grid,
                     dim3(256), 0, s, ap, bp, ep, M, N, K, pl.kchunk, pl.splits, 0,
                     H2Scale{amax_dy, 1.f}, H2Scale{amax_x, 1.f});
  NSM_LAUNCH_CHECK("conv3x3_wgrad_h2");
  return wgrad_finish(ws, pl, M, N, cin_p, 9, cin, cout, dw, s);
}
