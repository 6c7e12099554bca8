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
  return gemm_h2d<EpiBnBwd>(h2d_tile(M, cip, K, true), ap, bp, ep, M, cip, K, H2Scale{amax_dy2, 1.f},
                            H2Scale{amax_w, 1.f}, as_stream(stream));
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
