// fp32 GEMMs on the f16 matrix cores: two-term fp16 split of power-of-two
// scaled operands (f16x2). Included at the top of nsm_conv.hip only, after
// nsm_conv_split.inc (shares its LDS layouts).
//
// Each fp32 operand tensor X gets one power-of-two scale s = 2^(15 - e),
// e = ceil(log2 max|X|), from the absolute maximum its producer recorded
// (nsm_absmax / a producer's fused atomic max), so |x*s| <= 2^15 < 65504.
// x*s is exact (power of two), and is written as h + l with h = f16(x*s),
// l = f16(x*s - h) (round to nearest even; the residual is exact in fp32).
// Two fp16 terms hold 22 significand bits: |x*s - h - l| <= 2^-22 |x*s|
// while |x*s| >= 2^-2 (l normal); below that the error is at most 2^-25 in
// scaled units = 2^-40 of the tensor maximum. The product
//   (x*s)(y*t) = xh*yh + (xh*yl + xl*yh) + O(2^-22)
// keeps three terms; every f16 x f16 product is exact in fp32 and
// v_mfma_f32_32x32x16_f16 accumulates in fp32, and the epilogue multiplies
// the accumulators by 1/(s*t) (exact). Error, measured (numpy, DESIGN.md):
// rms / max over unit-normal K = 1024 GEMMs 2.6e-7 / 1.8e-6 of the output
// rms, against 4.1e-7 / 4.1e-6 for the fp32 MFMA and 3.5e-7 / 3.8e-6 for the
// bf16 three-way split: half the matrix-core products of the bf16 split
// (3 f16 MFMAs instead of 6 bf16 ones) and two LDS planes instead of three.
// Non-finite operands: max|X| = Inf/NaN gives s = 1, and h = Inf makes the
// residual NaN, so the outputs they touch are NaN (as under the bf16 split).

namespace nsm {

// where a GEMM's operands keep their absolute maxima (slots of NSM_AMAX_WORDS)
struct AmaxPair {
  const uint32_t* a;
  const uint32_t* b;
  __host__ __device__ bool on() const { return a && b; }
};
// pow2_scale_exp, exp2i, pack_h2, unpack_h2, split4h: nsm_common.h (shared with
// the elementwise TU, whose bn_act / bn_bwd_apply write h2 tensors)

// two f16 planes in the layout of SplitImg (16-bit elements, same swizzles)
template <bool KM, int R>
struct SplitImgH {
  using L = SplitImg<KM, R>;
  static constexpr int PLANE = L::PLANE;
  static constexpr int ELEMS = 2 * PLANE;
  __device__ static void put(bf16_t* S, int r, int k, f32x4 v, float s) {
    u32x2 h, l;
    split4h(v, s, h, l);
    const int o = KM ? k * L::KMS + r : L::mk(r, k);
    *(u32x2*)&S[o] = h;
    *(u32x2*)&S[PLANE + o] = l;
  }
  __device__ static f16x8 frag(const bf16_t* S, int p, int rb, int lane, int s) {
    return __builtin_bit_cast(f16x8, L::frag(S, p, rb, lane, s));
  }
};

template <class L, int R>
__device__ __forceinline__ void split_store_h(const L& ld, bf16_t* S, const f32x4* r, float s) {
  using I = SplitImgH<L::KM, R>;
  if constexpr (!L::KM) {
#pragma unroll
    for (int i = 0; i < L::NPT; ++i) I::put(S, ld.row0 + i * L::RSTEP, ld.kc, r[i], s);
  } else {
#pragma unroll
    for (int i = 0; i < L::NPT; ++i) I::put(S, ld.c4o, ld.krow0 + i * L::KSTEP, r[i], s);
  }
}

template <int TM, int TN>
__device__ __forceinline__ void mfma_split_h(f32x16 (&acc)[TM][TN], const f16x8 (&fa)[2][TM],
                                             const f16x8 (&fb)[2][TN]) {
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      f32x16 c = acc[tm][tn];
      c = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[1][tm], fb[0][tn], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][tm], fb[1][tn], c, 0, 0, 0);
      acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][tm], fb[0][tn], c, 0, 0, 0);
    }
}

// gemm_f32s_kernel's structure (one LDS stage, two blocks per CU) with the
// f16x2 split. amax.a / amax.b: bits of max|A| / max|B| (device).
template <int BM, int BN, int WM, int WN, class AL, class BL, class EP, class AP, class BP>
__global__ void __launch_bounds__(WM * WN * 64) __attribute__((amdgpu_waves_per_eu(1, 2)))
    gemm_f32h_kernel(AP ap, BP bp, typename EP::P ep, int M, int N, int K, int kchunk, int zsplit,
                     int remap, AmaxPair amax) {
  constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);
  using IA = SplitImgH<AL::KM, BM>;
  using IB = SplitImgH<BL::KM, BN>;
  constexpr int A_SZ = IA::ELEMS, STAGE = IA::ELEMS + IB::ELEMS;
  constexpr int EPI = WM * WN * (TM * 32) * (TN * 32 + 4) * 2;  // in 16-bit elements
  constexpr int LDS_ELEMS = STAGE > EPI ? STAGE : EPI;
  __shared__ __attribute__((aligned(16))) bf16_t lds[LDS_ELEMS];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (remap) xcd_block_order(bx, by, bz, remap);
  const int m0 = bx * BM, n0 = by * BN;
  const int split = bz % zsplit, batch = bz / zsplit;
  const int kbeg = split * kchunk;
  const int kend = min(K, kbeg + kchunk);
  const int nk = (kend - kbeg + BK - 1) / BK;
  const int ea = pow2_scale_exp(amax_read(amax.a)), eb = pow2_scale_exp(amax_read(amax.b));
  const float sa = exp2i(ea), sb = exp2i(eb);

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

  f32x4 ar[AL::NPT], br[BL::NPT];
  if (nk > 0) {
    a.load(ap, ar);
    b.load(bp, br);
    split_store_h<AL, BM>(a, lds, ar, sa);
    split_store_h<BL, BN>(b, lds + A_SZ, br, sb);
  }
  const int arb = wm * TM * 32, brb = wn * TN * 32;
  a.advance(ap);
  b.advance(bp);
  a.load(ap, ar);
  b.load(bp, br);
  __syncthreads();
  for (int it = 0; it < nk; ++it) {
    f16x8 fa[2][2][TM], fb[2][2][TN];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) fa[s][p][tm] = IA::frag(lds, p, arb + tm * 32, lane, s);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) fb[s][p][tn] = IB::frag(lds + A_SZ, p, brb + tn * 32, lane, s);
      }
    __syncthreads();
    split_store_h<AL, BM>(a, lds, ar, sa);
    split_store_h<BL, BN>(b, lds + A_SZ, br, sb);
    a.advance(ap);
    b.advance(bp);
    a.load(ap, ar);
    b.load(bp, br);
    mfma_split_h<TM, TN>(acc, fa[0], fb[0]);
    mfma_split_h<TM, TN>(acc, fa[1], fb[1]);
    __syncthreads();
  }
  // undo the scales (powers of two: exact; two steps so no factor underflows)
  const float ia = exp2i(-ea), ib = exp2i(-eb);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (acc[i][j] * ia) * ib;

  EpiCtx cx{m0, n0, m0 + arb, n0 + brb, wm, wn, lane, (float*)lds, bx, bz};
  EP::template apply<TM, TN, WM, WN>(ep, acc, cx, M, N, split);
}

// ---- pre-split (h2) operands: H2Scale, h2_exp, h2_store4 (nsm_common.h) ----
// h2 words of two consecutive channels held by lanes (2i, 2i+1): the even lane
// stores the pair's h terms, the odd lane the pair's l terms, one 4-B store
// each (the wave's 64 lanes cover 256 contiguous bytes)
__device__ __forceinline__ uint32_t h2_pair_word(float v, float s) {
  const float a = v * s;
  const _Float16 h = (_Float16)a;
  const _Float16 l = (_Float16)(a - (float)h);
  const uint32_t mine = (uint32_t)__builtin_bit_cast(unsigned short, h) |
                        ((uint32_t)__builtin_bit_cast(unsigned short, l) << 16);
  const uint32_t other = (uint32_t)__shfl_xor((int)mine, 1);
  return (threadIdx.x & 1) ? ((other >> 16) | (mine & 0xffff0000u))
                           : ((mine & 0xffffu) | (other << 16));
}
// f16 offset of that word in an h2 row: channel c (this lane's), pair-aligned
__device__ __forceinline__ int h2_pair_off(int c) {
  const int c0 = c & ~1;
  return 16 * (c0 >> 3) + (c0 & 7) + ((c & 1) ? 8 : 0);
}

}  // namespace nsm
