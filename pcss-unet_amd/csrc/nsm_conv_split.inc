// fp32 GEMMs on the bf16 matrix cores: exact three-way split (bf16x6).
// gemm_f32s_kernel, templated on the fp32 kernel's loaders and epilogues.
// Included at the top of nsm_conv.hip only (after nsm_conv.h), which
// instantiates and launches it (launch_f32_gemm).
//
// Each fp32 operand x is written as x = h + m + l with h = bf16(x),
// m = bf16(x - h), l = bf16(x - h - m) (round to nearest even). The splits
// are exact: an fp32 significand has 24 bits, each bf16 takes 8, and the
// residuals x - h, x - h - m are exact in fp32. The product
//   a*b = ah*bh + (ah*bm + am*bh) + (ah*bl + al*bh + am*bm) + O(2^-24 |a*b|)
// keeps the six terms down to 2^-16 relative; the dropped ones (am*bl, al*bm,
// al*bl) are below fp32's unit roundoff. Every bf16*bf16 product is exact in
// fp32 and v_mfma_f32_32x32x16_bf16 accumulates in fp32, so the GEMM carries
// fp32 accuracy (tests/test_gpu_split.py: max error against an fp64 GEMM
// within that of the fp32 MFMA path; numpy study in DESIGN.md) at 6 bf16
// MFMAs (6 x 32 cycles per 32x32x16) where v_mfma_f32_32x32x2_f32 takes 8 x 64
// cycles for the same 16-deep K: 2.67x fewer MFMA cycles.
//
// The loaders are the fp32 kernel's (global fp32 -> registers); the split
// happens on the way to LDS, so the HBM bytes are the fp32 GEMM's. LDS holds
// per stage and operand three bf16 planes of a BK = 32 slab (2 K-steps of 16):
//   MK [plane][rows][32]: 16-B chunks XOR-swizzled by (row >> 2) & 3, so the
//       16-lane groups of a ds_read_b128 fragment read cover all 64 banks;
//   KM [plane][32][KMS]: the bf16 weight-gradient image (KMStride), read
//       with ds_read_b64_tr_b16 (read_frag_b<true>).

// bf16x8, BKB, LDKB, KMStride, read_frag_b, xcd_block_order: nsm_conv.h
namespace nsm {

__device__ __forceinline__ void split4(f32x4 v, u32x2& h, u32x2& m, u32x2& l) {
  h = u32x2{pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)};
  v -= f32x4{bf_lo(h.x), bf_hi(h.x), bf_lo(h.y), bf_hi(h.y)};
  m = u32x2{pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)};
  v -= f32x4{bf_lo(m.x), bf_hi(m.x), bf_lo(m.y), bf_hi(m.y)};
  l = u32x2{pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)};
}

template <bool KM, int R>
struct SplitImg {
  static constexpr int KMS = KMStride<R>::value;
  static constexpr int PLANE = KM ? BK * KMS : R * BK;  // bf16 elements per plane
  static constexpr int ELEMS = 3 * PLANE;
  // MK: element (row r, k) of a plane
  __device__ static int mk(int r, int k) { return r * BK + ((((k >> 3) ^ (r >> 2)) & 3) << 3) + (k & 7); }
  // 4 consecutive k (MK) or 4 consecutive rows (KM, at K-row k) of one row / column
  __device__ static void put(bf16_t* S, int r, int k, f32x4 v) {
    u32x2 h, m, l;
    split4(v, h, m, l);
    const int o = KM ? k * KMS + r : mk(r, k);
    *(u32x2*)&S[o] = h;
    *(u32x2*)&S[PLANE + o] = m;
    *(u32x2*)&S[2 * PLANE + o] = l;
  }
  // fragment of plane p, K-step s (0, 1), rows rb..rb+31 (the bf16 operand map)
  __device__ static bf16x8 frag(const bf16_t* S, int p, int rb, int lane, int s) {
    if constexpr (!KM) {
      const int r = rb + (lane & 31), h = lane >> 5;
      return __builtin_bit_cast(bf16x8, *(const u32x4*)&S[p * PLANE + mk(r, 16 * s + 8 * h)]);
    } else {
      return read_frag_b<true, R>(S + p * PLANE, rb, lane, s);
    }
  }
};

// registers of an fp32 loader -> the split LDS image
template <class L, int R>
__device__ __forceinline__ void split_store(const L& ld, bf16_t* S, const f32x4* r) {
  using I = SplitImg<L::KM, R>;
  if constexpr (!L::KM) {
#pragma unroll
    for (int i = 0; i < L::NPT; ++i) I::put(S, ld.row0 + i * L::RSTEP, ld.kc, r[i]);
  } else {
#pragma unroll
    for (int i = 0; i < L::NPT; ++i) I::put(S, ld.c4o, ld.krow0 + i * L::KSTEP, r[i]);
  }
}

// MFMAs of one 16-deep K-step on the split fragments (smallest terms first)
template <int TM, int TN>
__device__ __forceinline__ void mfma_split(f32x16 (&acc)[TM][TN], const bf16x8 (&fa)[3][TM],
                                           const bf16x8 (&fb)[3][TN]) {
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      f32x16 c = acc[tm][tn];
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][tm], fb[1][tn], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[2][tm], fb[0][tn], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][tm], fb[2][tn], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][tm], fb[0][tn], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][tm], fb[1][tn], c, 0, 0, 0);
      acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][tm], fb[0][tn], c, 0, 0, 0);
    }
}

// The fp32 GEMM (gemm_f32_kernel's grid, loaders and epilogues) with the
// split products. One LDS stage (48 KB at 128x128): each wave takes the
// slab's fragments into registers, a barrier releases the stage, and the next
// slab's split and LDS writes, the global loads of the one after, and this
// slab's MFMAs are one basic block the scheduler interleaves; two blocks per
// CU, so the loads have a whole slab of both blocks to land. (Two LDS stages,
// 96 KB, hold one block per CU: the same GEMMs ran 1.3-1.5x longer.)
template <int BM, int BN, int WM, int WN, class AL, class BL, class EP, class AP, class BP>
__global__ void __launch_bounds__(WM * WN * 64) __attribute__((amdgpu_waves_per_eu(1, 2)))
    gemm_f32s_kernel(AP ap, BP bp, typename EP::P ep, int M, int N, int K, int kchunk, int zsplit,
                     int remap) {
  constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);
  using IA = SplitImg<AL::KM, BM>;
  using IB = SplitImg<BL::KM, BN>;
  constexpr int A_SZ = IA::ELEMS, STAGE = IA::ELEMS + IB::ELEMS;
  // the store epilogue stages each wave's TM*32 x (TN*32 + 4) floats in LDS
  constexpr int EPI = WM * WN * (TM * 32) * (TN * 32 + 4) * 2;  // in bf16 elements
  constexpr int LDS_ELEMS = STAGE > EPI ? STAGE : EPI;
  __shared__ __attribute__((aligned(16))) bf16_t lds[LDS_ELEMS];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  // XCD-aware order for batched / split-K grids: blocks are dealt round-robin
  // over the 8 XCDs, so dispatch slot L runs on XCD L % 8; give each XCD a
  // contiguous range of logical blocks (whole batch entries / K-splits), so
  // the blocks sharing an operand tile share that XCD's L2
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (remap) xcd_block_order(bx, by, bz, remap);
  const int m0 = bx * BM, n0 = by * BN;
  const int split = bz % zsplit, batch = bz / zsplit;
  const int kbeg = split * kchunk;
  const int kend = min(K, kbeg + kchunk);
  const int nk = (kend - kbeg + BK - 1) / BK;

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
    split_store<AL, BM>(a, lds, ar);
    split_store<BL, BN>(b, lds + A_SZ, br);
  }
  const int arb = wm * TM * 32, brb = wn * TN * 32;
  a.advance(ap);
  b.advance(bp);
  a.load(ap, ar);  // slab 1 (past the end: zero-fill / unused)
  b.load(bp, br);
  __syncthreads();
  for (int it = 0; it < nk; ++it) {
    bf16x8 fa[2][3][TM], fb[2][3][TN];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) fa[s][p][tm] = IA::frag(lds, p, arb + tm * 32, lane, s);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) fb[s][p][tn] = IB::frag(lds + A_SZ, p, brb + tn * 32, lane, s);
      }
    __syncthreads();  // the stage is free
    split_store<AL, BM>(a, lds, ar);
    split_store<BL, BN>(b, lds + A_SZ, br);
    a.advance(ap);
    b.advance(bp);
    a.load(ap, ar);
    b.load(bp, br);
    mfma_split<TM, TN>(acc, fa[0], fb[0]);
    mfma_split<TM, TN>(acc, fa[1], fb[1]);
    __syncthreads();  // slab it + 1 is in LDS
  }

  EpiCtx cx{m0, n0, m0 + arb, n0 + brb, wm, wn, lane, (float*)lds, bx, bz};
  EP::template apply<TM, TN, WM, WN>(ep, acc, cx, M, N, split);
}

}  // namespace nsm
