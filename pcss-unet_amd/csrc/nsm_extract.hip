// Learned feature extraction (paper §3.2): the "2-layer deep 1x1 convolution
// network" that compresses the composed G-buffer channels to the U-Net's input,
// forward and backward, each one streaming pass (nsm_amd/extract.py; DESIGN.md
// "Learned feature extraction").
//
//   x [B][Cin][H][W] f32 -> y [B][Cout][H][W] f32; w1 [Hd][Cin], b1 [Hd],
//   w2 [Cout][Hd], b2 [Cout]: the memory of nn.Conv2d(.., 1).weight / .bias.
//   1 <= Cin <= 32, 1 <= Hd <= 32, 1 <= Cout <= 16.
//
// Arithmetic, per pixel, every step one IEEE fp32 operation:
//   pre[j] = fmaf(w1[j][Cin-1], x[Cin-1], .. fmaf(w1[j][0], x[0], b1[j]))
//   h[j]   = pre[j] > 0 ? pre[j] : pre[j] * slope
//   y[c]   = fmaf(w2[c][Hd-1], h[Hd-1], .. fmaf(w2[c][0], h[0], b2[c]))
// i.e. each dot product is one fmaf chain that starts from the bias and takes
// its index in ascending order (ex_pre below, the only place it is written:
// the backward recomputes pre with it, so its mask is the forward's). Backward:
//   g[j]   = fmaf(w2[Cout-1][j], dy[Cout-1], .. fmaf(w2[0][j], dy[0], +0))
//   dh[j]  = pre[j] > 0 ? g[j] : g[j] * slope        (torch's choice at pre == 0)
//   dx[i]  = fmaf(w1[Hd-1][i], dh[Hd-1], .. fmaf(w1[0][i], dh[0], +0))
//   dw1[j][i] = sum dh[j] x[i], db1[j] = sum dh[j], dw2[c][j] = sum dy[c] h[j],
//   db2[c] = sum dy[c] over all B H W pixels, in the fixed order given below.
//   The four parameter gradients are written, not accumulated into.
//
// Work. A unit is 4 consecutive columns of one row (unit u: image u / (H Q), row
// (u % (H Q)) / Q, columns 4 (u % Q) .. + 3, Q = ceil(W / 4)); a thread owns a unit
// and produces all its channels, the hidden vector in registers. 16-byte
// accesses where the four columns exist and the address is 16-byte aligned,
// decided per access on the real address, 4-byte ones otherwise. The weights
// are staged in LDS once per block, in their own layouts, and read from there
// at a wave-uniform address; the hidden units are taken one at a time, a row of
// w1 serving pre[j] and, in the backward, the dx chains.
//
// Backward reduction. No atomics. A tile is EX_TILE units (one per thread of a
// 2-wave block); the grid is min(tiles, EX_MAX_GRID) blocks and block k takes
// the tiles k, k + grid, k + 2 grid, ..: a set fixed by the shape. For each of
// its 4 pixel slots e a wave stages, per-wave in LDS as [pixel][channel], first
// dy and h | 1, then dh and x | 1 (one region, used twice), and folds the 64
// pixels into its accumulators with the exact-fp32 MFMA, K = pixels:
//   [dw2 | db2] += dy^T (h | 1),   [dw1 | db1] += dh^T (x | 1)
// (v_mfma_f32_16x16x4_f32; the constant-1 column yields the bias gradients). A
// pixel outside the image carries x = 0 and dy = 0, hence dh = 0: it adds +0.
// Rows and columns of a 16-wide MFMA tile beyond the real channel counts hold
// whatever the region held before; an MFMA output depends on its own row of A
// and column of B only, and those outputs are never read. At the end wave 1's
// accumulators are added to wave 0's through LDS (wave 0 + wave 1) and the
// block writes its partial [P], P = Hd Cin + Hd + Cout Hd + Cout laid out
// dw1 | db1 | dw2 | db2, to ws[block][P]. extract_merge_kernel then sums the
// `grid` partials of each entry: EX_SLICES threads take contiguous runs of
// blocks in index order, and the runs are added in slice order. The result is a
// pure function of the arguments: the same bits on every run, stream and replay.
#include "nsm_common.h"

#pragma clang fp contract(off)

namespace nsm {

constexpr int EX_MAX_IN = 32, EX_MAX_HID = 32, EX_MAX_OUT = 16;
constexpr int EX_FWD_THREADS = 256;
constexpr int EX_BWD_THREADS = 128;  // 2 waves: the staging region of a block stays below 48 KiB
constexpr int EX_TILE = EX_BWD_THREADS;  // units of a tile
// blocks of the backward grid: 4 per CU of the 256; a block's registers allow 4 per CU
constexpr int EX_MAX_GRID = 1024;
constexpr int EX_SLICES = 16, EX_MERGE_COLS = 64;

struct ExtractArgs {
  const float *x, *dy, *w1, *b1, *w2, *b2;
  float *y, *dx, *ws;
  int Cin, Hd, Cout, H, W;
  uint32_t units;
  int tiles, grid;
  float slope;
  FastDiv q, hq;  // units of a row, of an image
};

__host__ __device__ constexpr int ex_r16(int n) { return (n + 15) & ~15; }
__host__ __device__ constexpr int ex_max(int a, int b) { return a > b ? a : b; }
inline int ex_params(int Cin, int Hd, int Cout) { return Hd * Cin + Hd + Cout * Hd + Cout; }
// floats of one staged pixel: rows of 16 k + 1 floats (an odd stride: the
// per-lane row writes and the MFMA operand reads both spread over the banks)
__host__ __device__ constexpr int ex_stage(int Cin, int Hd) {
  return ex_max(17 + ex_r16(Hd + 1) + 1, ex_r16(Hd) + 1 + ex_r16(Cin + 1) + 1);
}

__device__ __forceinline__ float ex_fma(float w, float x, float a) { return fmaf(w, x, a); }
__device__ __forceinline__ f32x4 ex_fma(float w, f32x4 x, f32x4 a) {
  return f32x4{fmaf(w, x.x, a.x), fmaf(w, x.y, a.y), fmaf(w, x.z, a.z), fmaf(w, x.w, a.w)};
}
__device__ __forceinline__ float ex_splat(float v, float) { return v; }
__device__ __forceinline__ f32x4 ex_splat(float v, f32x4) { return f32x4{v, v, v, v}; }

// w1, b1, w2, b2 into LDS in their own layouts; the caller synchronises
__device__ __forceinline__ void ex_stage_weights(const ExtractArgs& a, int Cin, int Hd, int Cout,
                                                 float* s, int threads) {
  float *s_w1 = s, *s_b1 = s_w1 + Hd * Cin, *s_w2 = s_b1 + Hd, *s_b2 = s_w2 + Cout * Hd;
  for (int k = threadIdx.x; k < Hd * Cin; k += threads) s_w1[k] = a.w1[k];
  for (int k = threadIdx.x; k < Hd; k += threads) s_b1[k] = a.b1[k];
  for (int k = threadIdx.x; k < Cout * Hd; k += threads) s_w2[k] = a.w2[k];
  for (int k = threadIdx.x; k < Cout; k += threads) s_b2[k] = a.b2[k];
}

// pre[j] of the file header from row j of w1: the one chain of the forward and
// of the backward's recomputation. T = f32x4 (a unit) or float (one pixel);
// x(i) gives channel i.
template <int CI, bool EXACT, class T, class X>
__device__ __forceinline__ T ex_pre(const float* wrow, float bias, int Cin, X x) {
  T acc = ex_splat(bias, T{});
#pragma unroll
  for (int i = 0; i < CI; ++i)
    if (EXACT || i < Cin) acc = ex_fma(wrow[i], x(i), acc);
  return acc;
}

// the 4 values at p[0..3]; a slot at or past n holds 0
__device__ __forceinline__ f32x4 ex_load(const float* __restrict__ p, int n) {
  if (n == 4 && ((uintptr_t)p & 15u) == 0) return *(const f32x4*)p;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < n) v[e] = p[e];
  return f32x4{v[0], v[1], v[2], v[3]};
}
__device__ __forceinline__ void ex_store(float* __restrict__ p, int n, f32x4 v) {
  if (n == 4 && ((uintptr_t)p & 15u) == 0) {
    *(f32x4*)p = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < n) p[e] = v[e];
  }
}

// unit u -> image, offset of its first pixel in a plane, columns it holds
__device__ __forceinline__ void ex_unit(const ExtractArgs& a, uint32_t u, uint32_t& b, uint32_t& off,
                                        int& n) {
  b = fdiv(u, a.hq);
  const uint32_t r = u - b * a.hq.d;
  const uint32_t row = fdiv(r, a.q), x0 = 4u * (r - row * a.q.d);
  off = row * (uint32_t)a.W + x0;
  n = min(4, a.W - (int)x0);
}

// The forward of one unit. The unit's x is loaded first (Cin 16-byte loads in
// flight); the hidden units are then taken one at a time, h[j] going straight
// into the Cout output chains, which therefore see j in ascending order.
template <int CI, int HD, int CO, bool EXACT>
__device__ __forceinline__ void extract_fwd_body(const ExtractArgs& a) {
  __shared__ float sw[HD * CI + HD + CO * HD + CO];
  const int Cin = EXACT ? CI : a.Cin, Hd = EXACT ? HD : a.Hd, Cout = EXACT ? CO : a.Cout;
  ex_stage_weights(a, Cin, Hd, Cout, sw, EX_FWD_THREADS);
  const float *s_w1 = sw, *s_b1 = s_w1 + Hd * Cin, *s_w2 = s_b1 + Hd, *s_b2 = s_w2 + Cout * Hd;
  __syncthreads();
  const uint32_t u = blockIdx.x * EX_FWD_THREADS + threadIdx.x;
  if (u >= a.units) return;
  uint32_t b, off;
  int n;
  ex_unit(a, u, b, off, n);
  const uint32_t HW = (uint32_t)a.H * a.W;
  const float* xp = a.x + (size_t)b * Cin * HW + off;
  float* yp = a.y + (size_t)b * Cout * HW + off;
  f32x4 xq[CI], yq[CO];
#pragma unroll
  for (int i = 0; i < CI; ++i)
    if (EXACT || i < Cin) xq[i] = ex_load(xp + (size_t)i * HW, n);
#pragma unroll
  for (int c = 0; c < CO; ++c)
    if (EXACT || c < Cout) yq[c] = ex_splat(s_b2[c], f32x4{});
#pragma unroll 2
  for (int j = 0; j < Hd; ++j) {
    f32x4 h = ex_pre<CI, EXACT, f32x4>(s_w1 + j * Cin, s_b1[j], Cin, [&](int i) { return xq[i]; });
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = lrelu(h[e], a.slope);
#pragma unroll
    for (int c = 0; c < CO; ++c)
      if (EXACT || c < Cout) yq[c] = ex_fma(s_w2[c * Hd + j], h, yq[c]);
  }
#pragma unroll
  for (int c = 0; c < CO; ++c)
    if (EXACT || c < Cout) ex_store(yp + (size_t)c * HW, n, yq[c]);
}

// grid: ceil(units / EX_FWD_THREADS) blocks. The paper's network (15 -> 16 -> 4)
// has an instance of its own, every loop bound a constant; the other one is
// sized for the limits.
__global__ void __launch_bounds__(EX_FWD_THREADS) extract_fwd_paper_kernel(ExtractArgs a) {
  extract_fwd_body<15, 16, 4, true>(a);
}
__global__ void __launch_bounds__(EX_FWD_THREADS) extract_fwd_kernel(ExtractArgs a) {
  extract_fwd_body<EX_MAX_IN, EX_MAX_HID, EX_MAX_OUT, false>(a);
}

// dynamic LDS: P + 2 * 64 * ex_stage(Cin, Hd) floats
template <int CI, int HD, int CO, bool EXACT>
__device__ __forceinline__ void extract_bwd_body(const ExtractArgs& a) {
  extern __shared__ float smem[];
  const int Cin = EXACT ? CI : a.Cin, Hd = EXACT ? HD : a.Hd, Cout = EXACT ? CO : a.Cout;
  const int P = Hd * Cin + Hd + Cout * Hd + Cout;
  ex_stage_weights(a, Cin, Hd, Cout, smem, EX_BWD_THREADS);
  const float *s_w1 = smem, *s_b1 = s_w1 + Hd * Cin, *s_w2 = s_b1 + Hd;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the wave's staging region, laid out twice:
  //   A2 [64][17] dy,  B2 [64][sB2] h | 1;   A1 [64][sA1] dh,  B1 [64][sB1] x | 1
  constexpr int NRH = ex_r16(HD) / 16, NCX = ex_r16(CI + 1) / 16, NCH = ex_r16(HD + 1) / 16;
  const int sA2 = 17, sB2 = ex_r16(Hd + 1) + 1, sA1 = ex_r16(Hd) + 1, sB1 = ex_r16(Cin + 1) + 1;
  float* st = smem + P + wave * 64 * ex_stage(Cin, Hd);
  float *A2 = st, *B2 = st + 64 * sA2, *A1 = st, *B1 = st + 64 * sA1;
  const int l15 = lane & 15, l4 = lane >> 4;
  const uint32_t HW = (uint32_t)a.H * a.W;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc1[NRH][NCX], acc2[NCH];
#pragma unroll
  for (int r = 0; r < NRH; ++r)
#pragma unroll
    for (int c = 0; c < NCX; ++c) acc1[r][c] = zero;
#pragma unroll
  for (int c = 0; c < NCH; ++c) acc2[c] = zero;
  __syncthreads();

#pragma unroll 1
  for (int tile = blockIdx.x; tile < a.tiles; tile += a.grid) {  // uniform over the block
    const uint32_t u = (uint32_t)tile * EX_TILE + threadIdx.x;
    uint32_t b = 0, off = 0;
    int n = 0;  // a unit past the last one: no access, x = dy = 0
    if (u < a.units) ex_unit(a, u, b, off, n);
    const float* xp = a.x + (size_t)b * Cin * HW + off;
    const float* dyp = a.dy + (size_t)b * Cout * HW + off;
    f32x4 xq[CI], dyq[CO], dxq[CI];
#pragma unroll
    for (int i = 0; i < CI; ++i)
      if (EXACT || i < Cin) xq[i] = ex_load(xp + (size_t)i * HW, n);
#pragma unroll
    for (int c = 0; c < CO; ++c)
      if (EXACT || c < Cout) dyq[c] = ex_load(dyp + (size_t)c * HW, n);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float dh[HD], dxe[CI];
#pragma unroll
      for (int i = 0; i < CI; ++i) dxe[i] = 0.f;
#pragma unroll
      for (int j = 0; j < HD; ++j) {
        if (EXACT || j < Hd) {
          const float* wrow = s_w1 + j * Cin;
          const float pre =
              ex_pre<CI, EXACT, float>(wrow, s_b1[j], Cin, [&](int i) { return xq[i][e]; });
          B2[lane * sB2 + j] = lrelu(pre, a.slope);
          float g = 0.f;
#pragma unroll
          for (int c = 0; c < CO; ++c)
            if (EXACT || c < Cout) g = fmaf(s_w2[c * Hd + j], dyq[c][e], g);
          dh[j] = pre > 0.f ? g : g * a.slope;
          if (a.dx) {  // uniform; the dx chains see j in ascending order
#pragma unroll
            for (int i = 0; i < CI; ++i)
              if (EXACT || i < Cin) dxe[i] = fmaf(wrow[i], dh[j], dxe[i]);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < CO; ++c)
        if (EXACT || c < Cout) A2[lane * sA2 + c] = dyq[c][e];
      B2[lane * sB2 + Hd] = 1.f;
#pragma unroll
      for (int i = 0; i < CI; ++i)
        if (EXACT || i < Cin) dxq[i][e] = dxe[i];
      __syncthreads();
      for (int k = 0; k < 16; ++k) {
        const int p = 4 * k + l4;
        const float av = A2[p * sA2 + l15];
#pragma unroll
        for (int cb = 0; cb < NCH; ++cb)
          if (EXACT || cb * 16 <= Hd)
            acc2[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, B2[p * sB2 + cb * 16 + l15],
                                                            acc2[cb], 0, 0, 0);
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < HD; ++j)
        if (EXACT || j < Hd) A1[lane * sA1 + j] = dh[j];
#pragma unroll
      for (int i = 0; i < CI; ++i)
        if (EXACT || i < Cin) B1[lane * sB1 + i] = xq[i][e];
      B1[lane * sB1 + Cin] = 1.f;
      __syncthreads();
      for (int k = 0; k < 16; ++k) {
        const int p = 4 * k + l4;
#pragma unroll
        for (int rb = 0; rb < NRH; ++rb) {
          if (EXACT || rb * 16 < Hd) {
            const float av = A1[p * sA1 + rb * 16 + l15];
#pragma unroll
            for (int cb = 0; cb < NCX; ++cb)
              if (EXACT || cb * 16 <= Cin)
                acc1[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    av, B1[p * sB1 + cb * 16 + l15], acc1[rb][cb], 0, 0, 0);
          }
        }
      }
      __syncthreads();
    }
    if (a.dx && n > 0) {
      float* dxp = a.dx + (size_t)b * Cin * HW + off;
#pragma unroll
      for (int i = 0; i < CI; ++i)
        if (EXACT || i < Cin) ex_store(dxp + (size_t)i * HW, n, dxq[i]);
    }
  }

  // wave 0 + wave 1 -> ws[block][P]; the weights' LDS is free now (the loop ends in a barrier).
  // Lane l holds D[row 4 (l / 16) + r][column l % 16] of a 16 x 16 MFMA tile in register r.
  float* red = smem;
  float* out = a.ws + (size_t)blockIdx.x * P;
  const int O2 = Hd * Cin + Hd;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) __syncthreads();
    if (wave != 1 - pass) continue;
#pragma unroll
    for (int rb = 0; rb < NRH; ++rb)
#pragma unroll
      for (int cb = 0; cb < NCX; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = rb * 16 + 4 * l4 + r, col = cb * 16 + l15;
          if (row < Hd && col <= Cin) {
            const int idx = col < Cin ? row * Cin + col : Hd * Cin + row;
            if (pass == 0)
              red[idx] = acc1[rb][cb][r];
            else
              out[idx] = acc1[rb][cb][r] + red[idx];
          }
        }
#pragma unroll
    for (int cb = 0; cb < NCH; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * l4 + r, col = cb * 16 + l15;
        if (row < Cout && col <= Hd) {
          const int idx = O2 + (col < Hd ? row * Hd + col : Cout * Hd + row);
          if (pass == 0)
            red[idx] = acc2[cb][r];
          else
            out[idx] = acc2[cb][r] + red[idx];
        }
      }
  }
}

// grid: a.grid blocks of 2 waves. Two instances, as for the forward; the paper's
// is held to the registers of 2 waves per SIMD.
__global__ void __launch_bounds__(EX_BWD_THREADS) __attribute__((amdgpu_waves_per_eu(2, 8)))
    extract_bwd_paper_kernel(ExtractArgs a) {
  extract_bwd_body<15, 16, 4, true>(a);
}
__global__ void __launch_bounds__(EX_BWD_THREADS) extract_bwd_kernel(ExtractArgs a) {
  extract_bwd_body<EX_MAX_IN, EX_MAX_HID, EX_MAX_OUT, false>(a);
}

// grid: ceil(P / EX_MERGE_COLS) blocks of EX_SLICES * EX_MERGE_COLS threads
__global__ void __launch_bounds__(EX_SLICES* EX_MERGE_COLS)
    extract_merge_kernel(const float* __restrict__ ws, int grid, int P, int n_w1, int n_b1, int n_w2,
                         float* __restrict__ dw1, float* __restrict__ db1, float* __restrict__ dw2,
                         float* __restrict__ db2) {
  __shared__ float sh[EX_SLICES][EX_MERGE_COLS];
  const int col = threadIdx.x % EX_MERGE_COLS, slice = threadIdx.x / EX_MERGE_COLS;
  const int p = blockIdx.x * EX_MERGE_COLS + col;
  const int run = (grid + EX_SLICES - 1) / EX_SLICES;  // blocks of one slice, contiguous
  float s = 0.f;
  if (p < P) {
    const int k1 = min(grid, (slice + 1) * run);
    for (int k = slice * run; k < k1; ++k) s += ws[(size_t)k * P + p];
  }
  sh[slice][col] = s;
  __syncthreads();
  if (slice == 0 && p < P) {
    float t = sh[0][col];
#pragma unroll
    for (int k = 1; k < EX_SLICES; ++k) t += sh[k][col];
    if (p < n_w1)
      dw1[p] = t;
    else if (p < n_w1 + n_b1)
      db1[p - n_w1] = t;
    else if (p < n_w1 + n_b1 + n_w2)
      dw2[p - n_w1 - n_b1] = t;
    else
      db2[p - n_w1 - n_b1 - n_w2] = t;
  }
}

struct ExPlan {
  long long units;
  int tiles, grid, P;
};

// false: a dimension outside the limits (no message: the callers say which)
static bool ex_plan(int B, int Cin, int H, int W, int Hd, int Cout, ExPlan& p) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin < 1 || Cin > EX_MAX_IN || Hd < 1 || Hd > EX_MAX_HID ||
      Cout < 1 || Cout > EX_MAX_OUT)
    return false;
  if ((long long)(Cin > Cout ? Cin : Cout) * H * W >= (1ll << 31)) return false;
  p.units = (long long)B * H * ((W + 3) / 4);
  if (p.units >= (1ll << 31)) return false;
  p.tiles = ceil_div(p.units, EX_TILE);
  p.grid = p.tiles < EX_MAX_GRID ? p.tiles : EX_MAX_GRID;
  p.P = ex_params(Cin, Hd, Cout);
  return true;
}

static int ex_check(const char* what, int B, int Cin, int H, int W, int Hd, int Cout, ExPlan& p) {
  NSM_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: shape %d x %d x %d x %d", what, B, Cin, H, W);
  NSM_CHECK_ARG(Cin >= 1 && Cin <= EX_MAX_IN, "%s: %d input channels (1 to %d)", what, Cin,
                EX_MAX_IN);
  NSM_CHECK_ARG(Hd >= 1 && Hd <= EX_MAX_HID, "%s: %d hidden channels (1 to %d)", what, Hd,
                EX_MAX_HID);
  NSM_CHECK_ARG(Cout >= 1 && Cout <= EX_MAX_OUT, "%s: %d output channels (1 to %d)", what, Cout,
                EX_MAX_OUT);
  NSM_CHECK_ARG(ex_plan(B, Cin, H, W, Hd, Cout, p),
                "%s: %d images of %d (in) and %d (out) x %d x %d samples (an image holds fewer "
                "than 2^31, the batch fewer than 2^33 pixels)", what, B, Cin, Cout, H, W);
  return 0;
}

static ExtractArgs ex_args(int Cin, int H, int W, int Hd, int Cout, float slope, const ExPlan& p) {
  ExtractArgs a = {};
  a.Cin = Cin, a.Hd = Hd, a.Cout = Cout, a.H = H, a.W = W, a.slope = slope;
  a.units = (uint32_t)p.units, a.tiles = p.tiles, a.grid = p.grid;
  a.q = make_fastdiv((uint32_t)((W + 3) / 4));
  a.hq = make_fastdiv((uint32_t)H * (uint32_t)((W + 3) / 4));
  return a;
}

}  // namespace nsm

using namespace nsm;

extern "C" int nsm_extract_fwd(const float* x, int B, int Cin, int H, int W, const float* w1,
                               const float* b1, int Hd, const float* w2, const float* b2, int Cout,
                               float slope, float* y, void* stream) {
  NSM_CHECK_ARG(x && w1 && b1 && w2 && b2 && y, "extract_fwd: null pointer");
  ExPlan p;
  if (int rc = ex_check("extract_fwd", B, Cin, H, W, Hd, Cout, p)) return rc;
  NSM_CHECK_ARG((((uintptr_t)x | (uintptr_t)y | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 |
                  (uintptr_t)b2) & 3u) == 0, "extract_fwd: unaligned pointer");
  ExtractArgs a = ex_args(Cin, H, W, Hd, Cout, slope, p);
  a.x = x, a.w1 = w1, a.b1 = b1, a.w2 = w2, a.b2 = b2, a.y = y;
  const dim3 grid((unsigned)ceil_div(p.units, EX_FWD_THREADS)), block(EX_FWD_THREADS);
  if (Cin == 15 && Hd == 16 && Cout == 4)
    hipLaunchKernelGGL(extract_fwd_paper_kernel, grid, block, 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(extract_fwd_kernel, grid, block, 0, as_stream(stream), a);
  NSM_LAUNCH_CHECK("extract_fwd");
  return 0;
}

extern "C" int nsm_extract_bwd_plan(int B, int Cin, int H, int W, int Hd, int Cout, int32_t* plan) {
  NSM_CHECK_ARG(plan, "extract_bwd_plan: null pointer");
  ExPlan p;
  if (int rc = ex_check("extract_bwd_plan", B, Cin, H, W, Hd, Cout, p)) return rc;
  plan[0] = p.grid, plan[1] = p.tiles, plan[2] = EX_TILE, plan[3] = 4, plan[4] = EX_MAX_GRID;
  plan[5] = p.P;
  return 0;
}

extern "C" size_t nsm_extract_bwd_ws(int B, int Cin, int H, int W, int Hd, int Cout) {
  ExPlan p;
  if (!ex_plan(B, Cin, H, W, Hd, Cout, p)) return 0;
  return (size_t)p.grid * p.P * sizeof(float);
}

extern "C" int nsm_extract_bwd(const float* x, const float* dy, int B, int Cin, int H, int W,
                               const float* w1, const float* b1, int Hd, const float* w2,
                               const float* b2, int Cout, float slope, float* dw1, float* db1,
                               float* dw2, float* db2, float* dx, void* ws, void* stream) {
  NSM_CHECK_ARG(x && dy && w1 && b1 && w2 && b2 && dw1 && db1 && dw2 && db2 && ws,
                "extract_bwd: null pointer (dx alone may be null)");
  ExPlan p;
  if (int rc = ex_check("extract_bwd", B, Cin, H, W, Hd, Cout, p)) return rc;
  NSM_CHECK_ARG((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)w1 | (uintptr_t)b1 |
                  (uintptr_t)w2 | (uintptr_t)b2 | (uintptr_t)dw1 | (uintptr_t)db1 |
                  (uintptr_t)dw2 | (uintptr_t)db2 | (uintptr_t)ws) & 3u) == 0,
                "extract_bwd: unaligned pointer");
  ExtractArgs a = ex_args(Cin, H, W, Hd, Cout, slope, p);
  a.x = x, a.dy = dy, a.w1 = w1, a.b1 = b1, a.w2 = w2, a.b2 = b2, a.dx = dx, a.ws = (float*)ws;
  const size_t lds = ((size_t)p.P + 2 * 64 * (size_t)ex_stage(Cin, Hd)) * sizeof(float);
  const dim3 grid((unsigned)p.grid), block(EX_BWD_THREADS);
  if (Cin == 15 && Hd == 16 && Cout == 4)
    hipLaunchKernelGGL(extract_bwd_paper_kernel, grid, block, lds, as_stream(stream), a);
  else
    hipLaunchKernelGGL(extract_bwd_kernel, grid, block, lds, as_stream(stream), a);
  hipLaunchKernelGGL(extract_merge_kernel, dim3((unsigned)ceil_div(p.P, EX_MERGE_COLS)),
                     dim3(EX_SLICES * EX_MERGE_COLS), 0, as_stream(stream), (const float*)a.ws,
                     p.grid, p.P, Hd * Cin, Hd, Cout * Hd, dw1, db1, dw2, db2);
  NSM_LAUNCH_CHECK("extract_bwd");
  return 0;
}
