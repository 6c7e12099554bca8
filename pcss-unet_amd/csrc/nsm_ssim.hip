// The structural-similarity term of CustomLoss (customLoss.py:187-191:
// `1 - pytorch_msssim.ssim(output, target)`) and the SSIM metric, fp32, on
// [B,1,H,W] images o (output) and t (target):
//   g: the 11-tap Gaussian (sigma 1.5, sum 1); <.> = g along H and along W, a
//   valid correlation: (H-10) x (W-10) windows per image;
//   S = (2ab + C1)/(a^2 + b^2 + C1) * (2(r - ab) + C2)/((p - a^2) + (q - b^2) + C2),
//   a = <o>, b = <t>, p = <o^2>, q = <t^2>, r = <ot>, C1 = (0.01 R)^2,
//   C2 = (0.03 R)^2; ssim_b = mean of S over image b, ssim = mean_b ssim_b.
// The kernels blur five other maps from which S follows without the
// cancellations of p - a^2 and r - ab: with U = o - 0.5, V = o - t,
// Wt = U - V (= t - 0.5),
//   a' = <U>, dm = <V>, p' = <U^2>, q' = <Wt^2>, z = <V^2>; b' = a' - dm;
//   1 - lum = dm^2 / D1,            D1 = (a'+.5)^2 + (b'+.5)^2 + C1,
//   1 - cs  = (z - dm^2) / D2,      D2 = (p' - a'^2) + (q' - b'^2) + C2,
//   1 - S   = (1 - lum) + lum (1 - cs)
// (variances and covariance are shift-invariant; 2 cov = var_o + var_t -
// var_(o-t)). o == t gives 1 - S == 0 exactly.
// One block works on an ST_H x ST_W tile of windows (forward) or pixels
// (backward) of ONE image; both stage a (ST_H+10) x (ST_W+10) region in LDS,
// zero outside the image (the valid window range), run the horizontal pass
// into LDS and the vertical pass in registers, so nothing leaks between the
// images of a batch or wraps from a neighbouring row.
//  * forward: sum of 1 - S per block (fixed order) -> partial; optionally the
//    per-window coefficients A = dS/da', P = dS/dp', Z = dS/dz (three planes of
//    B*(H-10)*(W-10) floats) for the backward; a single-block finalize in
//    double. No atomics: bitwise reproducible.
//  * backward: dssim/do[i] = (1/n) ((g*A)[i] + 2 U[i] (g*P)[i] + 2 V[i] (g*Z)[i]),
//    `*` the full (transposed) separable correlation: pixel i gathers from the
//    up to 11 x 11 windows that cover it. One writer per element.
#include <math.h>
#include "nsm_common.h"

namespace nsm {

constexpr int ST_H = 16, ST_W = 64;  // windows (fwd) / pixels (bwd) of one block's tile
constexpr int ST_THREADS = 256;      // thread = one column x 4 consecutive rows
constexpr int SWIN = 11, SHALO = SWIN - 1;
constexpr int SR_H = ST_H + SHALO, SR_W = ST_W + SHALO;  // staged region: 26 x 74
constexpr int ST_ROWS = ST_H / (ST_THREADS / ST_W);      // rows per thread: 4

struct Gauss11 {
  float w[SWIN];
};

// exp(-(i-5)^2 / (2 * 1.5^2)) / sum
static Gauss11 gauss11() {
  Gauss11 g;
  double v[SWIN], sum = 0.0;
  for (int i = 0; i < SWIN; ++i) {
    const double c = i - SWIN / 2;
    v[i] = exp(-(c * c) / (2.0 * 1.5 * 1.5));
    sum += v[i];
  }
  for (int i = 0; i < SWIN; ++i) g.w[i] = (float)(v[i] / sum);
  return g;
}

// flat block index -> image and tile origin
__device__ __forceinline__ void ssim_tile_of(int blk, int ntx, int nty, int& b, int& y0, int& x0) {
  const int per = ntx * nty;
  b = blk / per;
  const int r = blk - b * per;
  const int ty = r / ntx;
  y0 = ty * ST_H;
  x0 = (r - ty * ntx) * ST_W;
}

// One window from its five blurred maps: T = 1 - S and the partials of S.
__device__ __forceinline__ void ssim_point(float a, float dm, float p, float q, float z, float c1,
                                           float c2, float& T, float& A, float& P, float& Z) {
#pragma clang fp contract(off)
  const float b = a - dm;
  const float m1 = a + 0.5f, m2 = b + 0.5f;
  const float d1 = (m1 * m1 + m2 * m2) + c1;
  const float d2 = (fmaf(-a, a, p) + fmaf(-b, b, q)) + c2;
  const float oml = dm * dm / d1, lum = 1.f - oml;
  const float omc = fmaf(-dm, dm, z) / d2, cs = 1.f - omc;
  T = oml + omc * lum;
  A = 2.f * (cs * (oml * m1 - dm) / d1 + lum * (dm - a * omc) / d2);
  P = lum * omc / d2;
  Z = -lum / d2;
}

// partial[blk] = sum over the block's valid windows of 1 - S; coef (may be
// NULL): planes A, P, Z of `plane` floats each, [B][H-10][W-10]
__global__ void __launch_bounds__(ST_THREADS)
    ssim_fwd_kernel(const float* __restrict__ o, const float* __restrict__ t, int H, int W,
                    int ntx, int nty, Gauss11 G, float c1, float c2,
                    float* __restrict__ partial, float* __restrict__ coef, size_t plane) {
  __shared__ float su[SR_H * SR_W], sv[SR_H * SR_W];
  __shared__ float hm[5][SR_H * ST_W];
  __shared__ float red[ST_THREADS / 64];
  int b, y0, x0;
  ssim_tile_of(blockIdx.x, ntx, nty, b, y0, x0);
  const int Hw = H - SHALO, Ww = W - SHALO;
  const size_t img = (size_t)b * H * W;
  for (int i = threadIdx.x; i < SR_H * SR_W; i += ST_THREADS) {
    const int ry = i / SR_W, rx = i - ry * SR_W;
    const int y = y0 + ry, x = x0 + rx;
    float u = 0.f, v = 0.f;
    if (y < H && x < W) {
      const size_t g = img + (size_t)y * W + x;
      const float ov = o[g];
      u = ov - 0.5f;
      v = ov - t[g];
    }
    su[i] = u;
    sv[i] = v;
  }
  __syncthreads();
  // horizontal pass: the five maps of every staged row at the tile's columns
  for (int i = threadIdx.x; i < SR_H * ST_W; i += ST_THREADS) {
    const int ry = i / ST_W, x = i - ry * ST_W;
    const float* pu = su + ry * SR_W + x;
    const float* pv = sv + ry * SR_W + x;
    float a = 0.f, dm = 0.f, p = 0.f, q = 0.f, z = 0.f;
#pragma unroll
    for (int k = 0; k < SWIN; ++k) {
      const float u = pu[k], v = pv[k], wt = u - v, gk = G.w[k];
      a = fmaf(gk, u, a);
      dm = fmaf(gk, v, dm);
      p = fmaf(gk, u * u, p);
      q = fmaf(gk, wt * wt, q);
      z = fmaf(gk, v * v, z);
    }
    hm[0][i] = a;
    hm[1][i] = dm;
    hm[2][i] = p;
    hm[3][i] = q;
    hm[4][i] = z;
  }
  __syncthreads();
  // vertical pass: ST_ROWS consecutive windows of one column per thread
  const int tx = threadIdx.x & (ST_W - 1), ty = threadIdx.x / ST_W;
  float acc[ST_ROWS][5];
#pragma unroll
  for (int j = 0; j < ST_ROWS; ++j)
#pragma unroll
    for (int m = 0; m < 5; ++m) acc[j][m] = 0.f;
#pragma unroll
  for (int r = 0; r < ST_ROWS + SHALO; ++r) {
    float h[5];
#pragma unroll
    for (int m = 0; m < 5; ++m) h[m] = hm[m][(ty * ST_ROWS + r) * ST_W + tx];
#pragma unroll
    for (int j = 0; j < ST_ROWS; ++j) {
      const int k = r - j;
      if (k >= 0 && k < SWIN) {
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[j][m] = fmaf(G.w[k], h[m], acc[j][m]);
      }
    }
  }
  float tsum = 0.f;
  const int wx = x0 + tx;
#pragma unroll
  for (int j = 0; j < ST_ROWS; ++j) {
    const int wy = y0 + ty * ST_ROWS + j;
    if (wy < Hw && wx < Ww) {
      float T, A, P, Z;
      ssim_point(acc[j][0], acc[j][1], acc[j][2], acc[j][3], acc[j][4], c1, c2, T, A, P, Z);
      tsum += T;
      if (coef) {
        const size_t g = ((size_t)b * Hw + wy) * Ww + wx;
        coef[g] = A;
        coef[plane + g] = P;
        coef[2 * plane + g] = Z;
      }
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) tsum += __shfl_xor(tsum, s, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = tsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = 0.f;
    for (int w = 0; w < ST_THREADS / 64; ++w) r += red[w];
    partial[blockIdx.x] = r;
  }
}

// out[0] = ssim, out[1] = 1 - ssim, out[2] = (base ? *base : 0) + w * (1 - ssim),
// out[3 + b] = ssim of image b. One block; one wave per image at a time, every
// sum in double and in a fixed order.
__global__ void __launch_bounds__(ST_THREADS)
    ssim_finalize_kernel(const float* __restrict__ partial, int per, int B, double nwin, float w,
                         const float* __restrict__ base, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double sh[ST_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double wacc = 0.0;
  for (int b = wave; b < B; b += ST_THREADS / 64) {
    double s = 0.0;
    for (int i = lane; i < per; i += 64) s += (double)partial[(size_t)b * per + i];
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k, 64);
    const double mt = s / nwin;
    if (lane == 0) out[3 + b] = (float)(1.0 - mt);
    wacc += mt;
  }
  if (lane == 0) sh[wave] = wacc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int k = 0; k < ST_THREADS / 64; ++k) tot += sh[k];
    const double mt = tot / (double)B;
    const float loss = (float)mt;
    out[0] = (float)(1.0 - mt);
    out[1] = loss;
    const float wl = w * loss;
    out[2] = base ? base[0] + wl : wl;
  }
}

// grad[i] (+)= -(w * gs / n) * ((g*A)[i] + 2 U[i] (g*P)[i] + 2 V[i] (g*Z)[i]),
// the gradient of w * (1 - ssim) times the upstream gs; n = B (H-10) (W-10)
__global__ void __launch_bounds__(ST_THREADS)
    ssim_bwd_kernel(const float* __restrict__ o, const float* __restrict__ t,
                    const float* __restrict__ coef, size_t plane, int H, int W, int ntx, int nty,
                    Gauss11 G, float n, float w, const float* __restrict__ gscale, float* grad,
                    int accumulate) {
  __shared__ float sc[3][SR_H * SR_W];
  __shared__ float hm[3][SR_H * ST_W];
  int b, y0, x0;
  ssim_tile_of(blockIdx.x, ntx, nty, b, y0, x0);
  const int Hw = H - SHALO, Ww = W - SHALO;
  // region (ry, rx) is window (y0 - 10 + ry, x0 - 10 + rx); 0 outside the valid range
  for (int i = threadIdx.x; i < SR_H * SR_W; i += ST_THREADS) {
    const int ry = i / SR_W, rx = i - ry * SR_W;
    const int wy = y0 - SHALO + ry, wx = x0 - SHALO + rx;
    float a = 0.f, p = 0.f, z = 0.f;
    if (wy >= 0 && wy < Hw && wx >= 0 && wx < Ww) {
      const size_t g = ((size_t)b * Hw + wy) * Ww + wx;
      a = coef[g];
      p = coef[plane + g];
      z = coef[2 * plane + g];
    }
    sc[0][i] = a;
    sc[1][i] = p;
    sc[2][i] = z;
  }
  __syncthreads();
  // pixel x sits at offset j = 10 - k of window x - 10 + k: weight g[10 - k]
  for (int i = threadIdx.x; i < SR_H * ST_W; i += ST_THREADS) {
    const int ry = i / ST_W, x = i - ry * ST_W;
    const int c = ry * SR_W + x;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < SWIN; ++k) {
      const float gk = G.w[SHALO - k];
      s0 = fmaf(gk, sc[0][c + k], s0);
      s1 = fmaf(gk, sc[1][c + k], s1);
      s2 = fmaf(gk, sc[2][c + k], s2);
    }
    hm[0][i] = s0;
    hm[1][i] = s1;
    hm[2][i] = s2;
  }
  __syncthreads();
  const int tx = threadIdx.x & (ST_W - 1), ty = threadIdx.x / ST_W;
  float acc[ST_ROWS][3];
#pragma unroll
  for (int j = 0; j < ST_ROWS; ++j)
#pragma unroll
    for (int m = 0; m < 3; ++m) acc[j][m] = 0.f;
#pragma unroll
  for (int r = 0; r < ST_ROWS + SHALO; ++r) {
    float h[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) h[m] = hm[m][(ty * ST_ROWS + r) * ST_W + tx];
#pragma unroll
    for (int j = 0; j < ST_ROWS; ++j) {
      const int k = r - j;
      if (k >= 0 && k < SWIN) {
#pragma unroll
        for (int m = 0; m < 3; ++m) acc[j][m] = fmaf(G.w[SHALO - k], h[m], acc[j][m]);
      }
    }
  }
  const float gs = gscale ? gscale[0] : 1.f;
  const float c = -((w * gs) / n);
  const int x = x0 + tx;
  const size_t img = (size_t)b * H * W;
#pragma unroll
  for (int j = 0; j < ST_ROWS; ++j) {
    const int y = y0 + ty * ST_ROWS + j;
    if (y < H && x < W) {
      const size_t g = img + (size_t)y * W + x;
      const float ov = o[g];
      const float u = ov - 0.5f, v = ov - t[g];
      float inner, val;
      {
        // rounded one by one: the same bits whatever the upstream scale is
#pragma clang fp contract(off)
        inner = (acc[j][0] + 2.f * u * acc[j][1]) + 2.f * v * acc[j][2];
        val = c * inner;
      }
      grad[g] = accumulate ? grad[g] + val : val;
    }
  }
}

static bool ssim_shape_ok(int B, int H, int W) {
  if (B <= 0 || H < SWIN || W < SWIN) return false;
  const long long nb = (long long)B * ceil_div(H, ST_H) * ceil_div(W, ST_W);
  return nb < (1ll << 30) && (long long)H * W < (1ll << 31);
}

}  // namespace nsm

using namespace nsm;

extern "C" int nsm_ssim_blocks(int B, int H, int W) {
  if (!ssim_shape_ok(B, H, W)) return 0;
  return B * ceil_div(H - SHALO, ST_H) * ceil_div(W - SHALO, ST_W);
}

extern "C" int nsm_ssim_fwd(const float* o, const float* t, int B, int H, int W, float data_range,
                            float w, const float* base, float* partial, float* coef, float* out,
                            void* stream) {
  NSM_CHECK_ARG(o && t && partial && out, "ssim_fwd: null pointer");
  NSM_CHECK_ARG(ssim_shape_ok(B, H, W), "ssim_fwd: shape %d x %d x %d", B, H, W);
  NSM_CHECK_ARG(data_range > 0.f, "ssim_fwd: data_range %g", (double)data_range);
  const int Hw = H - SHALO, Ww = W - SHALO;
  const int ntx = ceil_div(Ww, ST_W), nty = ceil_div(Hw, ST_H), nb = B * ntx * nty;
  const float k1 = 0.01f * data_range, k2 = 0.03f * data_range;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(ssim_fwd_kernel, dim3(nb), dim3(ST_THREADS), 0, s, o, t, H, W, ntx, nty,
                     gauss11(), k1 * k1, k2 * k2, partial, coef, (size_t)B * Hw * Ww);
  hipLaunchKernelGGL(ssim_finalize_kernel, dim3(1), dim3(ST_THREADS), 0, s, partial, ntx * nty, B,
                     (double)Hw * Ww, w, base, out);
  NSM_LAUNCH_CHECK("ssim_fwd");
  return 0;
}

extern "C" int nsm_ssim_bwd(const float* o, const float* t, const float* coef, int B, int H, int W,
                            float w, const float* gscale, float* grad, int accumulate,
                            void* stream) {
  NSM_CHECK_ARG(o && t && coef && grad, "ssim_bwd: null pointer");
  NSM_CHECK_ARG(ssim_shape_ok(B, H, W), "ssim_bwd: shape %d x %d x %d", B, H, W);
  hipStream_t s = as_stream(stream);
  if (w == 0.f) {  // contributes exactly 0
    if (!accumulate && hipMemsetAsync(grad, 0, sizeof(float) * (size_t)B * H * W, s) != hipSuccess)
      return fail(NSM_E_HIP, "ssim_bwd: memset");
    return 0;
  }
  const int Hw = H - SHALO, Ww = W - SHALO;
  const int ntx = ceil_div(W, ST_W), nty = ceil_div(H, ST_H), nb = B * ntx * nty;
  hipLaunchKernelGGL(ssim_bwd_kernel, dim3(nb), dim3(ST_THREADS), 0, s, o, t, coef,
                     (size_t)B * Hw * Ww, H, W, ntx, nty, gauss11(),
                     (float)((double)B * Hw * Ww), w, gscale, grad, accumulate);
  NSM_LAUNCH_CHECK("ssim_bwd");
  return 0;
}
