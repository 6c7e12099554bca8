// The opt-in detail terms of CustomLoss (customLoss.py:139-185), fp32, on
// [B,1,H,W] images o (output) and t (target), N = B*H*W:
//   HF  = mean|hf(o) - hf(t)|, hf(x) = x - G*x, G the 5x5 Gaussian (sigma 1);
//   PEN = sum m|o - t| / (M + 1e-8), m = 0.1 < t < 0.9, M = sum m;
//   SOB = mean|mag(o) - mag(t)|, mag = sqrt(gx^2 + gy^2 + 1e-6) (3x3 Sobel).
// Every filter is a cross-correlation with zero padding at the image's own
// border. One block works on a DT_H x DT_W tile of ONE image, staged into LDS
// with a zero halo, so nothing leaks between the images of a batch or wraps
// from the previous row.
//  * forward: halo 2; four float partial sums per block (fixed order), then a
//    single-block finalize in double. No atomics: bitwise reproducible.
//  * backward: recomputed from o and t (nothing N-sized is saved). Halo 4:
//    d = o - t on tile+4, s = sign(d - G*d) on tile+2, the Sobel fields
//    u*gx/mag, u*gy/mag on tile+1, then each pixel of the tile gathers its
//    gradient. One writer per element.
#include <math.h>
#include "nsm_common.h"

namespace nsm {

constexpr int DT_H = 16, DT_W = 64;  // pixels of one block's tile (256 threads, 4 each)
constexpr int DT_THREADS = 256;

struct Gauss5 {
  float w[25];
};

// customLoss.py:106-114 in fp32: exp(-(x^2 + y^2) / (2 sigma^2)) / sum
static Gauss5 gauss5() {
  Gauss5 g;
  float sum = 0.f;
  for (int y = -2; y <= 2; ++y)
    for (int x = -2; x <= 2; ++x) {
      const float v = expf(-(float)(x * x + y * y) / 2.f);
      g.w[(y + 2) * 5 + (x + 2)] = v;
      sum += v;
    }
  for (int k = 0; k < 25; ++k) g.w[k] /= sum;
  return g;
}

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// Stage the (DT_H + 2*HALO) x (DT_W + 2*HALO) window of image `img` around the
// tile at (y0, x0) into so / st, zero outside the image.
template <int HALO>
__device__ __forceinline__ void stage_tile(const float* __restrict__ o, const float* __restrict__ t,
                                           size_t img, int H, int W, int y0, int x0, float* so,
                                           float* st) {
  constexpr int RW = DT_W + 2 * HALO, RH = DT_H + 2 * HALO;
  for (int i = threadIdx.x; i < RH * RW; i += DT_THREADS) {
    const int ry = i / RW, rx = i - ry * RW;
    const int y = y0 - HALO + ry, x = x0 - HALO + rx;
    float a = 0.f, b = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t g = img + (size_t)y * W + x;
      a = o[g];
      b = t[g];
    }
    so[i] = a;
    st[i] = b;
  }
}

// 3x3 Sobel magnitude at the centre `p` of a row-major LDS window of width RW
__device__ __forceinline__ void sobel(const float* p, int RW, float& gx, float& gy, float& mag) {
  const float a = p[-RW - 1], b = p[-RW], c = p[-RW + 1];
  const float d = p[-1], f = p[1];
  const float g = p[RW - 1], h = p[RW], i = p[RW + 1];
  gx = (c - a) + 2.f * (f - d) + (i - g);
  gy = (g - a) + 2.f * (h - b) + (i - c);
  mag = sqrtf(gx * gx + gy * gy + 1e-6f);
}

// flat block index -> image and tile origin
__device__ __forceinline__ void tile_of(int blk, int ntx, int nty, int& b, int& y0, int& x0) {
  const int per = ntx * nty;
  b = blk / per;
  const int r = blk - b * per;
  const int ty = r / ntx;
  y0 = ty * DT_H;
  x0 = (r - ty * ntx) * DT_W;
}

// partial[4*blk + {0,1,2,3}] = sum |r|, sum m|o-t|, sum m, sum |mag_o - mag_t|
__global__ void __launch_bounds__(DT_THREADS)
    detail_fwd_kernel(const float* __restrict__ o, const float* __restrict__ t, int H, int W,
                      int ntx, int nty, Gauss5 G, float* __restrict__ partial) {
  constexpr int HALO = 2, RW = DT_W + 2 * HALO, RH = DT_H + 2 * HALO;
  __shared__ float so[RH * RW], st[RH * RW];
  __shared__ float red[4][DT_THREADS / 64];
  int b, y0, x0;
  tile_of(blockIdx.x, ntx, nty, b, y0, x0);
  stage_tile<HALO>(o, t, (size_t)b * H * W, H, W, y0, x0, so, st);
  __syncthreads();
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < DT_H * DT_W; i += DT_THREADS) {
    const int ly = i / DT_W, lx = i - ly * DT_W;
    if (y0 + ly >= H || x0 + lx >= W) continue;
    const int c = (ly + HALO) * RW + lx + HALO;
    const float ov = so[c], tv = st[c];
    // hf(o) - hf(t) = d - G*d with d = o - t (the filter is linear)
    float blur = 0.f;
#pragma unroll
    for (int ky = 0; ky < 5; ++ky)
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) {
        const int q = c + (ky - 2) * RW + (kx - 2);
        blur += G.w[ky * 5 + kx] * (so[q] - st[q]);
      }
    acc[0] += fabsf((ov - tv) - blur);
    if (tv > 0.1f && tv < 0.9f) {
      acc[1] += fabsf(ov - tv);
      acc[2] += 1.f;
    }
    float gx, gy, mo, mt;
    sobel(so + c, RW, gx, gy, mo);
    sobel(st + c, RW, gx, gy, mt);
    acc[3] += fabsf(mo - mt);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float v = acc[k];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    if (lane == 0) red[k][wv] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    float r = 0.f;
    for (int w = 0; w < DT_THREADS / 64; ++w) r += red[threadIdx.x][w];
    partial[4 * (size_t)blockIdx.x + threadIdx.x] = r;
  }
}

// out[0..4] = HF, PEN, SOB, M, base + (w_hf*HF + w_pen*PEN) + w_sob*SOB; one
// block, fixed-order double accumulation (finalize_mean_kernel's scheme)
__global__ void __launch_bounds__(DT_THREADS)
    detail_finalize_kernel(const float* __restrict__ partial, int nblk, double n, float w_hf,
                           float w_pen, float w_sob, const float* __restrict__ base,
                           float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double sh[4][DT_THREADS];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblk; b += DT_THREADS)
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += (double)partial[4 * (size_t)b + k];
#pragma unroll
  for (int k = 0; k < 4; ++k) sh[k][threadIdx.x] = s[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot[4];
    for (int k = 0; k < 4; ++k) {
      double a = 0.0;
      for (int i = 0; i < DT_THREADS; ++i) a += sh[k][i];
      tot[k] = a;
    }
    const float hf = (float)(tot[0] / n);
    const float pen = (float)(tot[1] / (tot[2] + 1e-8));
    const float sob = (float)(tot[3] / n);
    out[0] = hf;
    out[1] = pen;
    out[2] = sob;
    out[3] = (float)tot[2];
    const float w = (w_hf * hf + w_pen * pen) + w_sob * sob;
    out[4] = base ? base[0] + w : w;
  }
}

// grad[p] (+)= (c_hf * (s[p] - sum_k G[k] s[p+k]) + c_pen * m[p] sign(o[p]-t[p]))
//             + c_sob * sum_q (A[q] Kx[p-q] + B[q] Ky[p-q]),
// c_hf = w_hf*gs/N, c_pen = w_pen*gs/(M + 1e-8), c_sob = w_sob*gs/N, A = u gx_o/mag_o,
// B = u gy_o/mag_o. A term whose weight is 0 is skipped and contributes exactly 0.
__global__ void __launch_bounds__(DT_THREADS)
    detail_bwd_kernel(const float* __restrict__ o, const float* __restrict__ t, int H, int W,
                      int ntx, int nty, Gauss5 G, float n, float w_hf, float w_pen, float w_sob,
                      const float* __restrict__ mcount, const float* __restrict__ gscale,
                      float* grad, int accumulate) {
  // every product below is rounded on its own, so that a term's value does not
  // depend on which other terms are switched on
#pragma clang fp contract(off)
  constexpr int HALO = 4, RW = DT_W + 2 * HALO, RH = DT_H + 2 * HALO;
  constexpr int SW = DT_W + 4, SH = DT_H + 4;  // s: tile + 2
  constexpr int FW = DT_W + 2, FH = DT_H + 2;  // Sobel fields: tile + 1
  __shared__ float so[RH * RW], st[RH * RW], sd[RH * RW];
  __shared__ float ss[SH * SW], fa[FH * FW], fb[FH * FW];
  int b, y0, x0;
  tile_of(blockIdx.x, ntx, nty, b, y0, x0);
  const size_t img = (size_t)b * H * W;
  stage_tile<HALO>(o, t, img, H, W, y0, x0, so, st);
  __syncthreads();
  for (int i = threadIdx.x; i < RH * RW; i += DT_THREADS) sd[i] = so[i] - st[i];
  __syncthreads();
  if (w_hf != 0.f) {
    for (int i = threadIdx.x; i < SH * SW; i += DT_THREADS) {
      const int ry = i / SW, rx = i - ry * SW;
      const int y = y0 - 2 + ry, x = x0 - 2 + rx;
      float s = 0.f;
      if (y >= 0 && y < H && x >= 0 && x < W) {
        const int c = (ry + 2) * RW + rx + 2;
        float blur = 0.f;
#pragma unroll
        for (int ky = 0; ky < 5; ++ky)
#pragma unroll
          for (int kx = 0; kx < 5; ++kx)
            blur += G.w[ky * 5 + kx] * sd[c + (ky - 2) * RW + (kx - 2)];
        s = sgn(sd[c] - blur);
      }
      ss[i] = s;
    }
  }
  if (w_sob != 0.f) {
    for (int i = threadIdx.x; i < FH * FW; i += DT_THREADS) {
      const int ry = i / FW, rx = i - ry * FW;
      const int y = y0 - 1 + ry, x = x0 - 1 + rx;
      float a = 0.f, bq = 0.f;
      if (y >= 0 && y < H && x >= 0 && x < W) {
        const int c = (ry + 3) * RW + rx + 3;
        float gx, gy, mo, tx, ty, mt;
        sobel(so + c, RW, gx, gy, mo);
        sobel(st + c, RW, tx, ty, mt);
        const float u = sgn(mo - mt);
        a = u * gx / mo;
        bq = u * gy / mo;
      }
      fa[i] = a;
      fb[i] = bq;
    }
  }
  __syncthreads();
  const float gs = gscale ? gscale[0] : 1.f;
  const float c_hf = (w_hf * gs) / n;
  const float c_sob = (w_sob * gs) / n;
  const float c_pen = w_pen != 0.f ? (w_pen * gs) / (mcount[0] + 1e-8f) : 0.f;
  for (int i = threadIdx.x; i < DT_H * DT_W; i += DT_THREADS) {
    const int ly = i / DT_W, lx = i - ly * DT_W;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    float hf = 0.f, pen = 0.f, sob = 0.f;
    if (w_hf != 0.f) {
      const int c = (ly + 2) * SW + lx + 2;
      float blur = 0.f;
#pragma unroll
      for (int ky = 0; ky < 5; ++ky)
#pragma unroll
        for (int kx = 0; kx < 5; ++kx)
          blur += G.w[ky * 5 + kx] * ss[c + (ky - 2) * SW + (kx - 2)];
      hf = c_hf * (ss[c] - blur);
    }
    if (w_pen != 0.f) {
      const int c = (ly + HALO) * RW + lx + HALO;
      const float tv = st[c];
      if (tv > 0.1f && tv < 0.9f) pen = c_pen * sgn(sd[c]);
    }
    if (w_sob != 0.f) {
      // gx[q] = sum_k Kx[k] x[q+k]: d gx[q] / d x[p] = Kx[p-q] = -Kx[q-p]
      const float* A = fa + (ly + 1) * FW + lx + 1;
      const float* Bf = fb + (ly + 1) * FW + lx + 1;
      const float ax = (A[-FW + 1] - A[-FW - 1]) + 2.f * (A[1] - A[-1]) + (A[FW + 1] - A[FW - 1]);
      const float by = (Bf[FW - 1] - Bf[-FW - 1]) + 2.f * (Bf[FW] - Bf[-FW]) +
                       (Bf[FW + 1] - Bf[-FW + 1]);
      sob = c_sob * -(ax + by);
    }
    const float v = (hf + pen) + sob;
    const size_t g = img + (size_t)y * W + x;
    grad[g] = accumulate ? grad[g] + v : v;
  }
}

static bool detail_shape_ok(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return false;
  const long long nb = (long long)B * ceil_div(H, DT_H) * ceil_div(W, DT_W);
  return nb < (1ll << 30) && (long long)H * W < (1ll << 31);
}

}  // namespace nsm

using namespace nsm;

extern "C" int nsm_detail_blocks(int B, int H, int W) {
  if (!detail_shape_ok(B, H, W)) return 0;
  return B * ceil_div(H, DT_H) * ceil_div(W, DT_W);
}

extern "C" int nsm_detail_loss_fwd(const float* o, const float* t, int B, int H, int W,
                                   float w_hf, float w_pen, float w_sob, const float* base,
                                   float* partial, float* out, void* stream) {
  NSM_CHECK_ARG(o && t && partial && out, "detail_loss_fwd: null pointer");
  NSM_CHECK_ARG(detail_shape_ok(B, H, W), "detail_loss_fwd: shape %d x %d x %d", B, H, W);
  const int ntx = ceil_div(W, DT_W), nty = ceil_div(H, DT_H), nb = B * ntx * nty;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(detail_fwd_kernel, dim3(nb), dim3(DT_THREADS), 0, s, o, t, H, W, ntx, nty,
                     gauss5(), partial);
  hipLaunchKernelGGL(detail_finalize_kernel, dim3(1), dim3(DT_THREADS), 0, s, partial, nb,
                     (double)B * H * W, w_hf, w_pen, w_sob, base, out);
  NSM_LAUNCH_CHECK("detail_loss_fwd");
  return 0;
}

extern "C" int nsm_detail_loss_bwd(const float* o, const float* t, int B, int H, int W,
                                   float w_hf, float w_pen, float w_sob, const float* mcount,
                                   const float* gscale, float* grad, int accumulate,
                                   void* stream) {
  NSM_CHECK_ARG(o && t && grad, "detail_loss_bwd: null pointer");
  NSM_CHECK_ARG(mcount || w_pen == 0.f, "detail_loss_bwd: the penumbra term needs its count M");
  NSM_CHECK_ARG(detail_shape_ok(B, H, W), "detail_loss_bwd: shape %d x %d x %d", B, H, W);
  const int ntx = ceil_div(W, DT_W), nty = ceil_div(H, DT_H), nb = B * ntx * nty;
  hipLaunchKernelGGL(detail_bwd_kernel, dim3(nb), dim3(DT_THREADS), 0, as_stream(stream), o, t, H,
                     W, ntx, nty, gauss5(), (float)((double)B * H * W), w_hf, w_pen, w_sob, mcount,
                     gscale, grad, accumulate);
  NSM_LAUNCH_CHECK("detail_loss_bwd");
  return 0;
}
