// Motion-vector reprojection shared by the temporal passes (nsm_temporal.hip:
// the instability metric, the reprojection op, the TAA resolve; nsm_svgf.hip:
// the SVGF temporal accumulation): the lookup, the bilinear sample and the
// position / depth / normal rejection tests, on the thread layout they share.
// The convention is in include/nsm.h (nsm_temporal_pair). Every includer gets
// the same inlined code, so a verdict and a sample have the same bits in every
// pass.
#pragma once
#include <math.h>
#include "nsm_common.h"

namespace nsm {

constexpr int TP_THREADS = 256, TP_VEC = 4;
constexpr int TP_PIX = TP_THREADS * TP_VEC;  // pixels of one block

// the four taps of one pixel: plane offsets i00, i00 + dx, i00 + dy, i00 + dy + dx
struct Taps {
  int i00, dx, dy;
  float w00, w01, w10, w11;
  bool ok;
};

// Lookup position of pixel (x, y) under motion (mvx, mvy): the position test in
// floating point, then the cell from floor, clamped so that px == W-1 is valid
// (cell W-2, weight 1 on its right tap). A rejected pixel gets the cell (0, 0).
__device__ __forceinline__ Taps reproject_taps(float mvx, float mvy, int x, int y, int H, int W,
                                               float scale_x, float scale_y) {
  Taps t;
  const float px = fmaf(mvx, scale_x, (float)x), py = fmaf(mvy, scale_y, (float)y);
  // NaN fails every comparison, +-Inf and 1e30 one of them
  t.ok = px >= 0.f && px <= (float)(W - 1) && py >= 0.f && py <= (float)(H - 1);
  const float cx = t.ok ? px : 0.f, cy = t.ok ? py : 0.f;
  const int x0 = max(min((int)floorf(cx), W - 2), 0), y0 = max(min((int)floorf(cy), H - 2), 0);
  const float fx = cx - (float)x0, fy = cy - (float)y0;
  const float gx = 1.f - fx, gy = 1.f - fy;
  t.i00 = y0 * W + x0;
  t.dx = W > 1 ? 1 : 0;
  t.dy = H > 1 ? W : 0;
  t.w00 = gy * gx;
  t.w01 = gy * fx;
  t.w10 = fy * gx;
  t.w11 = fy * fx;
  return t;
}

__device__ __forceinline__ float tap_sample(const float* __restrict__ plane, const Taps& t) {
  const float* p = plane + t.i00;
  return (t.w00 * p[0] + t.w01 * p[t.dx]) + (t.w10 * p[t.dy] + t.w11 * p[t.dy + t.dx]);
}

// plane pixel of slot j (< TP_VEC) of this thread in block blk of its image:
// a wave owns 64 * TP_VEC consecutive pixels, slot j of its lanes 64 consecutive
// ones of them
__device__ __forceinline__ uint32_t slot_pixel(uint32_t blk, int j) {
  return blk * TP_PIX + (threadIdx.x & ~63u) * TP_VEC + j * 64 + (threadIdx.x & 63u);
}

// the thread's TP_VEC values of a plane of HW floats (0 past its end)
__device__ __forceinline__ void ld_pix(const float* __restrict__ plane, uint32_t blk, uint32_t HW,
                                       float (&v)[TP_VEC]) {
#pragma unroll
  for (int j = 0; j < TP_VEC; ++j) {
    const uint32_t p = slot_pixel(blk, j);
    v[j] = p < HW ? plane[p] : 0.f;
  }
}

// the block's image b and block blk within it, and the taps of the thread's
// TP_VEC pixels (ok = false past the plane's end). mv == NULL: no motion.
__device__ __forceinline__ void thread_taps(const float* __restrict__ mv, int H, int W, FastDiv dw,
                                            int per, float scale_x, float scale_y, int& b,
                                            uint32_t& blk, Taps (&t)[TP_VEC]) {
  const uint32_t HW = (uint32_t)H * W;
  b = blockIdx.x / per;
  blk = blockIdx.x - b * per;
  float mx[TP_VEC] = {0.f, 0.f, 0.f, 0.f}, my[TP_VEC] = {0.f, 0.f, 0.f, 0.f};
  if (mv) {
    const float* m = mv + (size_t)b * 2 * HW;
    ld_pix(m, blk, HW, mx);
    ld_pix(m + HW, blk, HW, my);
  }
#pragma unroll
  for (int j = 0; j < TP_VEC; ++j) {
    const uint32_t p = slot_pixel(blk, j);
    if (p < HW) {
      const uint32_t y = fdiv(p, dw);
      t[j] = reproject_taps(mx[j], my[j], (int)(p - y * W), (int)y, H, W, scale_x, scale_y);
    } else {
      t[j] = Taps{0, 0, 0, 0.f, 0.f, 0.f, 0.f, false};
    }
  }
}

// The depth and normal tests of the thread's pixels (the metric, the TAA pass
// and the SVGF accumulation share them): zc/zp [B,1,H,W] and nc/np [B,3,H,W] of
// the current / previous frame, NULL in pairs; a failed test clears t[j].ok.
__device__ __forceinline__ void reject_taps(const float* __restrict__ zc,
                                            const float* __restrict__ zp,
                                            const float* __restrict__ nc,
                                            const float* __restrict__ np, int b, uint32_t blk,
                                            uint32_t HW, float depth_tol, float normal_cos,
                                            Taps (&t)[TP_VEC]) {
  float v[TP_VEC];
  if (zc) {
    ld_pix(zc + (size_t)b * HW, blk, HW, v);
    const float* zprev = zp + (size_t)b * HW;
#pragma unroll
    for (int j = 0; j < TP_VEC; ++j)
      t[j].ok = t[j].ok && fabsf(v[j] - tap_sample(zprev, t[j])) <= depth_tol * fabsf(v[j]);
  }
  if (nc) {
    float dot[TP_VEC] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 3; ++k) {
      ld_pix(nc + ((size_t)b * 3 + k) * HW, blk, HW, v);
      const float* nprev = np + ((size_t)b * 3 + k) * HW;
#pragma unroll
      for (int j = 0; j < TP_VEC; ++j)
        dot[j] = fmaf(v[j], tap_sample(nprev, t[j]), dot[j]);
    }
#pragma unroll
    for (int j = 0; j < TP_VEC; ++j)
      t[j].ok = t[j].ok && dot[j] >= normal_cos;
  }
}

// fp32 holds pixel coordinates exactly below 2^24; C*H*W < 2^31 keeps every
// plane offset in an int and every block count in an int
static inline bool temporal_shape_ok(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || H > (1 << 24) || W > (1 << 24)) return false;
  if ((long long)C * H * W >= (1ll << 31)) return false;
  return (long long)B * ceil_div((long long)H * W, TP_PIX) < (1ll << 31);
}

}  // namespace nsm
