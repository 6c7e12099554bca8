// The temporal-instability metric with motion-vector reprojection (the paper's
// Eq. 3; pert_loss.py:170-199 takes `motion_vectors` and leaves their branch as
// `pass`), the reprojection as an op of its own, and the temporal anti-aliasing
// resolve on the same lookup (taa_resolve_kernel below). Planar NCHW fp32.
//   D_t(p) = |I_t(p) - I_{t-1}(m(p))|,  E = mean(exp(alpha D) - 1)
//   m(p) = (x + mv[b,0,y,x] * scale_x, y + mv[b,1,y,x] * scale_y) in pixels,
//   integer coordinates are pixel centres (align_corners=True), bilinear.
// A pixel is rejected when m(p) is not finite or leaves [0, W-1] x [0, H-1]
// (tested in floating point, before any conversion to an integer; a rejected
// pixel's taps are clamped into the image), and optionally when the previous
// frame's interpolated depth or normal disagrees with the current one:
//   !(|z_t - z~| <= depth_tol |z_t|)   or   !(dot(n_t, n~) >= normal_cos)
// (n~ is not renormalised; a NaN on either side rejects).
// One thread works on TP_VEC pixels of one image plane: the taps and the four
// weights are computed once per pixel (reproject_taps, shared by both kernels)
// and reused for every channel, the depth and the normals. The lanes of a wave
// hold 64 consecutive pixels per slot, so a wave reads cur, mv, depth and
// normals as whole 256-byte runs and its gathers from the previous frame land
// on as few cache lines as the motion field allows (DESIGN.md has the measured
// comparison with four consecutive pixels per thread and 16-byte loads, which
// is 1.4 times slower: the gathers, 4 per plane and pixel, set the pace). The
// gathers are unconditional (a rejected pixel's taps are in the image), so the
// compiler issues them back to back. Surviving elements add exp(alpha D) - 1
// to an fp32 block sum and 1 to an integer block count; both go to a slab
// [B][blocks per image] per pair, and a single-block finalize sums the slabs
// of all pairs in a fixed order in double. No atomics: bitwise reproducible.
// The lookup, the sample, the rejection tests and the slot layout are in
// nsm_reproject.h, which the SVGF accumulation (nsm_svgf.hip) includes too.
#include <math.h>
#include "nsm_common.h"
#include "nsm_reproject.h"

namespace nsm {

// psum[blk], pcnt[blk]: the block's sum of exp(alpha D) - 1 over its surviving
// elements and their number. zc/zp (depth of the current / previous frame,
// [B,1,H,W]) and nc/np (normals, [B,3,H,W]) may be NULL in pairs.
__global__ void __launch_bounds__(TP_THREADS)
    temporal_pair_kernel(const float* __restrict__ cur, const float* __restrict__ prev,
                         const float* __restrict__ mv, const float* __restrict__ zc,
                         const float* __restrict__ zp, const float* __restrict__ nc,
                         const float* __restrict__ np, int C, int H, int W, FastDiv dw, int per,
                         float scale_x, float scale_y, float alpha, float depth_tol,
                         float normal_cos, float* __restrict__ psum, int* __restrict__ pcnt) {
  __shared__ float shs[TP_THREADS / 64];
  __shared__ int shc[TP_THREADS / 64];
  const uint32_t HW = (uint32_t)H * W;
  int b;
  uint32_t blk;
  Taps t[TP_VEC];
  thread_taps(mv, H, W, dw, per, scale_x, scale_y, b, blk, t);
  float s = 0.f;
  int cnt = 0;
  float v[TP_VEC];
  reject_taps(zc, zp, nc, np, b, blk, HW, depth_tol, normal_cos, t);
  for (int c = 0; c < C; ++c) {
    const size_t plane = ((size_t)b * C + c) * HW;
    ld_pix(cur + plane, blk, HW, v);
#pragma unroll
    for (int j = 0; j < TP_VEC; ++j)
      s += t[j].ok ? expf(alpha * fabsf(v[j] - tap_sample(prev + plane, t[j]))) - 1.f : 0.f;
  }
#pragma unroll
  for (int j = 0; j < TP_VEC; ++j) cnt += t[j].ok ? C : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    cnt += __shfl_xor(cnt, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    shs[threadIdx.x >> 6] = s;
    shc[threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = 0.f;
    int rc = 0;
    for (int w = 0; w < TP_THREADS / 64; ++w) {
      r += shs[w];
      rc += shc[w];
    }
    psum[blockIdx.x] = r;
    pcnt[blockIdx.x] = rc;
  }
}

// One block over the slabs of npairs pairs ([npairs][B][per]), pair after pair,
// image after image, every sum in double and in a fixed order:
//   sums[p*B + b], counts[p*B + b]: image b of pair p;
//   value of pair p = sum_b sums / (all_count > 0 ? all_count : sum_b counts),
//   0 when that divisor is 0; out[0] = mean of the pair values;
//   acc (may be NULL): acc[0] += sum of the pair values, acc[1] += npairs.
__global__ void __launch_bounds__(TP_THREADS)
    temporal_finalize_kernel(const float* __restrict__ psum, const int* __restrict__ pcnt,
                             int npairs, int B, int per, long long all_count,
                             float* __restrict__ sums, long long* __restrict__ counts,
                             float* __restrict__ out, double* acc) {
#pragma clang fp contract(off)
  __shared__ double shs[TP_THREADS / 64];
  __shared__ long long shc[TP_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double total = 0.0;
  for (int p = 0; p < npairs; ++p) {
    double ps = 0.0;
    long long pc = 0;
    for (int b = 0; b < B; ++b) {
      const size_t base = ((size_t)p * B + b) * per;
      double s = 0.0;
      long long c = 0;
      for (int i = threadIdx.x; i < per; i += TP_THREADS) {
        s += (double)psum[base + i];
        c += pcnt[base + i];
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        c += __shfl_xor(c, o, 64);
      }
      __syncthreads();  // the previous image's words have been read
      if (lane == 0) {
        shs[wave] = s;
        shc[wave] = c;
      }
      __syncthreads();
      s = 0.0;
      c = 0;
      for (int w = 0; w < TP_THREADS / 64; ++w) {
        s += shs[w];
        c += shc[w];
      }
      if (threadIdx.x == 0) {
        sums[(size_t)p * B + b] = (float)s;
        counts[(size_t)p * B + b] = c;
      }
      ps += s;
      pc += c;
    }
    const double den = all_count > 0 ? (double)all_count : (double)pc;
    total += den > 0.0 ? ps / den : 0.0;
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(total / (double)npairs);
    if (acc) {
      acc[0] += total;
      acc[1] += (double)npairs;
    }
  }
}

// out[b,c,y,x] = the bilinear sample of prev at m(p) (0 where rejected),
// valid[b,y,x] = 1 where m(p) lies inside the image
__global__ void __launch_bounds__(TP_THREADS)
    reproject_kernel(const float* __restrict__ prev, const float* __restrict__ mv, int C, int H,
                     int W, FastDiv dw, int per, float scale_x, float scale_y,
                     float* __restrict__ out, unsigned char* __restrict__ valid) {
  const uint32_t HW = (uint32_t)H * W;
  int b;
  uint32_t blk;
  Taps t[TP_VEC];
  thread_taps(mv, H, W, dw, per, scale_x, scale_y, b, blk, t);
  unsigned char* vb = valid + (size_t)b * HW;
#pragma unroll
  for (int j = 0; j < TP_VEC; ++j) {
    const uint32_t p = slot_pixel(blk, j);
    if (p < HW) vb[p] = t[j].ok ? 1 : 0;
  }
  for (int c = 0; c < C; ++c) {
    const size_t plane = ((size_t)b * C + c) * HW;
    float v[TP_VEC];
#pragma unroll
    for (int j = 0; j < TP_VEC; ++j) {
      const float q = tap_sample(prev + plane, t[j]);
      v[j] = t[j].ok ? q : 0.f;
    }
    float* o = out + plane;
#pragma unroll
    for (int j = 0; j < TP_VEC; ++j) {
      const uint32_t p = slot_pixel(blk, j);
      if (p < HW) o[p] = v[j];
    }
  }
}

// The temporal anti-aliasing resolve of one frame (the paper's "TAA (1 last
// frame)" baseline of Figure 6), same grid and slots as temporal_pair_kernel:
//   h = bilinear sample of hist (the previous RESOLVED frame) at m(p),
//   clamp: h = min(max(h, lo), hi), lo/hi = min/max of cur over the 3x3
//   neighbourhood of p, row and column indices clamped (edge replicate: the
//   neighbourhood never leaves the plane, whatever the block seam),
//   out = accepted ? fmaf(keep, h - cur, cur) : cur,  keep = 1 - blend,
// which is cur bit for bit when h == cur and when blend == 1. accepted (may be
// NULL) [B,1,H,W]: 1 where the history was used. The verdicts come from the
// previous INPUT frame's depth and normals (reject_taps), not from hist.
// The neighbourhood is eight more loads per pixel and channel, all of them on
// lines the wave's own row runs and its neighbours' bring into the cache (an
// LDS copy of the rows a block spans measured 1.2 to 1.9 times slower:
// DESIGN.md, "Temporal anti-aliasing pass").
__global__ void __launch_bounds__(TP_THREADS)
    taa_resolve_kernel(const float* __restrict__ cur, const float* __restrict__ hist,
                       const float* __restrict__ mv, const float* __restrict__ zc,
                       const float* __restrict__ zp, const float* __restrict__ nc,
                       const float* __restrict__ np, int C, int H, int W, FastDiv dw, int per,
                       float scale_x, float scale_y, float keep, int clamp, float depth_tol,
                       float normal_cos, float* __restrict__ out,
                       unsigned char* __restrict__ accepted) {
  const uint32_t HW = (uint32_t)H * W;
  int b;
  uint32_t blk;
  Taps t[TP_VEC];
  thread_taps(mv, H, W, dw, per, scale_x, scale_y, b, blk, t);
  reject_taps(zc, zp, nc, np, b, blk, HW, depth_tol, normal_cos, t);
  if (accepted) {
    unsigned char* ab = accepted + (size_t)b * HW;
#pragma unroll
    for (int j = 0; j < TP_VEC; ++j) {
      const uint32_t p = slot_pixel(blk, j);
      if (p < HW) ab[p] = t[j].ok ? 1 : 0;
    }
  }
  // plane offsets of the rows above, of and below each pixel and its columns
  // to the left and right (a slot past the plane's end uses the last pixel's)
  int r0[TP_VEC], r1[TP_VEC], r2[TP_VEC], xl[TP_VEC], xc[TP_VEC], xr[TP_VEC];
  if (clamp) {
#pragma unroll
    for (int j = 0; j < TP_VEC; ++j) {
      const uint32_t p = min(slot_pixel(blk, j), HW - 1);
      const int y = (int)fdiv(p, dw), x = (int)p - y * W;
      r0[j] = max(y - 1, 0) * W;
      r1[j] = y * W;
      r2[j] = min(y + 1, H - 1) * W;
      xl[j] = max(x - 1, 0);
      xc[j] = x;
      xr[j] = min(x + 1, W - 1);
    }
  }
  for (int c = 0; c < C; ++c) {
    const size_t plane = ((size_t)b * C + c) * HW;
    float v[TP_VEC], h[TP_VEC];
    ld_pix(cur + plane, blk, HW, v);
#pragma unroll
    for (int j = 0; j < TP_VEC; ++j) h[j] = tap_sample(hist + plane, t[j]);
    if (clamp) {
      const float* src = cur + plane;
#pragma unroll
      for (int j = 0; j < TP_VEC; ++j) {
        const float *a = src + r0[j], *m = src + r1[j], *z = src + r2[j];
        const float a0 = a[xl[j]], a1 = a[xc[j]], a2 = a[xr[j]];
        const float m0 = m[xl[j]], m2 = m[xr[j]];
        const float z0 = z[xl[j]], z1 = z[xc[j]], z2 = z[xr[j]];
        const float lo = fminf(fminf(fminf(a0, a1), fminf(a2, m0)),
                               fminf(fminf(m2, z0), fminf(fminf(z1, z2), v[j])));
        const float hi = fmaxf(fmaxf(fmaxf(a0, a1), fmaxf(a2, m0)),
                               fmaxf(fmaxf(m2, z0), fmaxf(fmaxf(z1, z2), v[j])));
        h[j] = fminf(fmaxf(h[j], lo), hi);
      }
    }
    float* o = out + plane;
#pragma unroll
    for (int j = 0; j < TP_VEC; ++j) {
      const uint32_t p = slot_pixel(blk, j);
      if (p < HW) o[p] = t[j].ok ? fmaf(keep, h[j] - v[j], v[j]) : v[j];
    }
  }
}

}  // namespace nsm

using namespace nsm;

extern "C" int nsm_temporal_blocks(int B, int C, int H, int W) {
  if (!temporal_shape_ok(B, C, H, W)) return 0;
  return ceil_div((long long)H * W, TP_PIX);
}

extern "C" int nsm_temporal_pair(const float* cur, const float* prev, const float* mv,
                                 const float* depth_cur, const float* depth_prev,
                                 const float* normal_cur, const float* normal_prev, int B, int C,
                                 int H, int W, float scale_x, float scale_y, float alpha,
                                 float depth_tol, float normal_cos, float* psum, int* pcnt,
                                 void* stream) {
  NSM_CHECK_ARG(cur && prev && psum && pcnt, "temporal_pair: null pointer");
  NSM_CHECK_ARG(!depth_cur == !depth_prev && !normal_cur == !normal_prev,
                "temporal_pair: depth and normals come for both frames of the pair or for none");
  NSM_CHECK_ARG(mv || (!depth_cur && !normal_cur),
                "temporal_pair: depth or normal rejection without motion vectors");
  NSM_CHECK_ARG(temporal_shape_ok(B, C, H, W), "temporal_pair: shape %d x %d x %d x %d", B, C, H, W);
  const int per = nsm_temporal_blocks(B, C, H, W);
  hipLaunchKernelGGL(temporal_pair_kernel, dim3(B * per), dim3(TP_THREADS), 0, as_stream(stream),
                     cur, prev, mv, depth_cur, depth_prev, normal_cur, normal_prev, C, H, W,
                     make_fastdiv((uint32_t)W), per, scale_x, scale_y, alpha, depth_tol, normal_cos,
                     psum, pcnt);
  NSM_LAUNCH_CHECK("temporal_pair");
  return 0;
}

extern "C" int nsm_temporal_finalize(const float* psum, const int* pcnt, int npairs, int B, int per,
                                     int64_t all_count, float* sums, int64_t* counts, float* out,
                                     double* acc, void* stream) {
  NSM_CHECK_ARG(psum && pcnt && sums && counts && out, "temporal_finalize: null pointer");
  NSM_CHECK_ARG(npairs > 0 && B > 0 && per > 0 && all_count >= 0,
                "temporal_finalize: %d pairs x %d images x %d blocks, all_count %lld", npairs, B,
                per, (long long)all_count);
  hipLaunchKernelGGL(temporal_finalize_kernel, dim3(1), dim3(TP_THREADS), 0, as_stream(stream),
                     psum, pcnt, npairs, B, per, (long long)all_count, sums, (long long*)counts, out,
                     acc);
  NSM_LAUNCH_CHECK("temporal_finalize");
  return 0;
}

extern "C" int nsm_taa_resolve(const float* cur, const float* hist, const float* mv,
                               const float* depth_cur, const float* depth_prev,
                               const float* normal_cur, const float* normal_prev, int B, int C,
                               int H, int W, float scale_x, float scale_y, float blend, int clamp,
                               float depth_tol, float normal_cos, float* out,
                               unsigned char* accepted, void* stream) {
  NSM_CHECK_ARG(cur && hist && out, "taa_resolve: null pointer");
  NSM_CHECK_ARG(out != hist && out != cur,
                "taa_resolve: out is %s (other threads gather from it)",
                out == hist ? "hist" : "cur");
  NSM_CHECK_ARG(blend > 0.f && blend <= 1.f, "taa_resolve: blend %g is not in (0, 1]",
                (double)blend);
  NSM_CHECK_ARG(!depth_cur == !depth_prev && !normal_cur == !normal_prev,
                "taa_resolve: depth and normals come for both frames or for none");
  NSM_CHECK_ARG(mv || (!depth_cur && !normal_cur),
                "taa_resolve: depth or normal rejection without motion vectors");
  NSM_CHECK_ARG(temporal_shape_ok(B, C, H, W), "taa_resolve: shape %d x %d x %d x %d", B, C, H, W);
  const int per = nsm_temporal_blocks(B, C, H, W);
  hipLaunchKernelGGL(taa_resolve_kernel, dim3(B * per), dim3(TP_THREADS), 0, as_stream(stream), cur,
                     hist, mv, depth_cur, depth_prev, normal_cur, normal_prev, C, H, W,
                     make_fastdiv((uint32_t)W), per, scale_x, scale_y, 1.f - blend, clamp,
                     depth_tol, normal_cos, out, accepted);
  NSM_LAUNCH_CHECK("taa_resolve");
  return 0;
}

extern "C" int nsm_reproject(const float* prev, const float* mv, int B, int C, int H, int W,
                             float scale_x, float scale_y, float* out, unsigned char* valid,
                             void* stream) {
  NSM_CHECK_ARG(prev && mv && out && valid, "reproject: null pointer");
  NSM_CHECK_ARG(temporal_shape_ok(B, C, H, W), "reproject: shape %d x %d x %d x %d", B, C, H, W);
  const int per = nsm_temporal_blocks(B, C, H, W);
  hipLaunchKernelGGL(reproject_kernel, dim3(B * per), dim3(TP_THREADS), 0, as_stream(stream), prev,
                     mv, C, H, W, make_fastdiv((uint32_t)W), per, scale_x, scale_y, out, valid);
  NSM_LAUNCH_CHECK("reproject");
  return 0;
}
