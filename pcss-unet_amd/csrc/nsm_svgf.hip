// Spatiotemporal variance-guided filtering (SVGF, Schied et al. 2017): the
// post-process denoiser of the paper's ray-tracing baseline (§4, Figure 9:
// "5-SPP raytracing with SVGF"), whose spatial half, the edge-avoiding a-trous
// wavelet filter, is also the depth-aware post filter of the PCSS baseline.
// Planar NCHW fp32, C = 1 (shadow visibility) or 3; include/nsm.h has the
// definition. Three kernels, no atomics, no allocation, no synchronisation:
//   svgf_accumulate_kernel: temporal accumulation of colour and of the first two
//     luminance moments on the lookup and the rejection tests of the TAA pass
//     (nsm_reproject.h, the same device functions and thread layout);
//   svgf_variance_kernel: the 7x7 spatial estimate for pixels with a short history;
//   svgf_atrous_kernel: one iteration of the 5x5 a-trous filter at step s.
// The two spatial kernels put one thread on one pixel and one wave on 64
// consecutive pixels of one row (a block is a 64 x 4 tile), so that every tap
// of a wave, at any step, is one 256-byte run of each plane it reads; an
// out-of-image tap is skipped, never clamped and never read.
// The depth and normal weights of a tap are folded into one exponential,
//   h(dx) h(dy) exp(-e_z - |l_p - l_q| / phi_l) max(0, n_p . n_q)^sigma_n
//     = h(dx) h(dy) exp(sigma_n log max(0, n_p . n_q) - e_z - |l_p - l_q| / phi_l),
// one expf and one logf per tap where powf alone is several times that; a
// non-positive dot product gives log = -inf and the weight 0, and sigma_n = 0
// drops the term (x^0 = 1 for every x). Contraction is off in this unit: every
// product is rounded as an ATen evaluation of the definition rounds it, and
// the two blends the definition writes as fma are fmaf calls.
#include <math.h>
#include "nsm_common.h"
#include "nsm_reproject.h"

#pragma clang fp contract(off)

namespace nsm {

constexpr int SV_TW = 64, SV_TH = 4;  // the tile of a block of the spatial kernels
constexpr int SV_THREADS = SV_TW * SV_TH;
constexpr int SV_MAX_STEP = 1 << 20;  // 2 * step + x stays far inside an int

template <int C>
__device__ __forceinline__ float luminance(const float (&c)[C]) {
  if constexpr (C == 1) {
    return c[0];
  } else {
    return 0.2126f * c[0] + 0.7152f * c[1] + 0.0722f * c[2];
  }
}

// what the edge weights need of the centre pixel: depth, normal, depth gradient
struct Guide {
  float z, nx, ny, nz, gx, gy;
};

// central differences of z with replicated edges, 0 along an axis of length 1
__device__ __forceinline__ Guide load_guide(const float* __restrict__ z,
                                            const float* __restrict__ n, size_t HW, int x, int y,
                                            int H, int W) {
  Guide g;
  const int p = y * W + x;
  const int xm = max(x - 1, 0), xp = min(x + 1, W - 1), ym = max(y - 1, 0), yp = min(y + 1, H - 1);
  g.z = z[p];
  g.nx = n[p];
  g.ny = n[HW + p];
  g.nz = n[2 * HW + p];
  g.gx = xp > xm ? (z[y * W + xp] - z[y * W + xm]) / (float)(xp - xm) : 0.f;
  g.gy = yp > ym ? (z[yp * W + x] - z[ym * W + x]) / (float)(yp - ym) : 0.f;
  return g;
}

// log(w_n) - e_z of the tap at plane offset q, (ox, oy) pixels from the centre
__device__ __forceinline__ float edge_exponent(const Guide& g, const float* __restrict__ z,
                                               const float* __restrict__ n, size_t HW, int q,
                                               float ox, float oy, float sigma_z, float sigma_n) {
  const float ez = fabsf(g.z - z[q]) / (sigma_z * fabsf(g.gx * ox + g.gy * oy) + 1e-8f);
  const float d = fmaxf(g.nx * n[q] + g.ny * n[HW + q] + g.nz * n[2 * HW + q], 0.f);
  const float ln = sigma_n != 0.f ? sigma_n * logf(d) : 0.f;
  return ln - ez;
}

// image b and pixel (x, y) of this thread; false past the image's right or lower edge
__device__ __forceinline__ bool tile_pixel(int H, int W, int tx, FastDiv dtx, FastDiv dper, int& b,
                                           int& x, int& y) {
  b = (int)fdiv(blockIdx.x, dper);
  const uint32_t r = blockIdx.x - (uint32_t)b * dper.d;
  const uint32_t ty = fdiv(r, dtx);
  x = (int)(r - ty * tx) * SV_TW + (int)(threadIdx.x & 63u);
  y = (int)ty * SV_TH + (int)(threadIdx.x >> 6);
  return x < W && y < H;
}

// ---- (a) temporal accumulation ----------------------------------------------
// Grid and slots of taa_resolve_kernel. hc == NULL: a first frame (no history).
template <int C>
__global__ void __launch_bounds__(TP_THREADS)
    svgf_accumulate_kernel(const float* __restrict__ cur, const float* __restrict__ zc,
                           const float* __restrict__ nc, const float* __restrict__ zp,
                           const float* __restrict__ np, const float* __restrict__ mv,
                           const float* __restrict__ hc, const float* __restrict__ hm,
                           const float* __restrict__ hn, int H, int W, FastDiv dw, int per,
                           float scale_x, float scale_y, float alpha, float moments_alpha,
                           float max_history, float depth_tol, float normal_cos,
                           float* __restrict__ oc, float* __restrict__ om, float* __restrict__ on,
                           float* __restrict__ ov, unsigned char* __restrict__ accepted) {
  const uint32_t HW = (uint32_t)H * W;
  int b;
  uint32_t blk;
  Taps t[TP_VEC];
  thread_taps(mv, H, W, dw, per, scale_x, scale_y, b, blk, t);
  if (hc) {
    if (mv) reject_taps(zc, zp, nc, np, b, blk, HW, depth_tol, normal_cos, t);
  } else {
#pragma unroll
    for (int j = 0; j < TP_VEC; ++j) t[j].ok = false;
  }
  // the history length at the nearest tap, and the two blend weights
  float mx[TP_VEC] = {0.f, 0.f, 0.f, 0.f}, my[TP_VEC] = {0.f, 0.f, 0.f, 0.f};
  if (mv && hc) {
    const float* m = mv + (size_t)b * 2 * HW;
    ld_pix(m, blk, HW, mx);
    ld_pix(m + HW, blk, HW, my);
  }
  float len[TP_VEC], keep[TP_VEC], keep_m[TP_VEC];
#pragma unroll
  for (int j = 0; j < TP_VEC; ++j) {
    float N = 1.f;
    if (t[j].ok) {  // the pixel is in the plane, its position in the image, hn is there
      const uint32_t p = slot_pixel(blk, j);
      const uint32_t y = fdiv(p, dw);
      const float px = fmaf(mx[j], scale_x, (float)(p - y * W)), py = fmaf(my[j], scale_y, (float)y);
      const int ix = max(min((int)floorf(px + 0.5f), W - 1), 0);
      const int iy = max(min((int)floorf(py + 0.5f), H - 1), 0);
      N = fminf(hn[(size_t)b * HW + (size_t)iy * W + ix] + 1.f, max_history);
    }
    const float inv = 1.f / N;
    len[j] = N;
    keep[j] = 1.f - fmaxf(alpha, inv);
    keep_m[j] = 1.f - fmaxf(moments_alpha, inv);
  }
  float v[C][TP_VEC];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const size_t plane = ((size_t)b * C + c) * HW;
    ld_pix(cur + plane, blk, HW, v[c]);
    float* o = oc + plane;
#pragma unroll
    for (int j = 0; j < TP_VEC; ++j) {
      const uint32_t p = slot_pixel(blk, j);
      float r = v[c][j];
      if (t[j].ok) r = fmaf(keep[j], tap_sample(hc + plane, t[j]) - r, r);
      if (p < HW) o[p] = r;
    }
  }
  const size_t mom = (size_t)b * 2 * HW, one = (size_t)b * HW;
#pragma unroll
  for (int j = 0; j < TP_VEC; ++j) {
    const uint32_t p = slot_pixel(blk, j);
    float cj[C];
#pragma unroll
    for (int c = 0; c < C; ++c) cj[c] = v[c][j];
    const float l = luminance<C>(cj);
    float m1 = l, m2 = l * l;
    if (t[j].ok) {
      m1 = fmaf(keep_m[j], tap_sample(hm + mom, t[j]) - m1, m1);
      m2 = fmaf(keep_m[j], tap_sample(hm + mom + HW, t[j]) - m2, m2);
    }
    if (p < HW) {
      om[mom + p] = m1;
      om[mom + HW + p] = m2;
      on[one + p] = len[j];
      ov[one + p] = fmaxf(0.f, m2 - m1 * m1);
      if (accepted) accepted[one + p] = t[j].ok ? 1 : 0;
    }
  }
}

// ---- (b) spatial variance fallback ------------------------------------------
template <int C>
__global__ void __launch_bounds__(SV_THREADS)
    svgf_variance_kernel(const float* __restrict__ color, const float* __restrict__ mom,
                         const float* __restrict__ hn, const float* __restrict__ var,
                         const float* __restrict__ z, const float* __restrict__ n, int H, int W,
                         int tx, FastDiv dtx, FastDiv dper, float min_history, float sigma_z,
                         float sigma_n, float* __restrict__ oc, float* __restrict__ ov) {
  int b, x, y;
  if (!tile_pixel(H, W, tx, dtx, dper, b, x, y)) return;
  const size_t HW = (size_t)H * W;
  const int p = y * W + x;
  const float* cb = color + (size_t)b * C * HW;
  float* ob = oc + (size_t)b * C * HW;
  const float N = hn[(size_t)b * HW + p];
  if (!(N < min_history)) {
#pragma unroll
    for (int c = 0; c < C; ++c) ob[c * HW + p] = cb[c * HW + p];
    ov[(size_t)b * HW + p] = var[(size_t)b * HW + p];
    return;
  }
  const float* zb = z + (size_t)b * HW;
  const float* nb = n + (size_t)b * 3 * HW;
  const float* mb = mom + (size_t)b * 2 * HW;
  const Guide g = load_guide(zb, nb, HW, x, y, H, W);
  float sw = 1.f, s1 = mb[p], s2 = mb[HW + p], sc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) sc[c] = cb[c * HW + p];
  for (int dy = -3; dy <= 3; ++dy) {
    const int qy = y + dy;
    if (qy < 0 || qy >= H) continue;
#pragma unroll
    for (int dx = -3; dx <= 3; ++dx) {
      const int qx = x + dx;
      if ((dx == 0 && dy == 0) || qx < 0 || qx >= W) continue;
      const int q = qy * W + qx;
      const float w = expf(edge_exponent(g, zb, nb, HW, q, (float)dx, (float)dy, sigma_z, sigma_n));
      sw += w;
      s1 += w * mb[q];
      s2 += w * mb[HW + q];
#pragma unroll
      for (int c = 0; c < C; ++c) sc[c] += w * cb[c * HW + q];
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) ob[c * HW + p] = sc[c] / sw;
  const float M1 = s1 / sw, M2 = s2 / sw;
  ov[(size_t)b * HW + p] = fmaxf(0.f, M2 - M1 * M1) * (min_history / N);
}

// ---- (c) one a-trous iteration ----------------------------------------------
// LUM: the luminance term and the variance output (var and ov are not touched
// without it).
template <int C, bool LUM>
__global__ void __launch_bounds__(SV_THREADS)
    svgf_atrous_kernel(const float* __restrict__ color, const float* __restrict__ var,
                       const float* __restrict__ z, const float* __restrict__ n, int H, int W,
                       int tx, FastDiv dtx, FastDiv dper, int step, float sigma_z, float sigma_n,
                       float sigma_l, float* __restrict__ oc, float* __restrict__ ov) {
  int b, x, y;
  if (!tile_pixel(H, W, tx, dtx, dper, b, x, y)) return;
  const size_t HW = (size_t)H * W;
  const int p = y * W + x;
  const float* cb = color + (size_t)b * C * HW;
  const float* zb = z + (size_t)b * HW;
  const float* nb = n + (size_t)b * 3 * HW;
  const float* vb = LUM ? var + (size_t)b * HW : nullptr;
  const Guide g = load_guide(zb, nb, HW, x, y, H, W);
  float cp[C];
#pragma unroll
  for (int c = 0; c < C; ++c) cp[c] = cb[c * HW + p];
  const float lp = luminance<C>(cp);
  float inv_phi = 0.f;
  if constexpr (LUM) {
    // the 3x3 Gaussian of the variance, edges replicated
    const int xm = max(x - 1, 0), xp = min(x + 1, W - 1);
    const int r0 = max(y - 1, 0) * W, r1 = y * W, r2 = min(y + 1, H - 1) * W;
    const float corner = (vb[r0 + xm] + vb[r0 + xp]) + (vb[r2 + xm] + vb[r2 + xp]);
    const float edge = (vb[r0 + x] + vb[r2 + x]) + (vb[r1 + xm] + vb[r1 + xp]);
    const float gv = 0.25f * vb[p] + 0.125f * edge + 0.0625f * corner;
    inv_phi = 1.f / (sigma_l * sqrtf(fmaxf(gv, 0.f) + 1e-10f));
  }
  constexpr float H5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  constexpr float W0 = 0.375f * 0.375f;
  float sw = W0, sv = 0.f, sc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) sc[c] = W0 * cp[c];
  if constexpr (LUM) sv = (W0 * W0) * vb[p];
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      if (dx == 0 && dy == 0) continue;
      const int qx = x + dx * step, qy = y + dy * step;
      if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
      const int q = qy * W + qx;
      float cq[C];
#pragma unroll
      for (int c = 0; c < C; ++c) cq[c] = cb[c * HW + q];
      float e = edge_exponent(g, zb, nb, HW, q, (float)(dx * step), (float)(dy * step), sigma_z,
                              sigma_n);
      if constexpr (LUM) e -= fabsf(lp - luminance<C>(cq)) * inv_phi;
      const float w = (H5[dx + 2] * H5[dy + 2]) * expf(e);
      sw += w;
#pragma unroll
      for (int c = 0; c < C; ++c) sc[c] += w * cq[c];
      if constexpr (LUM) sv += (w * w) * vb[q];
    }
  }
  float* ob = oc + (size_t)b * C * HW;
#pragma unroll
  for (int c = 0; c < C; ++c) ob[c * HW + p] = sc[c] / sw;
  if constexpr (LUM) ov[(size_t)b * HW + p] = sv / (sw * sw);
}

// tiles of one image (0: unsupported shape)
static int svgf_tiles(int B, int C, int H, int W) {
  if ((C != 1 && C != 3) || !temporal_shape_ok(B, C, H, W)) return 0;
  const long long per = (long long)ceil_div(W, SV_TW) * ceil_div(H, SV_TH);
  return per * B < (1ll << 31) ? (int)per : 0;
}

}  // namespace nsm

using namespace nsm;

extern "C" int nsm_svgf_blocks(int B, int C, int H, int W) { return svgf_tiles(B, C, H, W); }

extern "C" int nsm_svgf_accumulate(const float* cur, const float* depth_cur,
                                   const float* normal_cur, const float* depth_prev,
                                   const float* normal_prev, const float* mv,
                                   const float* hist_color, const float* hist_moments,
                                   const float* hist_len, int B, int C, int H, int W,
                                   float scale_x, float scale_y, float alpha, float moments_alpha,
                                   int max_history, float depth_tol, float normal_cos,
                                   float* out_color, float* out_moments, float* out_len,
                                   float* out_var, unsigned char* accepted, void* stream) {
  NSM_CHECK_ARG(cur && out_color && out_moments && out_len && out_var,
                "svgf_accumulate: null pointer");
  NSM_CHECK_ARG(!hist_color == !hist_moments && !hist_color == !hist_len,
                "svgf_accumulate: the history colour, moments and length come together or not at "
                "all (a first frame)");
  NSM_CHECK_ARG(!(mv && hist_color) || (depth_cur && normal_cur && depth_prev && normal_prev),
                "svgf_accumulate: motion vectors need both frames' depth and normals");
  NSM_CHECK_ARG(out_color != hist_color && out_moments != hist_moments && out_len != hist_len,
                "svgf_accumulate: an output is its own history (other threads gather from it)");
  NSM_CHECK_ARG(alpha > 0.f && alpha <= 1.f && moments_alpha > 0.f && moments_alpha <= 1.f,
                "svgf_accumulate: alpha %g / moments_alpha %g is not in (0, 1]", (double)alpha,
                (double)moments_alpha);
  NSM_CHECK_ARG(max_history >= 1 && max_history <= (1 << 24),
                "svgf_accumulate: max_history %d is not in [1, 2^24]", max_history);
  NSM_CHECK_ARG(svgf_tiles(B, C, H, W) > 0, "svgf_accumulate: shape %d x %d x %d x %d", B, C, H, W);
  const int per = ceil_div((long long)H * W, TP_PIX);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(B * per), dim3(TP_THREADS), 0, as_stream(stream), cur,
                       depth_cur, normal_cur, depth_prev, normal_prev, mv, hist_color, hist_moments,
                       hist_len, H, W, make_fastdiv((uint32_t)W), per, scale_x, scale_y, alpha,
                       moments_alpha, (float)max_history, depth_tol, normal_cos, out_color,
                       out_moments, out_len, out_var, accepted);
  };
  if (C == 1)
    launch(svgf_accumulate_kernel<1>);
  else
    launch(svgf_accumulate_kernel<3>);
  NSM_LAUNCH_CHECK("svgf_accumulate");
  return 0;
}

extern "C" int nsm_svgf_variance(const float* color, const float* moments, const float* hist_len,
                                 const float* var, const float* depth, const float* normals, int B,
                                 int C, int H, int W, int min_history, float sigma_z,
                                 float sigma_n, float* out_color, float* out_var, void* stream) {
  NSM_CHECK_ARG(color && moments && hist_len && var && depth && normals && out_color && out_var,
                "svgf_variance: null pointer");
  NSM_CHECK_ARG(out_color != color && out_var != var,
                "svgf_variance: an output is its input (other threads gather from it)");
  NSM_CHECK_ARG(min_history >= 0 && min_history <= (1 << 24),
                "svgf_variance: min_history %d is not in [0, 2^24]", min_history);
  const int per = svgf_tiles(B, C, H, W);
  NSM_CHECK_ARG(per > 0, "svgf_variance: shape %d x %d x %d x %d", B, C, H, W);
  const int tx = ceil_div(W, SV_TW);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(B * per), dim3(SV_THREADS), 0, as_stream(stream), color,
                       moments, hist_len, var, depth, normals, H, W, tx, make_fastdiv((uint32_t)tx),
                       make_fastdiv((uint32_t)per), (float)min_history, sigma_z, sigma_n, out_color,
                       out_var);
  };
  if (C == 1)
    launch(svgf_variance_kernel<1>);
  else
    launch(svgf_variance_kernel<3>);
  NSM_LAUNCH_CHECK("svgf_variance");
  return 0;
}

extern "C" int nsm_svgf_atrous(const float* color, const float* var, const float* depth,
                               const float* normals, int B, int C, int H, int W, int step,
                               float sigma_z, float sigma_n, float sigma_l, float* out_color,
                               float* out_var, void* stream) {
  NSM_CHECK_ARG(color && depth && normals && out_color, "svgf_atrous: null pointer");
  const bool lum = var && sigma_l != 0.f;
  NSM_CHECK_ARG(!lum || out_var, "svgf_atrous: a variance comes in and none can go out");
  NSM_CHECK_ARG(out_color != color && (!lum || out_var != var),
                "svgf_atrous: an output is its input (other threads gather from it)");
  NSM_CHECK_ARG(step >= 1 && step <= SV_MAX_STEP, "svgf_atrous: step %d is not in [1, 2^20]", step);
  const int per = svgf_tiles(B, C, H, W);
  NSM_CHECK_ARG(per > 0, "svgf_atrous: shape %d x %d x %d x %d", B, C, H, W);
  const int tx = ceil_div(W, SV_TW);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(B * per), dim3(SV_THREADS), 0, as_stream(stream), color, var,
                       depth, normals, H, W, tx, make_fastdiv((uint32_t)tx),
                       make_fastdiv((uint32_t)per), step, sigma_z, sigma_n, sigma_l, out_color,
                       out_var);
  };
  if (C == 1) {
    if (lum)
      launch(svgf_atrous_kernel<1, true>);
    else
      launch(svgf_atrous_kernel<1, false>);
  } else {
    if (lum)
      launch(svgf_atrous_kernel<3, true>);
    else
      launch(svgf_atrous_kernel<3, false>);
  }
  NSM_LAUNCH_CHECK("svgf_atrous");
  return 0;
}
