// VGG19 perceptual-loss feature stack (customLoss.py:7-90), fp32 only: the
// element-wise passes of the forward and, below them, of its input-gradient
// chain ("Element-wise sources"). The kernels are at global scope.
#include "nsm_elem.h"

using namespace nsm;

// out[img][pixel][0..31]: channels 0-2 = (nan_to_num(clamp(v, 0, 1)) - mean) / denom
// (the 1-channel image repeated x3, customLoss.py:44-62), channels 3..31 = 0.
// Images 0..B-1 come from `a`, B..2B-1 from `b` (output and target batched).
__global__ void vgg_prep_kernel(const float* __restrict__ a, const float* __restrict__ b, int B,
                                long long HW, float mean, float denom, float* __restrict__ out) {
  long long total = 2ll * B * HW;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long half = (long long)B * HW;
    float v = i < half ? a[i] : b[i - half];
    // torch.clamp keeps NaN; nan_to_num(nan=0.5) then maps it (inf cannot survive the clamp)
    v = v != v ? 0.5f : fminf(fmaxf(v, 0.f), 1.f);
    const float n = (v - mean) / denom;
    f32x4* row = (f32x4*)(out + (size_t)i * 32);
    row[0] = f32x4{n, n, n, 0.f};
#pragma unroll
    for (int k = 1; k < 8; ++k) row[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// 2x2/2 max pool on NHWC (nn.MaxPool2d(2, 2), floor); NaN propagates as in ATen
__device__ __forceinline__ float nanmax(float m, float v) { return (v > m || v != v) ? v : m; }

__global__ void maxpool2_fwd_kernel(const float* __restrict__ x, int B, int H, int W, int C4,
                                    float* __restrict__ y) {
  const int Ho = H / 2, Wo = W / 2;
  long long total = (long long)B * Ho * Wo * C4;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    int c = (int)(i % C4);
    long long t = i / C4;
    int ox = (int)(t % Wo);
    t /= Wo;
    int oy = (int)(t % Ho);
    int b = (int)(t / Ho);
    const float* base = x + (((size_t)b * H + 2 * oy) * W + 2 * ox) * (C4 * 4) + c * 4;
    size_t rs = (size_t)W * C4 * 4, cs = (size_t)C4 * 4;
    f32x4 m = *(const f32x4*)base;
    const f32x4 v1 = *(const f32x4*)(base + cs), v2 = *(const f32x4*)(base + rs),
                v3 = *(const f32x4*)(base + rs + cs);
    m.x = nanmax(nanmax(nanmax(m.x, v1.x), v2.x), v3.x);
    m.y = nanmax(nanmax(nanmax(m.y, v1.y), v2.y), v3.y);
    m.z = nanmax(nanmax(nanmax(m.z, v1.z), v2.z), v3.z);
    m.w = nanmax(nanmax(nanmax(m.w, v1.w), v2.w), v3.w);
    *(f32x4*)(y + (size_t)i * 4) = m;
  }
}

extern "C" int nsm_vgg_prep(const float* output, const float* target, int B, int H, int W,
                            float mean, float denom, float* out, void* stream) {
  NSM_CHECK_ARG(output && target && out && B > 0 && H > 0 && W > 0, "vgg_prep: bad args");
  long long work = 2ll * B * H * W;
  hipLaunchKernelGGL(vgg_prep_kernel, dim3(grid_for(work)), dim3(256), 0, as_stream(stream), output,
                     target, B, (long long)H * W, mean, denom, out);
  NSM_LAUNCH_CHECK("vgg_prep");
  return 0;
}

extern "C" int nsm_maxpool2_fwd(const float* x, int B, int H, int W, int C, float* y,
                                void* stream) {
  NSM_CHECK_ARG(x && y && C % 4 == 0 && H >= 2 && W >= 2, "maxpool2_fwd: bad args");
  long long work = (long long)B * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2_fwd_kernel, dim3(grid_for(work)), dim3(256), 0, as_stream(stream), x,
                     B, H, W, C / 4, y);
  NSM_LAUNCH_CHECK("maxpool2_fwd");
  return 0;
}

// ---- backward of the stack (output half only; the weights are frozen) -------
// d(coef' * |y - t|)/dy with coef' = coef * gscale, the sign of nsm_l1_loss_bwd
__device__ __forceinline__ float tap_sign(float y, float t, float mag) {
  const float d = y - t;
  return d > 0.f ? mag : (d < 0.f ? -mag : 0.f);
}

__device__ __forceinline__ f32x4 tap_sign4(const f32x4 y, const f32x4 t, float mag) {
  return f32x4{tap_sign(y.x, t.x, mag), tap_sign(y.y, t.y, mag), tap_sign(y.z, t.z, mag),
               tap_sign(y.w, t.w, mag)};
}

// g = (relu ? (y > 0 ? g : 0) : g) + (t ? mag * sign(y - t) : 0), in place;
// overwrite: nothing arrives from above (the last tap), g is written only
__global__ void vgg_tap_relu_bwd_kernel(float* __restrict__ g, const float* __restrict__ y,
                                        const float* __restrict__ t, long long n4, float coef,
                                        const float* __restrict__ gscale, int relu,
                                        int overwrite) {
  const float mag = coef * (gscale ? gscale[0] : 1.f);
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const f32x4 yv = ((const f32x4*)y)[i];
    f32x4 gv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!overwrite) {
      gv = ((const f32x4*)g)[i];
      if (relu) {
        gv.x = yv.x > 0.f ? gv.x : 0.f;
        gv.y = yv.y > 0.f ? gv.y : 0.f;
        gv.z = yv.z > 0.f ? gv.z : 0.f;
        gv.w = yv.w > 0.f ? gv.w : 0.f;
      }
    }
    if (t) {
      const f32x4 s = tap_sign4(yv, ((const f32x4*)t)[i], mag);
      gv.x += s.x;
      gv.y += s.y;
      gv.z += s.z;
      gv.w += s.w;
    }
    ((f32x4*)g)[i] = gv;
  }
}

// MaxPool2d(2,2) backward behind the ReLU the forward moved past the pool: per
// channel the pooled gradient goes to the window's first maximum of the
// pre-ReLU y (the scan of nanmax / ATen: strict >, NaN wins) if that maximum
// is > 0; every input also gets its tap term. One thread: one pooled position
// x 4 channels, its 4 inputs, and the odd trailing column / row / corner next
// to it (no pooled gradient there), so each g_y element has one writer.
__global__ void maxpool2_bwd_kernel(const float* __restrict__ gp, const float* __restrict__ y,
                                    const float* __restrict__ t, int B, int H, int W, int C4,
                                    float coef, const float* __restrict__ gscale,
                                    float* __restrict__ gy) {
  const int Ho = H / 2, Wo = W / 2;
  const float mag = coef * (gscale ? gscale[0] : 1.f);
  const size_t rs = (size_t)W * C4 * 4, cs = (size_t)C4 * 4;
  long long total = (long long)B * Ho * Wo * C4;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    int c = (int)(i % C4);
    long long r = i / C4;
    int ox = (int)(r % Wo);
    r /= Wo;
    int oy = (int)(r % Ho);
    int b = (int)(r / Ho);
    const size_t base = (((size_t)b * H + 2 * oy) * W + 2 * ox) * (C4 * 4) + c * 4;
    const size_t off[4] = {base, base + cs, base + rs, base + rs + cs};
    const f32x4 g = *(const f32x4*)(gp + (size_t)i * 4);
    f32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = *(const f32x4*)(y + off[k]);
    f32x4 m = v[0];
    int ix = 0, iy = 0, iz = 0, iw = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      if (v[k].x > m.x || v[k].x != v[k].x) { m.x = v[k].x; ix = k; }
      if (v[k].y > m.y || v[k].y != v[k].y) { m.y = v[k].y; iy = k; }
      if (v[k].z > m.z || v[k].z != v[k].z) { m.z = v[k].z; iz = k; }
      if (v[k].w > m.w || v[k].w != v[k].w) { m.w = v[k].w; iw = k; }
    }
    const f32x4 gm = f32x4{m.x > 0.f ? g.x : 0.f, m.y > 0.f ? g.y : 0.f, m.z > 0.f ? g.z : 0.f,
                           m.w > 0.f ? g.w : 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f32x4 o = f32x4{ix == k ? gm.x : 0.f, iy == k ? gm.y : 0.f, iz == k ? gm.z : 0.f,
                      iw == k ? gm.w : 0.f};
      if (t) {
        const f32x4 s = tap_sign4(v[k], *(const f32x4*)(t + off[k]), mag);
        o.x += s.x;
        o.y += s.y;
        o.z += s.z;
        o.w += s.w;
      }
      *(f32x4*)(gy + off[k]) = o;
    }
    // the odd edge: column W-1 beside the last pooled column, row H-1 below
    // the last pooled row, and the corner where both are odd
    const bool ecol = (W & 1) && ox == Wo - 1, erow = (H & 1) && oy == Ho - 1;
    auto edge = [&](size_t e) {
      f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t) o = tap_sign4(*(const f32x4*)(y + e), *(const f32x4*)(t + e), mag);
      *(f32x4*)(gy + e) = o;
    };
    if (ecol) {
      edge(base + 2 * cs);
      edge(base + rs + 2 * cs);
    }
    if (erow) {
      edge(base + 2 * rs);
      edge(base + 2 * rs + cs);
    }
    if (ecol && erow) edge(base + 2 * rs + 2 * cs);
  }
}

// adjoint of nsm_vgg_prep for the output images: the three repeated channels'
// gradients summed, / denom, passed where 0 <= o <= 1 (clamp's backward keeps
// the bounds; NaN and out-of-range inputs get 0), times `scale`
__global__ void vgg_prep_bwd_kernel(const float* __restrict__ g32, const float* __restrict__ o,
                                    long long n, float denom, float scale, float* grad,
                                    int accumulate) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (long long)gridDim.x * blockDim.x) {
    const f32x4 g = *(const f32x4*)(g32 + (size_t)i * 32);
    const float v = o[i];
    float r = (v >= 0.f && v <= 1.f) ? (g.x + g.y + g.z) / denom * scale : 0.f;
    grad[i] = accumulate ? grad[i] + r : r;
  }
}

extern "C" int nsm_vgg_tap_relu_bwd(float* g, const float* y, const float* t, int64_t n,
                                    float coef, const float* gscale, int relu, int overwrite,
                                    void* stream) {
  NSM_CHECK_ARG(g && y && n > 0 && n % 4 == 0 && (t || !overwrite), "vgg_tap_relu_bwd: bad args");
  hipLaunchKernelGGL(vgg_tap_relu_bwd_kernel, dim3(grid_for(n / 4, 256, 2048)), dim3(256), 0,
                     as_stream(stream), g, y, t, (long long)(n / 4), coef, gscale, relu, overwrite);
  NSM_LAUNCH_CHECK("vgg_tap_relu_bwd");
  return 0;
}

extern "C" int nsm_maxpool2_bwd(const float* g_pooled, const float* y, const float* t, int B,
                                int H, int W, int C, float coef, const float* gscale, float* g_y,
                                void* stream) {
  NSM_CHECK_ARG(g_pooled && y && g_y && B > 0 && C > 0 && C % 4 == 0 && H >= 2 && W >= 2,
                "maxpool2_bwd: bad args");
  long long work = (long long)B * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3(grid_for(work, 256, 2048)), dim3(256), 0,
                     as_stream(stream), g_pooled, y, t, B, H, W, C / 4, coef, gscale, g_y);
  NSM_LAUNCH_CHECK("maxpool2_bwd");
  return 0;
}

extern "C" int nsm_vgg_prep_bwd(const float* g32, const float* output, int B, int H, int W,
                                float denom, float scale, float* grad, int accumulate,
                                void* stream) {
  NSM_CHECK_ARG(g32 && output && grad && B > 0 && H > 0 && W > 0 && denom != 0.f,
                "vgg_prep_bwd: bad args");
  long long n = (long long)B * H * W;
  hipLaunchKernelGGL(vgg_prep_bwd_kernel, dim3(grid_for(n, 256, 2048)), dim3(256), 0,
                     as_stream(stream), g32, output, n, denom, scale, grad, accumulate);
  NSM_LAUNCH_CHECK("vgg_prep_bwd");
  return 0;
}
