// The element-wise kernels at the model's edges ("Element-wise
// sources"): pixel (un)shuffle + layout change at the input and its gradient,
// the conv10 + pixel_shuffle + sigmoid head, the L1 / exp-difference /
// channel-std / perturbation / frame-normalisation passes of the losses, and
// the stand-alone optimizer pieces (gradient norm, clip coefficient, the
// AdamW / Adam / SGD steps; the fused step tail is nsm_tail.hip).
// Activations are NHWC in the storage type of the call (fp32, bf16 or f16),
// 8 channels per lane; cross-block sums are deterministic (per-block
// partials merged in a fixed order, in double).
#include "nsm_elem.h"

namespace nsm {

// ---------------------------------------------------------------------------
// Model boundary: pixel_unshuffle(2) + NCHW->NHWC (+ zero channel pad), and its
// inverse for the input gradient.
// ---------------------------------------------------------------------------
// thread per output pixel: each group of 8 output channels = 2 input planes x
// 2 rows x 2 columns (channel 4c + 2i + j, F.pixel_unshuffle), read as float2
// pairs coalesced along x and written as one 16-B (bf16) / 32-B (fp32) vector
// H2: out is an h2 tensor [npix][2 cp] scaled from the slot `amax` holds
// (max|x|, filled beforehand), T = bf16_t (16-bit storage)
template <typename T, bool H2 = false>
__global__ void __launch_bounds__(256) input_prep_kernel(const float* __restrict__ x, int B, int C,
                                                         int H, int W, T* __restrict__ out, int cp,
                                                         uint32_t npix, FastDiv fdRw, FastDiv fdRh,
                                                         uint32_t* __restrict__ amax) {
  const int Rh = H / 2, Rw = W / 2;
  const size_t plane = (size_t)H * W;
  float hs = 0.f;
  if constexpr (H2) hs = exp2i(h2_exp(H2Scale{amax, 1.f}));
  uint32_t am = 0;  // max|out| (conv2's f16x2 operand scale)
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < npix; p += gridDim.x * 256u) {
    const uint32_t t = fdiv(p, fdRw);
    const int rx = (int)(p - t * (uint32_t)Rw);
    const uint32_t b = fdiv(t, fdRh);
    const int ry = (int)(t - b * (uint32_t)Rh);
    const float* src = x + (size_t)b * C * plane + (size_t)(2 * ry) * W + 2 * rx;
    for (int g = 0; g < cp / 8; ++g) {
      f32x2 r[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {  // plane 2g + (q >> 1), row 2ry + (q & 1)
        const int c = 2 * g + (q >> 1);
        r[q] = c < C ? *(const f32x2*)(src + (size_t)c * plane + (q & 1) * W) : f32x2{0.f, 0.f};
      }
      const F8 v{f32x4{r[0].x, r[0].y, r[1].x, r[1].y}, f32x4{r[2].x, r[2].y, r[3].x, r[3].y}};
      if constexpr (H2) {
        h2_store8((bf16_t*)out + (size_t)p * 2 * cp, 8 * g, v, hs);
      } else {
        st8(out + (size_t)p * cp + 8 * g, v);
        if (amax) {
          amax_fold(am, v.a);
          amax_fold(am, v.b);
        }
      }
    }
  }
  if constexpr (!H2) amax_flush(am, amax);
}

template <typename T>
__global__ void input_grad_kernel(const T* __restrict__ dX, int B, int C, int H, int W, int cp,
                                  float* __restrict__ dx) {
  // thread per (b, c, ry, rx): one float4 of dX (channels 4c..4c+3 of pixel
  // (ry,rx)) -> the 2x2 block of plane c; rx fastest so stores coalesce.
  const int Rh = H / 2, Rw = W / 2;
  long long total = (long long)B * C * Rh * Rw;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    int rx = (int)(i % Rw);
    long long t = i / Rw;
    int ry = (int)(t % Rh);
    t /= Rh;
    int c = (int)(t % C);
    int b = (int)(t / C);
    f32x4 v = ld4(dX + (((size_t)b * Rh + ry) * Rw + rx) * cp + 4 * c);
    float* o = dx + (((size_t)b * C + c) * H + 2 * ry) * W + 2 * rx;
    *(f32x2*)o = f32x2{v.x, v.y};
    *(f32x2*)(o + W) = f32x2{v.z, v.w};
  }
}

// ---------------------------------------------------------------------------
// Head: conv10 (1x1, 16->4, bias) -> pixel_shuffle(2) -> sigmoid
// ---------------------------------------------------------------------------
template <typename T>
__global__ void head_fwd_kernel(const T* __restrict__ z, int ldz, int B, int Rh, int Rw,
                                const float* __restrict__ w10, const float* __restrict__ b10,
                                float* __restrict__ out) {
  __shared__ float w[68];
  if (threadIdx.x < 64) w[threadIdx.x] = w10[threadIdx.x];
  if (threadIdx.x < 4) w[64 + threadIdx.x] = b10[threadIdx.x];
  __syncthreads();
  long long npix = (long long)B * Rh * Rw;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix;
       p += (long long)gridDim.x * blockDim.x) {
    float zz[16];
    const T* zr = z + (size_t)p * ldz;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 v = ld4(zr + 4 * q);
      zz[4 * q] = v.x;
      zz[4 * q + 1] = v.y;
      zz[4 * q + 2] = v.z;
      zz[4 * q + 3] = v.w;
    }
    int rx = (int)(p % Rw);
    long long t = p / Rw;
    int ry = (int)(t % Rh);
    int b = (int)(t / Rh);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < 16; ++c) acc += w[j * 16 + c] * zz[c];
      acc += w[64 + j];
      float s = 1.f / (1.f + expf(-acc));
      int di = j >> 1, dj = j & 1;
      out[((size_t)b * 2 * Rh + 2 * ry + di) * (2 * Rw) + 2 * rx + dj] = s;
    }
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T>
__global__ void __launch_bounds__(256) head_bwd_kernel(
    const float* __restrict__ gout, const float* __restrict__ out, const T* __restrict__ z,
    int ldz, int B, int Rh, int Rw, const float* __restrict__ w10, T* __restrict__ dz,
    float* __restrict__ partial) {
  __shared__ float w[64];
  __shared__ float red[4][68];
  if (threadIdx.x < 64) w[threadIdx.x] = w10[threadIdx.x];
  __syncthreads();
  float accw[68];
#pragma unroll
  for (int k = 0; k < 68; ++k) accw[k] = 0.f;
  long long npix = (long long)B * Rh * Rw;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix;
       p += (long long)gridDim.x * blockDim.x) {
    int rx = (int)(p % Rw);
    long long t = p / Rw;
    int ry = (int)(t % Rh);
    int b = (int)(t / Rh);
    float d[4];
#pragma unroll
    for (int di = 0; di < 2; ++di) {  // the (dj = 0, 1) pair is adjacent: one 8-B load each
      size_t o = ((size_t)b * 2 * Rh + 2 * ry + di) * (2 * Rw) + 2 * rx;
      const f32x2 ov = *(const f32x2*)(out + o), gv = *(const f32x2*)(gout + o);
      d[2 * di] = gv.x * (1.f - ov.x) * ov.x;  // ATen sigmoid_backward
      d[2 * di + 1] = gv.y * (1.f - ov.y) * ov.y;
    }
    const T* zr = z + (size_t)p * ldz;
    T* dzr = dz + (size_t)p * ldz;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 v = ld4(zr + 4 * q);
      float zv[4] = {v.x, v.y, v.z, v.w};
      f32x4 g;
      float gv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int c = 4 * q + e;
        gv[e] = d[0] * w[c] + d[1] * w[16 + c] + d[2] * w[32 + c] + d[3] * w[48 + c];
#pragma unroll
        for (int j = 0; j < 4; ++j) accw[j * 16 + c] += d[j] * zv[e];
      }
      g.x = gv[0];
      g.y = gv[1];
      g.z = gv[2];
      g.w = gv[3];
      st4(dzr + 4 * q, g);
    }
    for (int c = 16; c < ldz; c += 4) st4(dzr + c, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int j = 0; j < 4; ++j) accw[64 + j] += d[j];
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // dw10 (64 sums): a reduce-scatter butterfly. Each xor step halves the values
  // a lane holds (it keeps the half its lane bit selects and adds the partner's
  // copy of it), so after 6 steps lane L holds the wave sum of accw[L]: 63
  // cross-lane moves instead of 64 full wave reductions (384)
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const bool up = (lane & o) != 0;
#pragma unroll
    for (int i = 0; i < o; ++i) {
      const float lo = accw[i], hi = accw[i + o];
      accw[i] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, o, 64);
    }
  }
  red[wv][lane] = accw[0];
#pragma unroll
  for (int k = 64; k < 68; ++k) {
    float s = wave_sum(accw[k]);
    if (lane == 0) red[wv][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 68) {
    float s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    partial[(size_t)blockIdx.x * 68 + threadIdx.x] = s;
  }
}

// out[j] = sum_b partial[b][j]: one block per output column j (< 68)
__global__ void __launch_bounds__(256) head_reduce_kernel(const float* __restrict__ partial,
                                                          int nblk, float* dw10, float* db10) {
  __shared__ double sh[256];
  const int j = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) s += partial[(size_t)b * 68 + j];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (j < 64)
      dw10[j] = (float)sh[0];
    else
      db10[j - 64] = (float)sh[0];
  }
}

// ---------------------------------------------------------------------------
// Losses
// ---------------------------------------------------------------------------
__device__ __forceinline__ float block_sum256(float v, float* sh) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wv] = v;
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x == 0) {
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) r += sh[k];
  }
  return r;
}

__global__ void __launch_bounds__(256) l1_partial_kernel(const float* __restrict__ o,
                                                         const float* __restrict__ t, int64_t n,
                                                         float* __restrict__ partial) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    s += fabsf(o[i] - t[i]);
  float r = block_sum256(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// sum of exp(alpha*|a-b|) - 1 (measure_temporal_instability, pert_loss.py:170-199)
__global__ void __launch_bounds__(256) expdiff_partial_kernel(const float* __restrict__ a,
                                                              const float* __restrict__ b,
                                                              int64_t n, float alpha,
                                                              float* __restrict__ partial) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    s += expf(alpha * fabsf(a[i] - b[i])) - 1.f;
  float r = block_sum256(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

__global__ void finalize_mean_kernel(const float* __restrict__ partial, int nblk, double scale,
                                     float* out) {
  // one wave; fixed-order double accumulation
  __shared__ double sh[64];
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 64) s += partial[b];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int k = 0; k < 64; ++k) tot += sh[k];
    out[0] = (float)(tot * scale);
  }
}

__global__ void l1_bwd_kernel(const float* __restrict__ o, const float* __restrict__ t, int64_t n,
                              float alpha, const float* __restrict__ gscale, float* grad,
                              int accumulate) {
  const float gs = gscale ? gscale[0] : 1.f;
  const float mag = (alpha * gs) / (float)n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float d = o[i] - t[i];
    float s = d > 0.f ? mag : (d < 0.f ? -mag : 0.f);
    grad[i] = accumulate ? grad[i] + s : s;
  }
}

__global__ void __launch_bounds__(1024) channel_std_kernel(const float* __restrict__ x, int B, int C,
                                                           int HW, float* __restrict__ std_o) {
  // one block per channel, double accumulation, two passes (torch.std, unbiased)
  __shared__ double sh[16];
  const int c = blockIdx.x;
  const long long n = (long long)B * HW;
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += blockDim.x) {
    long long b = i / HW, r = i - b * HW;
    s += x[((size_t)b * C + c) * HW + r];
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  double tot = 0.0;
  for (int k = 0; k < (int)(blockDim.x >> 6); ++k) tot += sh[k];
  const double mean = tot / n;
  __syncthreads();
  double s2 = 0.0;
  for (long long i = threadIdx.x; i < n; i += blockDim.x) {
    long long b = i / HW, r = i - b * HW;
    double d = x[((size_t)b * C + c) * HW + r] - mean;
    s2 += d * d;
  }
  for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s2;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t2 = 0.0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) t2 += sh[k];
    std_o[c] = (float)sqrt(t2 / (double)(n > 1 ? n - 1 : 1));
  }
}

// setdata.py:316: x = (x - mean[c]) / (std[c] + eps), in place on [B][C][HW]
__global__ void normalize_frames_kernel(float* __restrict__ x, int C, long long HW, long long total,
                                        const float* __restrict__ mean,
                                        const float* __restrict__ stdv, float eps) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)((i / HW) % C);
    const float d = stdv[c] + eps;
    x[i] = (x[i] - mean[c]) / d;
  }
}

__global__ void perturb_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                               const float* __restrict__ stdv, int C, int HW, long long total,
                               float factor, float* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int c = (int)((i / HW) % C);
    out[i] = x[i] + (noise[i] * stdv[c]) * factor;
  }
}

// ---------------------------------------------------------------------------
// Train-step tail: global grad norm, clip coefficient, AdamW (torch semantics)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sumsq_partial_kernel(const float* __restrict__ g, int64_t n,
                                                            float* __restrict__ partial) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float v = g[i];
    s += v * v;
  }
  float r = block_sum256(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

__global__ void clip_coef_kernel(const float* __restrict__ sumsq, float inv_world, float max_norm,
                                 float* coef) {
  float norm = sqrtf(sumsq[0]) * inv_world;
  float c = max_norm / (norm + 1e-6f);
  coef[0] = inv_world * fminf(c, 1.f);
}

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                             float* __restrict__ m, float* __restrict__ v, int64_t n, float decay,
                             float beta1, float beta2, float eps, float step_size,
                             float bc2_sqrt, const float* __restrict__ gcoef) {
  const float gc = gcoef ? gcoef[0] : 1.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float gi = g[i] * gc;
    float pi = p[i] * decay;
    float mi = m[i];
    mi = mi + (1.f - beta1) * (gi - mi);
    float vi = v[i] * beta2 + (1.f - beta2) * gi * gi;
    float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi = pi - step_size * (mi / denom);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
  }
}

// torch.optim.Adam (single-tensor path, L2 weight decay): g += wd*p, then the
// moments and the update of adamw_kernel without the decoupled decay. Every
// rounding of torch's op sequence is kept (no FMA contraction).
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v, int64_t n, float wd,
                            float beta1, float beta2, float eps, float step_size, float bc2_sqrt,
                            const float* __restrict__ gcoef) {
#pragma clang fp contract(off)
  const float gc = gcoef ? gcoef[0] : 1.f;
  const float w1 = 1.f - beta1, w2 = 1.f - beta2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float pi = p[i];
    float gi = g[i] * gc;
    gi = gi + wd * pi;
    float mi = m[i];
    mi = mi + w1 * (gi - mi);
    float vi = v[i] * beta2;
    vi = vi + (w2 * gi) * gi;
    float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi = pi - step_size * (mi / denom);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
  }
}

// torch.optim.SGD (dampening 0, no Nesterov): g += wd*p; buf = g on the first
// step, else buf = mu*buf + g; p -= lr*buf. MOMENTUM = false: p -= lr*g, no buffer.
template <bool MOMENTUM>
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                           float* __restrict__ buf, int64_t n, float lr, float momentum, float wd,
                           int first, const float* __restrict__ gcoef) {
#pragma clang fp contract(off)
  const float gc = gcoef ? gcoef[0] : 1.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float pi = p[i];
    float gi = g[i] * gc;
    gi = gi + wd * pi;
    if (MOMENTUM) {
      if (!first) gi = buf[i] * momentum + gi;
      buf[i] = gi;
    }
    p[i] = pi - lr * gi;
  }
}

}  // namespace nsm

using namespace nsm;

// ============================== C ABI ======================================
extern "C" int nsm_input_prep(const float* x, int B, int C, int H, int W, void* out, int cp,
                              int dtype, uint32_t* amax, void* stream) {
  NSM_CHECK_ARG(x && out && H % 2 == 0 && W % 2 == 0 && cp >= 4 * C && cp % 8 == 0,
                "input_prep: bad args");
  NSM_CHECK_ARG(((uintptr_t)x % 8) == 0, "input_prep: x must be 8-byte aligned");
  const long long npix = (long long)B * (H / 2) * (W / 2);
  NSM_CHECK_ARG(npix < (1ll << 31), "input_prep: too large");
  dim3 g(grid_for(npix, 256, 2048));
  const FastDiv fw = make_fastdiv(W / 2), fh = make_fastdiv(H / 2);
  return for_dtype(dtype, "input_prep", [&](auto t) {
    using T = typename decltype(t)::type;
    // max|out| is recorded for the fp32 storage only
    uint32_t* am = std::is_same<T, float>::value ? amax : nullptr;
    hipLaunchKernelGGL(input_prep_kernel<T>, g, dim3(256), 0, as_stream(stream), x, B, C, H, W,
                       (T*)out, cp, (uint32_t)npix, fw, fh, am);
    NSM_LAUNCH_CHECK("input_prep");
    return 0;
  });
}

extern "C" int nsm_input_prep_h2(const float* x, int B, int C, int H, int W, void* out, int cp,
                                 uint32_t* amax, void* stream) {
  NSM_CHECK_ARG(x && out && amax && H % 2 == 0 && W % 2 == 0 && cp >= 4 * C && cp % 8 == 0,
                "input_prep_h2: bad args");
  NSM_CHECK_ARG(((uintptr_t)x % 8) == 0 && ((uintptr_t)out % 16) == 0, "input_prep_h2: alignment");
  const long long npix = (long long)B * (H / 2) * (W / 2);
  NSM_CHECK_ARG(npix < (1ll << 31), "input_prep_h2: too large");
  const int rc = nsm_absmax(x, (int64_t)B * C * H * W, amax, stream);  // the scale source
  if (rc) return rc;
  dim3 g(grid_for(npix, 256, 2048));
  hipLaunchKernelGGL((input_prep_kernel<bf16_t, true>), g, dim3(256), 0, as_stream(stream), x, B, C,
                     H, W, (bf16_t*)out, cp, (uint32_t)npix, make_fastdiv(W / 2),
                     make_fastdiv(H / 2), amax);
  NSM_LAUNCH_CHECK("input_prep_h2");
  return 0;
}

extern "C" int nsm_input_grad(const void* dX, int B, int C, int H, int W, int cp, float* dx,
                              int dtype, void* stream) {
  NSM_CHECK_ARG(dX && dx && H % 2 == 0 && W % 2 == 0 && cp >= 4 * C && cp % 4 == 0,
                "input_grad: bad args");
  long long work = (long long)B * C * (H / 2) * (W / 2);
  dim3 g(grid_for(work));
  return for_dtype(dtype, "input_grad", [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(input_grad_kernel<T>, g, dim3(256), 0, as_stream(stream), (const T*)dX, B,
                       C, H, W, cp, dx);
    NSM_LAUNCH_CHECK("input_grad");
    return 0;
  });
}

extern "C" int nsm_head_fwd(const void* z, int ldz, int B, int Rh, int Rw, const float* w10,
                            const float* b10, float* out, int dtype, void* stream) {
  NSM_CHECK_ARG(z && w10 && b10 && out && ldz >= 16 && ldz % 4 == 0, "head_fwd: bad args");
  long long npix = (long long)B * Rh * Rw;
  dim3 g(grid_for(npix));
  return for_dtype(dtype, "head_fwd", [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(head_fwd_kernel<T>, g, dim3(256), 0, as_stream(stream), (const T*)z, ldz, B,
                       Rh, Rw, w10, b10, out);
    NSM_LAUNCH_CHECK("head_fwd");
    return 0;
  });
}

extern "C" int nsm_head_bwd_blocks(int B, int Rh, int Rw) {
  return grid_for((long long)B * Rh * Rw, 256, 1024);
}

extern "C" int nsm_head_bwd(const float* gout, const float* out, const void* z, int ldz, int B,
                            int Rh, int Rw, const float* w10, void* dz, float* partial, float* dw10,
                            float* db10, int dtype, void* stream) {
  NSM_CHECK_ARG(gout && out && z && w10 && dz && partial && dw10 && db10 && ldz % 4 == 0,
                "head_bwd: bad args");
  int nblk = nsm_head_bwd_blocks(B, Rh, Rw);
  hipStream_t s = as_stream(stream);
  return for_dtype(dtype, "head_bwd", [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(head_bwd_kernel<T>, dim3(nblk), dim3(256), 0, s, gout, out, (const T*)z,
                       ldz, B, Rh, Rw, w10, (T*)dz, partial);
    NSM_LAUNCH_CHECK("head_bwd");
    hipLaunchKernelGGL(head_reduce_kernel, dim3(68), dim3(256), 0, s, partial, nblk, dw10, db10);
    NSM_LAUNCH_CHECK("head_reduce");
    return 0;
  });
}

extern "C" int nsm_loss_blocks(int64_t n) { return grid_for(n, 1024, 1024); }

extern "C" int nsm_l1_loss_fwd(const float* o, const float* t, int64_t n, float alpha,
                               float* partial, float* out, void* stream) {
  NSM_CHECK_ARG(o && t && partial && out && n > 0, "l1_loss_fwd: bad args");
  int nb = nsm_loss_blocks(n);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(l1_partial_kernel, dim3(nb), dim3(256), 0, s, o, t, n, partial);
  hipLaunchKernelGGL(finalize_mean_kernel, dim3(1), dim3(64), 0, s, partial, nb,
                     (double)alpha / (double)n, out);
  NSM_LAUNCH_CHECK("l1_loss_fwd");
  return 0;
}

extern "C" int nsm_expdiff_mean(const float* a, const float* b, int64_t n, float alpha,
                                float* partial, float* out, void* stream) {
  NSM_CHECK_ARG(a && b && partial && out && n > 0, "expdiff_mean: bad args");
  int nb = nsm_loss_blocks(n);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(expdiff_partial_kernel, dim3(nb), dim3(256), 0, s, a, b, n, alpha, partial);
  hipLaunchKernelGGL(finalize_mean_kernel, dim3(1), dim3(64), 0, s, partial, nb, 1.0 / (double)n,
                     out);
  NSM_LAUNCH_CHECK("expdiff_mean");
  return 0;
}

extern "C" int nsm_l1_loss_bwd(const float* o, const float* t, int64_t n, float alpha,
                               const float* gscale, float* grad, int accumulate, void* stream) {
  NSM_CHECK_ARG(o && t && grad && n > 0, "l1_loss_bwd: bad args");
  hipLaunchKernelGGL(l1_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, as_stream(stream), o, t, n,
                     alpha, gscale, grad, accumulate);
  NSM_LAUNCH_CHECK("l1_loss_bwd");
  return 0;
}

extern "C" int nsm_channel_std(const float* x, int B, int C, int H, int W, float* partial,
                               float* std_o, void* stream) {
  (void)partial;
  NSM_CHECK_ARG(x && std_o && B * H * W > 0, "channel_std: bad args");
  hipLaunchKernelGGL(channel_std_kernel, dim3(C), dim3(1024), 0, as_stream(stream), x, B, C, H * W,
                     std_o);
  NSM_LAUNCH_CHECK("channel_std");
  return 0;
}

extern "C" int nsm_perturb(const float* x, const float* noise, const float* stdv, int B, int C,
                           int H, int W, float factor, float* out, void* stream) {
  NSM_CHECK_ARG(x && noise && stdv && out, "perturb: bad args");
  long long total = (long long)B * C * H * W;
  hipLaunchKernelGGL(perturb_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), x,
                     noise, stdv, C, H * W, total, factor, out);
  NSM_LAUNCH_CHECK("perturb");
  return 0;
}

extern "C" int nsm_normalize_frames(float* x, int B, int C, int64_t HW, const float* mean,
                                    const float* stdv, float eps, void* stream) {
  NSM_CHECK_ARG(x && mean && stdv && B > 0 && C > 0 && HW > 0, "normalize_frames: bad args");
  long long total = (long long)B * C * HW;
  hipLaunchKernelGGL(normalize_frames_kernel, dim3(grid_for(total)), dim3(256), 0,
                     as_stream(stream), x, C, (long long)HW, total, mean, stdv, eps);
  NSM_LAUNCH_CHECK("normalize_frames");
  return 0;
}

extern "C" int nsm_sumsq(const float* g, int64_t n, float* partial, float* out, void* stream) {
  NSM_CHECK_ARG(g && partial && out && n > 0, "sumsq: bad args");
  int nb = nsm_loss_blocks(n);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nb), dim3(256), 0, s, g, n, partial);
  hipLaunchKernelGGL(finalize_mean_kernel, dim3(1), dim3(64), 0, s, partial, nb, 1.0, out);
  NSM_LAUNCH_CHECK("sumsq");
  return 0;
}

extern "C" int nsm_clip_coef(const float* sumsq, float inv_world, float max_norm, float* coef,
                             void* stream) {
  NSM_CHECK_ARG(sumsq && coef, "clip_coef: bad args");
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(1), 0, as_stream(stream), sumsq, inv_world,
                     max_norm, coef);
  NSM_LAUNCH_CHECK("clip_coef");
  return 0;
}

extern "C" int nsm_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int step,
                              const float* gcoef, void* stream) {
  NSM_CHECK_ARG(p && g && m && v && n > 0 && step >= 1, "adamw: bad args");
  double bc1 = 1.0 - pow((double)beta1, step);
  double bc2 = 1.0 - pow((double)beta2, step);
  float step_size = (float)(lr / bc1);
  float bc2_sqrt = (float)sqrt(bc2);
  float decay = 1.f - lr * weight_decay;
  hipLaunchKernelGGL(adamw_kernel, dim3(grid_for(n)), dim3(256), 0, as_stream(stream), p, g, m, v,
                     n, decay, beta1, beta2, eps, step_size, bc2_sqrt, gcoef);
  NSM_LAUNCH_CHECK("adamw");
  return 0;
}

extern "C" int nsm_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr,
                             float beta1, float beta2, float eps, float weight_decay, int step,
                             const float* gcoef, void* stream) {
  NSM_CHECK_ARG(p && g && m && v && n > 0 && step >= 1, "adam: bad args");
  double bc1 = 1.0 - pow((double)beta1, step);
  double bc2 = 1.0 - pow((double)beta2, step);
  float step_size = (float)(lr / bc1);
  float bc2_sqrt = (float)sqrt(bc2);
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, as_stream(stream), p, g, m, v,
                     n, weight_decay, beta1, beta2, eps, step_size, bc2_sqrt, gcoef);
  NSM_LAUNCH_CHECK("adam");
  return 0;
}

extern "C" int nsm_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr,
                            float momentum, float weight_decay, int step, const float* gcoef,
                            void* stream) {
  NSM_CHECK_ARG(p && g && n > 0 && step >= 1 && (buf || momentum == 0.f), "sgd: bad args");
  if (momentum != 0.f)
    hipLaunchKernelGGL(sgd_kernel<true>, dim3(grid_for(n)), dim3(256), 0, as_stream(stream), p, g,
                       buf, n, lr, momentum, weight_decay, step == 1 ? 1 : 0, gcoef);
  else
    hipLaunchKernelGGL(sgd_kernel<false>, dim3(grid_for(n)), dim3(256), 0, as_stream(stream), p, g,
                       (float*)nullptr, n, lr, 0.f, weight_decay, 0, gcoef);
  NSM_LAUNCH_CHECK("sgd");
  return 0;
}
