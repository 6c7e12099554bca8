// BatchNorm on NHWC activations ("Element-wise sources"): batch
// statistics and their finalize / merge kernels, the apply + LeakyReLU
// (+ Dropout2d mask, + skip) pass, and the backward's reduce / finalize / apply,
// each also in the form that writes an h2 operand for the fp32 1x1 convs.
// Cross-block reductions are deterministic: each block writes a partial row, a
// small finalize kernel merges the rows in a fixed order (double).
#include "nsm_elem.h"

namespace nsm {

// Column reductions over an [M][C] NHWC matrix: block = 256 threads laid out
// as rl row-lanes x cl 8-channel lanes; grid = (gx channel groups, nchunk).
static inline int gcd_i(int a, int b) {
  while (b) {
    int t = a % b;
    a = b;
    b = t;
  }
  return a;
}
struct ColRed {
  int cl, rl, gx, nchunk, rpc;
};
static ColRed colred_plan(int M, int C) {
  ColRed r;
  r.cl = gcd_i(C / 8, 64);
  r.rl = 256 / r.cl;
  r.gx = (C / 8) / r.cl;
  long long want = (M + 63) / 64;
  long long cap = 1024 / r.gx;  // ~1024 blocks fill the 256 CUs; finalize stays short
  if (cap < 1) cap = 1;
  r.nchunk = (int)(want < cap ? want : cap);
  if (r.nchunk < 1) r.nchunk = 1;
  r.rpc = ceil_div(M, r.nchunk);
  return r;
}

template <typename T>
__global__ void __launch_bounds__(256) bn_stats_kernel(const T* __restrict__ y, int ld, int M,
                                                       int C, int cl, int rl, int rpc,
                                                       float* __restrict__ partial) {
  __shared__ F8 red[256];
  const int tid = threadIdx.x, tc = tid % cl, tr = tid / cl;
  const int c = (blockIdx.x * cl + tc) * 8;
  const int r0 = blockIdx.y * rpc, r1 = min(M, r0 + rpc);
  F8 s = f8zero();
#pragma unroll 4
  for (int r = r0 + tr; r < r1; r += rl) s += ld8(y + (size_t)r * ld + c);
  red[tid] = s;
  col_tree_reduce(red, cl, rl, tid);
  const float n = (float)max(r1 - r0, 1);
  const F8 sum = red[tc];
  const F8 mean = (1.f / n) * sum;
  __syncthreads();
  F8 s2 = f8zero();
#pragma unroll 4
  for (int r = r0 + tr; r < r1; r += rl) {
    F8 d = ld8(y + (size_t)r * ld + c) - mean;
    s2 += d * d;
  }
  red[tid] = s2;
  col_tree_reduce(red, cl, rl, tid);
  if (tr == 0) {
    float* pr = partial + (size_t)blockIdx.y * 2 * C;
    st8(pr + c, sum);
    st8(pr + C + c, red[tc]);
  }
}

// Finalize kernels: one wave per channel; lanes stride over the partial rows
// (4 independent accumulators keep several loads in flight), fixed-order
// double reduction with cross-lane butterflies.
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// fixed-order double sum over a 256-thread block (red: 4 doubles of LDS)
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();  // red may still be read from a previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// One 256-thread block per channel: every partial row of a pass is loaded by
// one lane in one round (the per-wave form took ~nchunk/256 dependent rounds).
__global__ void __launch_bounds__(256) bn_finalize_train_kernel(
    const float* __restrict__ partial, int nchunk, int rpc, int M, int C, int c_real,
    const float* __restrict__ gamma, const float* __restrict__ beta, float* run_mean,
    float* run_var, int64_t* num_batches, float momentum, float eps, int n_updates, float* mean_o,
    float* invstd_o, float* scale_o, float* shift_o, uint32_t* bound, float bound_mul) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  if (blockIdx.x == 0 && tid == 0 && num_batches) *num_batches += n_updates;
  // rpc == 0: counted partials [nchunk][3][C] = {sum, M2, count} (the Winograd
  // output transform's slots); else {sum, M2} of rpc-row chunks
  const size_t st = (size_t)(rpc ? 2 : 3) * C;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int k = tid;
  for (; k + 768 < nchunk; k += 1024) {
    s0 += partial[k * st + c];
    s1 += partial[(k + 256) * st + c];
    s2 += partial[(k + 512) * st + c];
    s3 += partial[(k + 768) * st + c];
  }
  for (; k < nchunk; k += 256) s0 += partial[k * st + c];
  const double mean = block_sum_d((s0 + s1) + (s2 + s3), red) / M;
  double q0 = 0.0, q1 = 0.0;
  for (k = tid; k < nchunk; k += 512) {
    int n0 = rpc ? min(M, k * rpc + rpc) - k * rpc : (int)partial[k * st + 2 * C + c];
    if (n0 > 0) {
      double d = partial[k * st + c] / n0 - mean;
      q0 += partial[k * st + C + c] + n0 * d * d;
    }
    int k1 = k + 256;
    if (k1 < nchunk) {
      int n1 = rpc ? min(M, k1 * rpc + rpc) - k1 * rpc : (int)partial[k1 * st + 2 * C + c];
      if (n1 > 0) {
        double d = partial[k1 * st + c] / n1 - mean;
        q1 += partial[k1 * st + C + c] + n1 * d * d;
      }
    }
  }
  const double m2 = block_sum_d(q0 + q1, red);
  if (tid != 0) return;
  const float var_b = (float)(m2 / M);
  const float var_u = M > 1 ? (float)(m2 / (M - 1)) : var_b;
  const float mf = (float)mean;
  const float inv = 1.0f / sqrtf(var_b + eps);
  const float sc = gamma[c] * inv;
  mean_o[c] = mf;
  invstd_o[c] = inv;
  scale_o[c] = sc;
  shift_o[c] = beta[c] - mf * sc;
  if (bound) {
    // max over the batch of |lrelu(y*scale+shift)| * mask_max, the scale source
    // of the h2 activated operand (nsm_bn_act_h2) known before it is written:
    // y*scale + shift = scale (y - mean) + beta and, for n values with biased
    // variance var, max|y - mean| <= sqrt(var (n - 1)) (Samuelson), so
    // |BN(y)| <= |scale| sqrt(var (n - 1)) + |beta|; LeakyReLU does not grow
    // it. In double, 1e-6 up (the fp32 apply rounds within the s headroom).
    const double b = ((double)fabsf(sc) * sqrt((double)var_b * (double)(M - 1)) +
                      (double)fabsf(beta[c])) * (double)bound_mul * (1.0 + 1e-6);
    atomicMax(bound + (c & (AMAX_LINES - 1)) * AMAX_STRIDE, __float_as_uint((float)b) & 0x7fffffffu);
  }
  if (c < c_real && run_mean) {
    float rm = run_mean[c], rv = run_var[c];
    for (int u = 0; u < n_updates; ++u) {
      rm = momentum * mf + (1.f - momentum) * rm;
      rv = momentum * var_u + (1.f - momentum) * rv;
    }
    run_mean[c] = rm;
    run_var[c] = rv;
  }
}

// First level of the BN-partial merge for grids with many row chunks:
// out[g] = Chan merge of chunks [g*G, (g+1)*G) (fixed order, double), one
// thread per (group, channel), coalesced along channels.
// rpc == 0: counted rows in and out ({sum, M2, count}, stride 3C)
__global__ void bn_partials_merge_kernel(const float* __restrict__ partial, int nchunk, int rpc,
                                         int M, int C, int G, float* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (c >= C) return;
  const size_t st = (size_t)(rpc ? 2 : 3) * C;
  const int k0 = g * G, k1 = min(nchunk, k0 + G);
  double s = 0.0;
  long long n = 0;
  for (int k = k0; k < k1; ++k) {
    s += partial[(size_t)k * st + c];
    n += rpc ? max(0, min(M, (k + 1) * rpc) - k * rpc) : (long long)partial[(size_t)k * st + 2 * C + c];
  }
  const double mean = n > 0 ? s / (double)n : 0.0;
  double m2 = 0.0;
  for (int k = k0; k < k1; ++k) {
    const int nk = rpc ? min(M, (k + 1) * rpc) - k * rpc : (int)partial[(size_t)k * st + 2 * C + c];
    if (nk <= 0) continue;
    const double d = partial[(size_t)k * st + c] / nk - mean;
    m2 += partial[(size_t)k * st + C + c] + nk * d * d;
  }
  out[(size_t)g * st + c] = (float)s;
  out[(size_t)g * st + C + c] = (float)m2;
  if (!rpc) out[(size_t)g * st + 2 * C + c] = (float)n;
}

// Plain-sum merge of partial rows (the BN-backward {sum dz, sum dz*xhat}
// format): out[g][j] = sum over rows [g*G, (g+1)*G) of part[.][j], fixed
// order, one thread per column (coalesced along the row)
__global__ void sum_rows_kernel(const float* __restrict__ part, int nrows, int width, int G,
                                float* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, g = blockIdx.y;
  if (j >= width) return;
  const int k0 = g * G, k1 = min(nrows, k0 + G);
  double s = 0.0, s1 = 0.0;  // two rows' loads in flight, fixed order
  int k = k0;
  for (; k + 1 < k1; k += 2) {
    s += part[(size_t)k * width + j];
    s1 += part[(size_t)(k + 1) * width + j];
  }
  if (k < k1) s += part[(size_t)k * width + j];
  out[(size_t)g * width + j] = (float)(s + s1);
}

__global__ void bn_finalize_eval_kernel(const float* __restrict__ rm, const float* __restrict__ rv,
                                        const float* __restrict__ gamma,
                                        const float* __restrict__ beta, int C, int c_real, float eps,
                                        float* mean_o, float* invstd_o, float* scale_o,
                                        float* shift_o) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float m = c < c_real ? rm[c] : 0.f;
  float v = c < c_real ? rv[c] : 1.f;
  float inv = 1.0f / sqrtf(v + eps);
  float sc = gamma[c] * inv;
  mean_o[c] = m;
  invstd_o[c] = inv;
  scale_o[c] = sc;
  shift_o[c] = beta[c] - m * sc;
}

// Pixel-row streaming (bn_act, bn_bwd_apply): a block covers whole pixels
// (blockDim = k*C8, pix_launch), so each lane keeps ONE 8-channel group for
// the whole grid-stride loop and its per-channel vectors stay in registers.
//
// out = lrelu(y*scale+shift) (* mask[b][c]) (+ res)
template <typename T>
__global__ void __launch_bounds__(256) bn_act_kernel(const T* __restrict__ y, int ldy, int M,
                                                     int C8, FastDiv fdHW,
                                                     const float* __restrict__ scale,
                                                     const float* __restrict__ shift, float slope,
                                                     const float* __restrict__ mask,
                                                     const T* __restrict__ res, int ldres,
                                                     T* __restrict__ out, int ldo,
                                                     uint32_t* __restrict__ amax) {
  const int ppb = blockDim.x / C8, tp = threadIdx.x / C8;
  const int c = (threadIdx.x - tp * C8) * 8;
  const F8 sc = ldf8(scale + c), sh = ldf8(shift + c);
  const int pstep = gridDim.x * ppb;
  uint32_t am = 0;  // max|out| (an f16x2 GEMM operand scale, fp32 only)
  for (int p = blockIdx.x * ppb + tp; p < M; p += pstep) {
    F8 o = lrelu8(ld8(y + (size_t)p * ldy + c) * sc + sh, slope);
    // Dropout2d after the LeakyReLU (Unetmodel.py:23-24)
    if (mask) o = o * ld8(mask + (size_t)fdiv((uint32_t)p, fdHW) * (C8 * 8) + c);
    if (res) o += ld8(res + (size_t)p * ldres + c);
    st8(out + (size_t)p * ldo + c, o);
    if (amax) {
      amax_fold(am, o.a);
      amax_fold(am, o.b);
    }
  }
  amax_flush(am, amax);
}

// bn_act's activated operand written as an h2 tensor out [M][2C] (fp32 in):
// the 1x1 conv's A1 (nsm_conv_h2d.inc), scale from the bound slot its BN
// finalize filled (nsm_bn_finalize_train `bound`)
__global__ void __launch_bounds__(256) bn_act_h2_kernel(const float* __restrict__ y, int ldy, int M,
                                                        int C8, FastDiv fdHW,
                                                        const float* __restrict__ scale,
                                                        const float* __restrict__ shift,
                                                        float slope,
                                                        const float* __restrict__ mask,
                                                        bf16_t* __restrict__ out, H2Scale hs) {
  const float s = exp2i(h2_exp(hs));  // every lane: amax_read is a wave reduction
  const int ppb = 256 / C8, tp = threadIdx.x / C8;  // (pix_launch_h2: whole waves)
  if (tp >= ppb) return;
  const int c = (threadIdx.x - tp * C8) * 8;
  const F8 sc = ldf8(scale + c), sh = ldf8(shift + c);
  const int pstep = gridDim.x * ppb;
  for (int p = blockIdx.x * ppb + tp; p < M; p += pstep) {
    F8 mk = f8zero();
    if (mask) mk = ld8(mask + (size_t)fdiv((uint32_t)p, fdHW) * (C8 * 8) + c);
    u32x4 h, l;
    bn_act_h2_8(ld8(y + (size_t)p * ldy + c), sc, sh, slope, mask != nullptr, mk, s, h, l);
    bf16_t* row = out + (size_t)p * 16 * C8;
    *(u32x4*)(row + 2 * c) = h;
    *(u32x4*)(row + 2 * c + 8) = l;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) bn_bwd_reduce_kernel(
    const T* __restrict__ g, int ldg, const T* __restrict__ y, int ldy, int M, int C,
    FastDiv fdHW, const float* __restrict__ scale, const float* __restrict__ shift, float slope,
    const float* __restrict__ mask, const float* __restrict__ mean,
    const float* __restrict__ invstd, int cl, int rl, int rpc, float* __restrict__ partial,
    uint32_t* __restrict__ amax) {
  __shared__ F8 red[256];
  const int tid = threadIdx.x, tc = tid % cl, tr = tid / cl;
  const int c = (blockIdx.x * cl + tc) * 8;
  const int r0 = blockIdx.y * rpc, r1 = min(M, r0 + rpc);
  const F8 sc = ldf8(scale + c), sh = ldf8(shift + c);
  const F8 mu = ldf8(mean + c), is = ldf8(invstd + c);
  F8 s1 = f8zero(), s2 = f8zero();
  uint32_t am = 0;  // max|scale * dz| (scale = gamma * invstd = k1 of the finalize)
#pragma unroll 2
  for (int r = r0 + tr; r < r1; r += rl) {
    const F8 v = ld8(y + (size_t)r * ldy + c);
    const F8 gg = ld8(g + (size_t)r * ldg + c);
    const int b = mask ? (int)fdiv((uint32_t)r, fdHW) : 0;
    const F8 dz = bn_dz8(gg, v, sc, sh, slope, mask, b, C, c);
    s1 += dz;
    s2 += dz * ((v - mu) * is);
    if (amax) {
      amax_fold(am, sc.a * dz.a);
      amax_fold(am, sc.b * dz.b);
    }
  }
  amax_flush(am, amax);
  red[tid] = s1;
  col_tree_reduce(red, cl, rl, tid);
  const F8 t1 = red[tc];
  __syncthreads();
  red[tid] = s2;
  col_tree_reduce(red, cl, rl, tid);
  if (tr == 0) {
    float* pr = partial + (size_t)blockIdx.y * 2 * C;
    st8(pr + c, t1);
    st8(pr + C + c, red[tc]);
  }
}

__global__ void __launch_bounds__(256) bn_bwd_finalize_kernel(
    const float* __restrict__ partial, int nchunk, int M, int C, int c_real,
    const float* __restrict__ gamma, const float* __restrict__ invstd, float* dgamma,
    float* dbeta, float* dbias_prev, float* coef, const uint32_t* __restrict__ amax_k1dz,
    uint32_t* __restrict__ bound) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int c = blockIdx.x;  // one block per channel (see bn_finalize_train_kernel)
  // max over the tensor of |k1 dz| (recorded by the reduction's producer): every
  // lane of the block's waves (amax_read is a wave reduction)
  const float a_k1dz = bound ? __uint_as_float(amax_read(amax_k1dz)) : 0.f;
  const size_t st = (size_t)2 * C;
  double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
  int k = tid;
  for (; k + 256 < nchunk; k += 512) {
    a0 += partial[k * st + c];
    b0 += partial[k * st + C + c];
    a1 += partial[(k + 256) * st + c];
    b1 += partial[(k + 256) * st + C + c];
  }
  for (; k < nchunk; k += 256) {
    a0 += partial[k * st + c];
    b0 += partial[k * st + C + c];
  }
  const double S1 = block_sum_d(a0 + a1, red), S2 = block_sum_d(b0 + b1, red);
  if (tid != 0) return;
  const float gm = gamma[c], is = invstd[c];
  const double mdz = S1 / M, mdzx = S2 / M;
  const float k1 = gm * is;
  const float k2 = (float)(-(double)gm * is * is * mdzx);
  const float k3 = (float)(-(double)k1 * mdz);
  coef[c] = k1;
  coef[C + c] = k2;
  coef[2 * C + c] = k3;
  if (bound) {
    // dy = k1 dz + k2 (y - mean) + k3 with max|y - mean| <= sqrt(var (M - 1))
    // <= sqrt(M - 1) / invstd (Samuelson, biased var): a bound of max|dy| known
    // before nsm_bn_bwd_apply_h2 writes dy, the scale source of that h2 tensor
    const double b = ((double)a_k1dz + fabs((double)k2) * sqrt((double)(M - 1)) / (double)is +
                      fabs((double)k3)) * (1.0 + 1e-6);
    atomicMax(bound + (c & (AMAX_LINES - 1)) * AMAX_STRIDE, __float_as_uint((float)b) & 0x7fffffffu);
  }
  if (c < c_real) {
    if (dgamma) dgamma[c] = (float)S2;
    if (dbeta) dbeta[c] = (float)S1;
    // sum_p dy = k1*S1 + k2*sum(y-mean) + k3*M == 0 analytically (pre-BN bias)
    if (dbias_prev) dbias_prev[c] = (float)((double)k1 * S1 + (double)k3 * M);
  }
}

template <typename T>
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(
    const T* __restrict__ g, int ldg, const T* __restrict__ y, int ldy, int M, int C, int C8,
    FastDiv fdHW, const float* __restrict__ scale, const float* __restrict__ shift, float slope,
    const float* __restrict__ mask, const float* __restrict__ mean,
    const float* __restrict__ coef, T* __restrict__ dy, int lddy, uint32_t* __restrict__ amax) {
  const int ppb = blockDim.x / C8, tp = threadIdx.x / C8;
  const int c = (threadIdx.x - tp * C8) * 8;
  const F8 sc = ldf8(scale + c), sh = ldf8(shift + c), mu = ldf8(mean + c);
  const F8 k1 = ldf8(coef + c), k2 = ldf8(coef + C + c), k3 = ldf8(coef + 2 * C + c);
  const int pstep = gridDim.x * ppb;
  uint32_t am = 0;  // max|dy| (an f16x2 GEMM operand scale, fp32 only)
  for (int p = blockIdx.x * ppb + tp; p < M; p += pstep) {
    const F8 v = ld8(y + (size_t)p * ldy + c);
    const F8 gg = ld8(g + (size_t)p * ldg + c);
    const int b = mask ? (int)fdiv((uint32_t)p, fdHW) : 0;
    const F8 dz = bn_dz8(gg, v, sc, sh, slope, mask, b, C, c);
    const F8 d = k1 * dz + k2 * (v - mu) + k3;
    st8(dy + (size_t)p * lddy + c, d);
    if (amax) {
      amax_fold(am, d.a);
      amax_fold(am, d.b);
    }
  }
  amax_flush(am, amax);
}

// nsm_bn_bwd_apply (fp32) writing dy as an h2 tensor [M][2C] with the scale
// source `bound` (nsm_bn_bwd_finalize's): the 1x1 conv's output gradient dY2
// read by its h2 weight and input gradients (nsm_conv_h2d.inc)
__global__ void __launch_bounds__(256) bn_bwd_apply_h2_kernel(
    const float* __restrict__ g, int ldg, const float* __restrict__ y, int ldy, int M, int C,
    int C8, FastDiv fdHW, const float* __restrict__ scale, const float* __restrict__ shift,
    float slope, const float* __restrict__ mask, const float* __restrict__ mean,
    const float* __restrict__ coef, bf16_t* __restrict__ dy, H2Scale hs) {
  const float s = exp2i(h2_exp(hs));  // every lane: amax_read is a wave reduction
  const int ppb = 256 / C8, tp = threadIdx.x / C8;  // (pix_launch_h2: whole waves)
  if (tp >= ppb) return;
  const int c = (threadIdx.x - tp * C8) * 8;
  const F8 sc = ldf8(scale + c), sh = ldf8(shift + c), mu = ldf8(mean + c);
  const F8 k1 = ldf8(coef + c), k2 = ldf8(coef + C + c), k3 = ldf8(coef + 2 * C + c);
  const int pstep = gridDim.x * ppb;
  for (int p = blockIdx.x * ppb + tp; p < M; p += pstep) {
    const F8 v = ld8(y + (size_t)p * ldy + c);
    const F8 gg = ld8(g + (size_t)p * ldg + c);
    const int b = mask ? (int)fdiv((uint32_t)p, fdHW) : 0;
    const F8 dz = bn_dz8(gg, v, sc, sh, slope, mask, b, C, c);
    h2_store8(dy + (size_t)p * 2 * C, c, k1 * dz + k2 * (v - mu) + k3, s);
  }
}

// streaming launch over [M pixels][C8 channel groups]: blockDim = the largest
// multiple of C8 <= 256 (each lane keeps one channel group), <= 2048 blocks
static void pix_launch(long long M, int C8, dim3& grid, dim3& block) {
  const int tpb = (256 / C8) * C8;
  const long long ppb = tpb / C8;
  long long g = (M + ppb - 1) / ppb;
  g = g < 1 ? 1 : (g > 2048 ? 2048 : g);
  grid = dim3((unsigned)g);
  block = dim3((unsigned)tpb);
}

// pix_launch for the kernels that read an h2 scale (h2_exp reduces the 64
// lines of the maximum slot across the wave: every lane of every wave must be
// there): the block rounded up to whole waves, the lanes past the last pixel
// group leave after the reduction. (C = 96: 252 threads left 4 lanes of the
// last wave out and its rows took a maximum short of 4 lines.)
static void pix_launch_h2(long long M, int C8, dim3& grid, dim3& block) {
  pix_launch(M, C8, grid, block);
  block.x = (block.x + 63u) & ~63u;
}

}  // namespace nsm

using namespace nsm;

// ============================== C ABI ======================================
extern "C" int nsm_reduce_chunks(int M, int C) {
  if (M <= 0 || C <= 0 || C % 8) return 0;
  return colred_plan(M, C).nchunk;
}

extern "C" int nsm_bn_stats(const void* y, int ld, int M, int C, float* partial, int nchunk,
                            int dtype, void* stream) {
  NSM_CHECK_ARG(y && partial && M > 0 && C % 8 == 0 && ld % 8 == 0, "bn_stats: bad args");
  ColRed r = colred_plan(M, C);
  NSM_CHECK_ARG(nchunk == r.nchunk, "bn_stats: nchunk %d != %d", nchunk, r.nchunk);
  dim3 g(r.gx, r.nchunk);
  return for_dtype(dtype, "bn_stats", [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(bn_stats_kernel<T>, g, dim3(256), 0, as_stream(stream), (const T*)y, ld, M,
                       C, r.cl, r.rl, r.rpc, partial);
    NSM_LAUNCH_CHECK("bn_stats");
    return 0;
  });
}

extern "C" int nsm_reduce_rows(int M, int C) {
  if (M <= 0 || C <= 0 || C % 8) return 0;
  return colred_plan(M, C).rpc;
}

extern "C" int nsm_bn_finalize_train(const float* partial, int nchunk, int rows_per_chunk, int M,
                                     int C, int c_real, const float* gamma, const float* beta,
                                     float* run_mean, float* run_var, int64_t* num_batches,
                                     float momentum, float eps, int n_updates, float* mean,
                                     float* invstd, float* scale, float* shift, uint32_t* bound,
                                     float bound_mul, void* stream) {
  NSM_CHECK_ARG(partial && gamma && beta && mean && invstd && scale && shift, "bn_finalize: null");
  NSM_CHECK_ARG(M > 1, "bn_finalize: Expected more than 1 value per channel when training");
  NSM_CHECK_ARG(nchunk >= 1 && (rows_per_chunk == 0 ||
                                (rows_per_chunk >= 1 && (long long)nchunk * rows_per_chunk >= M)),
                "bn_finalize: chunks do not cover M");
  hipLaunchKernelGGL(bn_finalize_train_kernel, dim3(C), dim3(256), 0,
                     as_stream(stream), partial, nchunk, rows_per_chunk, M, C, c_real, gamma, beta,
                     run_mean,
                     run_var, num_batches, momentum, eps, n_updates, mean, invstd, scale, shift,
                     bound, bound_mul);
  NSM_LAUNCH_CHECK("bn_finalize_train");
  return 0;
}

extern "C" int nsm_bn_partials_merge(const float* partial, int nchunk, int rows_per_chunk, int M,
                                     int C, int group, float* out, void* stream) {
  NSM_CHECK_ARG(partial && out && nchunk >= 1 && group >= 1 && rows_per_chunk >= 0,
                "bn_partials_merge: bad args");
  dim3 grid(ceil_div(C, 256), ceil_div(nchunk, group));
  hipLaunchKernelGGL(bn_partials_merge_kernel, grid, dim3(256), 0, as_stream(stream), partial,
                     nchunk, rows_per_chunk, M, C, group, out);
  NSM_LAUNCH_CHECK("bn_partials_merge");
  return 0;
}

extern "C" int nsm_sum_rows(const float* part, int nrows, int width, int group, float* out,
                            void* stream) {
  NSM_CHECK_ARG(part && out && nrows >= 1 && width >= 1 && group >= 1, "sum_rows: bad args");
  dim3 grid(ceil_div(width, 256), ceil_div(nrows, group));
  hipLaunchKernelGGL(sum_rows_kernel, grid, dim3(256), 0, as_stream(stream), part, nrows, width,
                     group, out);
  NSM_LAUNCH_CHECK("sum_rows");
  return 0;
}

extern "C" int nsm_bn_finalize_eval(const float* run_mean, const float* run_var,
                                    const float* gamma, const float* beta, int C, int c_real,
                                    float eps, float* mean, float* invstd, float* scale,
                                    float* shift, void* stream) {
  NSM_CHECK_ARG(run_mean && run_var && gamma && beta && scale && shift, "bn_finalize_eval: null");
  hipLaunchKernelGGL(bn_finalize_eval_kernel, dim3(ceil_div(C, 256)), dim3(256), 0,
                     as_stream(stream), run_mean, run_var, gamma, beta, C, c_real, eps, mean, invstd,
                     scale, shift);
  NSM_LAUNCH_CHECK("bn_finalize_eval");
  return 0;
}

extern "C" int nsm_bn_act(const void* y, int ldy, int M, int C, const float* scale,
                          const float* shift, float slope, const float* mask, int HW,
                          const void* res, int ldres, void* out, int ldo, int dtype,
                          uint32_t* amax, void* stream) {
  NSM_CHECK_ARG(y && scale && shift && out && C % 8 == 0 && C <= 2048 && ldy % 8 == 0 &&
                    ldo % 8 == 0 && (!res || ldres % 8 == 0) && (!mask || HW > 0),
                "bn_act: bad args");
  NSM_CHECK_ARG(M >= 0 && M < (1 << 30), "bn_act: too large");
  if (M == 0) return 0;
  dim3 g, b;
  pix_launch(M, C / 8, g, b);
  const FastDiv fh = make_fastdiv(mask ? HW : 1);
  return for_dtype(dtype, "bn_act", [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(bn_act_kernel<T>, g, b, 0, as_stream(stream), (const T*)y, ldy, M, C / 8,
                       fh, scale, shift, slope, mask, (const T*)res, ldres, (T*)out, ldo, amax);
    NSM_LAUNCH_CHECK("bn_act");
    return 0;
  });
}

extern "C" int nsm_bn_act_h2(const float* y, int ldy, int M, int C, const float* scale,
                             const float* shift, float slope, const float* mask, int HW, void* out,
                             const uint32_t* bound, void* stream) {
  NSM_CHECK_ARG(y && scale && shift && out && bound && C % 8 == 0 && C <= 2048 && ldy % 8 == 0 &&
                    (!mask || HW > 0) && ((uintptr_t)out % 16) == 0,
                "bn_act_h2: bad args");
  NSM_CHECK_ARG(M >= 0 && M < (1 << 30), "bn_act_h2: too large");
  if (M == 0) return 0;
  dim3 g, b;
  pix_launch_h2(M, C / 8, g, b);
  hipLaunchKernelGGL(bn_act_h2_kernel, g, b, 0, as_stream(stream), y, ldy, M, C / 8,
                     make_fastdiv(mask ? HW : 1), scale, shift, slope, mask, (bf16_t*)out,
                     H2Scale{bound, 1.f});
  NSM_LAUNCH_CHECK("bn_act_h2");
  return 0;
}

extern "C" int nsm_bn_bwd_reduce(const void* g, int ldg, const void* y, int ldy, int M, int C,
                                 int HW, const float* scale, const float* shift, float slope,
                                 const float* mask, const float* mean, const float* invstd,
                                 float* partial, int nchunk, int dtype, uint32_t* amax_k1dz,
                                 void* stream) {
  NSM_CHECK_ARG(g && y && scale && shift && mean && invstd && partial && C % 8 == 0 &&
                    ldg % 8 == 0 && ldy % 8 == 0, "bn_bwd_reduce: bad args");
  ColRed r = colred_plan(M, C);
  NSM_CHECK_ARG(nchunk == r.nchunk, "bn_bwd_reduce: nchunk mismatch");
  dim3 gr(r.gx, r.nchunk);
  return for_dtype(dtype, "bn_bwd_reduce", [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<T>, gr, dim3(256), 0, as_stream(stream), (const T*)g,
                       ldg, (const T*)y, ldy, M, C, make_fastdiv(HW), scale, shift, slope, mask,
                       mean, invstd, r.cl, r.rl, r.rpc, partial, amax_k1dz);
    NSM_LAUNCH_CHECK("bn_bwd_reduce");
    return 0;
  });
}

extern "C" int nsm_bn_bwd_finalize(const float* partial, int nchunk, int M, int C, int c_real,
                                   const float* gamma, const float* invstd, float* dgamma,
                                   float* dbeta, float* dbias_prev, float* coef,
                                   const uint32_t* amax_k1dz, uint32_t* bound, void* stream) {
  NSM_CHECK_ARG(partial && gamma && invstd && coef, "bn_bwd_finalize: bad args");
  NSM_CHECK_ARG(!bound || amax_k1dz, "bn_bwd_finalize: a bound needs the max|k1 dz| slot");
  NSM_CHECK_ARG(M > 1 || !bound, "bn_bwd_finalize: M");
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(256), 0,
                     as_stream(stream), partial, nchunk, M, C, c_real, gamma, invstd, dgamma, dbeta,
                     dbias_prev, coef, amax_k1dz, bound);
  NSM_LAUNCH_CHECK("bn_bwd_finalize");
  return 0;
}

extern "C" int nsm_bn_bwd_apply(const void* g, int ldg, const void* y, int ldy, int M, int C,
                                int HW, const float* scale, const float* shift, float slope,
                                const float* mask, const float* mean, const float* coef, void* dy,
                                int lddy, int dtype, uint32_t* amax, void* stream) {
  NSM_CHECK_ARG(g && y && scale && shift && mean && coef && dy && C % 8 == 0 && C <= 2048 &&
                    ldg % 8 == 0 && ldy % 8 == 0 && lddy % 8 == 0 && (!mask || HW > 0),
                "bn_bwd_apply: bad args");
  NSM_CHECK_ARG(M >= 0 && M < (1 << 30), "bn_bwd_apply: too large");
  if (M == 0) return 0;
  dim3 gr, b;
  pix_launch(M, C / 8, gr, b);
  const FastDiv fh = make_fastdiv(mask ? HW : 1);
  return for_dtype(dtype, "bn_bwd_apply", [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, gr, b, 0, as_stream(stream), (const T*)g, ldg,
                       (const T*)y, ldy, M, C, C / 8, fh, scale, shift, slope, mask, mean, coef,
                       (T*)dy, lddy, amax);
    NSM_LAUNCH_CHECK("bn_bwd_apply");
    return 0;
  });
}

extern "C" int nsm_bn_bwd_apply_h2(const float* g, int ldg, const float* y, int ldy, int M, int C,
                                   int HW, const float* scale, const float* shift, float slope,
                                   const float* mask, const float* mean, const float* coef,
                                   void* dy, const uint32_t* bound, void* stream) {
  NSM_CHECK_ARG(g && y && scale && shift && mean && coef && dy && bound && C % 8 == 0 &&
                    C <= 2048 && ldg % 8 == 0 && ldy % 8 == 0 && (!mask || HW > 0) &&
                    ((uintptr_t)dy % 16) == 0,
                "bn_bwd_apply_h2: bad args");
  NSM_CHECK_ARG(M >= 0 && M < (1 << 30), "bn_bwd_apply_h2: too large");
  if (M == 0) return 0;
  dim3 gr, b;
  pix_launch_h2(M, C / 8, gr, b);
  hipLaunchKernelGGL(bn_bwd_apply_h2_kernel, gr, b, 0, as_stream(stream), g, ldg, y, ldy, M, C,
                     C / 8, make_fastdiv(mask ? HW : 1), scale, shift, slope, mask, mean, coef,
                     (bf16_t*)dy, H2Scale{bound, 1.f});
  NSM_LAUNCH_CHECK("bn_bwd_apply_h2");
  return 0;
}
