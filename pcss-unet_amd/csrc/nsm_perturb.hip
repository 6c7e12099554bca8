// The perturbation-loss step (the paper's §3.3, Eq. 2; pert_loss.py:7-163): the
// P noisy copies of the input from one pass, and the L1 term plus the P
// perturbation terms as one forward and one backward pass.
//
//   pert_variants: out[i][b][c][p] = x[b][c][p] + (z * std[c]) * factor for the
//     P variants i from one read of x. The product z * std[c] is rounded to
//     fp32, then the multiply by factor and the add are one fused multiply-add:
//     the arithmetic of nsm_perturb's kernel as it is built (nsm_elem.hip, whose
//     unit contracts that expression), written out here with fmaf so that it
//     does not depend on a contraction mode. With the same z the bits are
//     nsm_perturb's. z is noises[i][b][c][p] when given, else
//     gauss_hash(seed ^ mix64(i), (b * C + c) * HW + p): a function of seed,
//     variant, image, channel and pixel, never of P or of the launch geometry.
//     The seed is a kernel argument or, with seed_dev, a device word read by
//     every thread, so a replayed graph draws new noise from a new word.
//     grid: x over the plane's pixels (4 per thread), y over the B * C planes
//     (folded above 65535). One writer per element.
//   pert_loss_partial: block blk folds the elements [blk * PL_ELEMS, + PL_ELEMS)
//     of |o - t| and of each |o - p_i|: o is read once, 8 elements per thread
//     pairwise, the wave by xor shuffles, the 4 waves pairwise (11 levels), and
//     the block stores 1 + P fp32 partials to partial[j * nblk + blk]. No atomics.
//   pert_loss_finalize: one block; wave w folds the terms w, w + 4, ... in double
//     in a fixed order, then thread 0 forms the record.
//   pert_loss_bwd: grad (+)= gs * (c0 * sgn(o - t) + c1 * sum_i sgn(o - p_i)):
//     the signs are whole numbers, so the sum over i is exact; three roundings.
#include <math.h>
#include "nsm_common.h"

namespace nsm {

constexpr int PV_THREADS = 256;
constexpr int PL_THREADS = 256, PL_ELEMS = PL_THREADS * 8;  // elements of one loss block
constexpr int PB_THREADS = 256;

// the P perturbed outputs, by value in the kernel arguments (capturable: no
// device-side pointer table to upload)
struct PertPtrs {
  const float* p[NSM_PERT_MAX];
};

template <bool VEC>
__global__ void __launch_bounds__(PV_THREADS)
    pert_variants_kernel(const float* __restrict__ x, const float* __restrict__ stdv,
                         const float* __restrict__ noises, uint64_t seed,
                         const int64_t* __restrict__ seed_dev, int P, int C, int planes,
                         uint32_t HW, float factor, float* __restrict__ out) {
#pragma clang fp contract(off)
  const uint32_t p0 = (blockIdx.x * PV_THREADS + threadIdx.x) * 4u;
  if (p0 >= HW) return;
  if (seed_dev) seed = (uint64_t)seed_dev[0];
  const size_t total = (size_t)planes * HW;
  const int cnt = VEC ? 4 : (int)min(4u, HW - p0);
  for (int plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    const float s = stdv[plane % C];
    const size_t e0 = (size_t)plane * HW + p0;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
      const f32x4 q = *(const f32x4*)(x + e0);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
      for (int k = 0; k < cnt; ++k) v[k] = x[e0 + k];
    }
    for (int i = 0; i < P; ++i) {
      float z[4] = {0.f, 0.f, 0.f, 0.f};
      if (noises) {
        const float* nz = noises + (size_t)i * total + e0;
        if (VEC) {
          const f32x4 q = *(const f32x4*)nz;
          z[0] = q.x, z[1] = q.y, z[2] = q.z, z[3] = q.w;
        } else {
          for (int k = 0; k < cnt; ++k) z[k] = nz[k];
        }
      } else {
        const uint64_t key = seed ^ mix64((uint64_t)(uint32_t)i);
#pragma unroll
        for (int k = 0; k < 4; ++k) z[k] = gauss_hash(key, (uint64_t)e0 + k);
      }
      float r[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float e = z[k] * s;  // rounded before the fused multiply-add
        r[k] = fmaf(e, factor, v[k]);
      }
      float* dst = out + (size_t)i * total + e0;
      if (VEC) {
        *(f32x4*)dst = f32x4{r[0], r[1], r[2], r[3]};
      } else {
        for (int k = 0; k < cnt; ++k) dst[k] = r[k];
      }
    }
  }
}

// 8 elements of one thread: the quads at e0 (h = 0) and e0 + PL_ELEMS / 2
template <bool VEC>
__device__ __forceinline__ void pl_load8(const float* __restrict__ a, uint32_t blk, uint32_t n,
                                         float* d) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t e0 = blk * PL_ELEMS + h * (PL_ELEMS / 2) + threadIdx.x * 4u;
    if (VEC) {
      f32x4 q = f32x4{0.f, 0.f, 0.f, 0.f};
      if (e0 < n) q = *(const f32x4*)(a + e0);
      d[4 * h] = q.x, d[4 * h + 1] = q.y, d[4 * h + 2] = q.z, d[4 * h + 3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) d[4 * h + k] = e0 + k < n ? a[e0 + k] : 0.f;
    }
  }
}

// sum |o - a| of the thread's 8 elements, pairwise, then over the wave
__device__ __forceinline__ float pl_fold(const float* o, const float* a) {
#pragma clang fp contract(off)
  float d[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = fabsf(o[k] - a[k]);
  float s = ((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7]));
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w, 64);
  return s;
}

template <bool VEC>
__global__ void __launch_bounds__(PL_THREADS)
    pert_loss_partial_kernel(const float* __restrict__ o, const float* __restrict__ t,
                             PertPtrs pp, int P, uint32_t n, float* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ float sh[NSM_PERT_MAX + 1][PL_THREADS / 64];
  const uint32_t blk = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float ov[8], av[8];
  pl_load8<VEC>(o, blk, n, ov);  // past the end both sides read 0: |0 - 0| adds nothing
  pl_load8<VEC>(t, blk, n, av);
  float s = pl_fold(ov, av);
  if (lane == 0) sh[0][wave] = s;
#pragma unroll
  for (int i = 0; i < NSM_PERT_MAX; ++i) {
    if (i < P) {  // uniform over the grid
      pl_load8<VEC>(pp.p[i], blk, n, av);
      s = pl_fold(ov, av);
      if (lane == 0) sh[i + 1][wave] = s;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x <= P) {
    const float* q = sh[threadIdx.x];
    partial[(size_t)threadIdx.x * gridDim.x + blk] = (q[0] + q[1]) + (q[2] + q[3]);
  }
}

__global__ void __launch_bounds__(PL_THREADS)
    pert_loss_finalize_kernel(const float* __restrict__ partial, int nblk, int P, double inv_n,
                              float alpha, float w, const float* __restrict__ vgg,
                              float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double means[NSM_PERT_MAX + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j <= P; j += PL_THREADS / 64) {
    const float* p = partial + (size_t)j * nblk;
    double a = 0.0;
    for (int k = lane; k < nblk; k += 64) a += (double)p[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) means[j] = a * inv_n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ps = 0.0;
    for (int i = 1; i <= P; ++i) {
      ps += means[i];
      out[2 + i] = (float)means[i];
    }
    const double pert = ps / (double)P;
    const double v = vgg ? (double)vgg[0] : 0.0;
    out[0] = (float)means[0];
    out[1] = (float)pert;
    out[2] = (float)((double)alpha * means[0] + (1.0 - (double)alpha) * v + (double)w * pert);
  }
}

__device__ __forceinline__ float pl_sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

template <bool VEC>
__global__ void __launch_bounds__(PB_THREADS)
    pert_loss_bwd_kernel(const float* __restrict__ o, const float* __restrict__ t, PertPtrs pp,
                         int P, uint32_t n, float c0, float c1, const float* __restrict__ gscale,
                         float* __restrict__ grad, int accumulate) {
#pragma clang fp contract(off)
  const uint32_t e0 = (blockIdx.x * PB_THREADS + threadIdx.x) * 4u;
  if (e0 >= n) return;
  const float gs = gscale ? gscale[0] : 1.f;
  const int cnt = VEC ? 4 : (int)min(4u, n - e0);
  float ov[4] = {0.f, 0.f, 0.f, 0.f}, s0[4], sp[4] = {0.f, 0.f, 0.f, 0.f};
  float av[4] = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    const f32x4 q = *(const f32x4*)(o + e0), r = *(const f32x4*)(t + e0);
    ov[0] = q.x, ov[1] = q.y, ov[2] = q.z, ov[3] = q.w;
    av[0] = r.x, av[1] = r.y, av[2] = r.z, av[3] = r.w;
  } else {
    for (int k = 0; k < cnt; ++k) ov[k] = o[e0 + k], av[k] = t[e0 + k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) s0[k] = pl_sgn(ov[k] - av[k]);
#pragma unroll
  for (int i = 0; i < NSM_PERT_MAX; ++i) {
    if (i < P) {
      const float* a = pp.p[i];
      if (VEC) {
        const f32x4 r = *(const f32x4*)(a + e0);
        av[0] = r.x, av[1] = r.y, av[2] = r.z, av[3] = r.w;
      } else {
        for (int k = 0; k < cnt; ++k) av[k] = a[e0 + k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) sp[k] += pl_sgn(ov[k] - av[k]);  // whole numbers: exact
    }
  }
  float g[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float a = c0 * s0[k];  // exact: s0 is -1, 0 or 1
    const float b = c1 * sp[k];
    g[k] = gs * (a + b);
  }
  if (VEC) {
    f32x4 r = f32x4{g[0], g[1], g[2], g[3]};
    if (accumulate) r = *(const f32x4*)(grad + e0) + r;
    *(f32x4*)(grad + e0) = r;
  } else {
    for (int k = 0; k < cnt; ++k) grad[e0 + k] = accumulate ? grad[e0 + k] + g[k] : g[k];
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// copies and checks the host pointer array; vec: every one is 16-byte aligned
static bool pert_ptrs(const float* const* pouts, int P, PertPtrs& pp, bool& vec) {
  for (int i = 0; i < NSM_PERT_MAX; ++i) pp.p[i] = nullptr;
  for (int i = 0; i < P; ++i) {
    if (!pouts[i]) return false;
    pp.p[i] = pouts[i];
    vec = vec && aligned16(pouts[i]);
  }
  return true;
}

}  // namespace nsm

using namespace nsm;

extern "C" int nsm_perturb_variants(const float* x, const float* stdv, const float* noises,
                                    uint64_t seed, const int64_t* seed_dev, int P, int B, int C,
                                    int H, int W, float factor, float* out, void* stream) {
  NSM_CHECK_ARG(x && stdv && out, "perturb_variants: null pointer");
  NSM_CHECK_ARG(P >= 1 && P <= NSM_PERT_MAX, "perturb_variants: %d variants (1..%d)", P,
                NSM_PERT_MAX);
  NSM_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31) - 4 &&
                    (long long)B * C < (1ll << 31),
                "perturb_variants: shape %d x %d x %d x %d", B, C, H, W);
  const uint32_t HW = (uint32_t)H * W;
  const int planes = B * C;
  const dim3 grid(ceil_div(ceil_div(HW, 4), PV_THREADS), planes < 65535 ? planes : 65535);
  const bool vec = HW % 4 == 0 && aligned16(x) && aligned16(out) && (!noises || aligned16(noises));
  if (vec)
    hipLaunchKernelGGL(pert_variants_kernel<true>, grid, dim3(PV_THREADS), 0, as_stream(stream),
                       x, stdv, noises, seed, seed_dev, P, C, planes, HW, factor, out);
  else
    hipLaunchKernelGGL(pert_variants_kernel<false>, grid, dim3(PV_THREADS), 0, as_stream(stream),
                       x, stdv, noises, seed, seed_dev, P, C, planes, HW, factor, out);
  NSM_LAUNCH_CHECK("perturb_variants");
  return 0;
}

extern "C" int nsm_pert_loss_blocks(int64_t n) {
  if (n <= 0 || n > (1ll << 31) - PL_ELEMS) return 0;
  return ceil_div(n, PL_ELEMS);
}

extern "C" int nsm_pert_loss_fwd(const float* o, const float* t, const float* const* pouts, int P,
                                 int64_t n, float alpha, float w, const float* vgg,
                                 float* partial, float* out, void* stream) {
  NSM_CHECK_ARG(o && t && pouts && partial && out, "pert_loss_fwd: null pointer");
  NSM_CHECK_ARG(P >= 1 && P <= NSM_PERT_MAX, "pert_loss_fwd: %d perturbed outputs (1..%d)", P,
                NSM_PERT_MAX);
  const int nb = nsm_pert_loss_blocks(n);
  NSM_CHECK_ARG(nb > 0, "pert_loss_fwd: %lld elements", (long long)n);
  PertPtrs pp;
  bool vec = n % 4 == 0 && aligned16(o) && aligned16(t);
  NSM_CHECK_ARG(pert_ptrs(pouts, P, pp, vec), "pert_loss_fwd: null perturbed output");
  hipStream_t s = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(pert_loss_partial_kernel<true>, dim3(nb), dim3(PL_THREADS), 0, s, o, t, pp,
                       P, (uint32_t)n, partial);
  else
    hipLaunchKernelGGL(pert_loss_partial_kernel<false>, dim3(nb), dim3(PL_THREADS), 0, s, o, t,
                       pp, P, (uint32_t)n, partial);
  NSM_LAUNCH_CHECK("pert_loss_fwd");
  hipLaunchKernelGGL(pert_loss_finalize_kernel, dim3(1), dim3(PL_THREADS), 0, s, partial, nb, P,
                     1.0 / (double)n, alpha, w, vgg, out);
  NSM_LAUNCH_CHECK("pert_loss_finalize");
  return 0;
}

extern "C" int nsm_pert_loss_bwd(const float* o, const float* t, const float* const* pouts, int P,
                                 int64_t n, float alpha, float w, const float* gscale,
                                 float* grad, int accumulate, void* stream) {
  NSM_CHECK_ARG(o && t && pouts && grad, "pert_loss_bwd: null pointer");
  NSM_CHECK_ARG(P >= 1 && P <= NSM_PERT_MAX, "pert_loss_bwd: %d perturbed outputs (1..%d)", P,
                NSM_PERT_MAX);
  NSM_CHECK_ARG(nsm_pert_loss_blocks(n) > 0, "pert_loss_bwd: %lld elements", (long long)n);
  PertPtrs pp;
  bool vec = n % 4 == 0 && aligned16(o) && aligned16(t) && aligned16(grad);
  NSM_CHECK_ARG(pert_ptrs(pouts, P, pp, vec), "pert_loss_bwd: null perturbed output");
  // formed in double, rounded to fp32 once
  const float c0 = (float)((double)alpha / (double)n);
  const float c1 = (float)((double)w / ((double)P * (double)n));
  const dim3 grid(ceil_div(ceil_div(n, 4), PB_THREADS));
  if (vec)
    hipLaunchKernelGGL(pert_loss_bwd_kernel<true>, grid, dim3(PB_THREADS), 0, as_stream(stream),
                       o, t, pp, P, (uint32_t)n, c0, c1, gscale, grad, accumulate);
  else
    hipLaunchKernelGGL(pert_loss_bwd_kernel<false>, grid, dim3(PB_THREADS), 0, as_stream(stream),
                       o, t, pp, P, (uint32_t)n, c0, c1, gscale, grad, accumulate);
  NSM_LAUNCH_CHECK("pert_loss_bwd");
  return 0;
}
