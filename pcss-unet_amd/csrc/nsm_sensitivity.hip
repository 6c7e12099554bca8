// The paper's feature-sensitivity analysis (§3.2, Eq. 1): which input channels
// does the network's output depend on?
//   S_i = E[ |phi(f_i + eps_i) - phi(f_i)| ] / s_i,  eps_i ~ N(0, s_i) per pixel
//   of channel i only,  s_i = factor * sigma_i;   relative_i = S_i / sum_j S_j
// The host (nsm_amd/sensitivity.py) lays the work out as image slots: the B
// unperturbed images first, then variant (i, r) of image b at slot
//   B + ((i_idx * R + r) * B + b),
// runs them chunk by chunk through one captured eval forward, and needs two
// kernels around each replay:
//   sens_variants: writes the slots [first, first + n) of that plan into the
//     forward's input, planar NCHW fp32: a copy of the image's planes, and on
//     the slot's channel x + z * s_i (the product rounded before the add, so
//     the result is torch's `x[:, i] + z * s` bit for bit). z comes from
//     `noises` ([C', R, B, H, W]) or from gauss_hash keyed by (seed, channel,
//     repeat) with the counter (image, pixel): never by slot or chunk position,
//     so a variant's texture does not depend on the chunking. Slots past the
//     plan (the last chunk's fillers) hold image 0. One writer per element.
//   sens_reduce: per variant slot of the chunk, sum |o - base_b| and
//     sum (o - base_b) over the image's n output elements. A block folds 2048
//     elements in a fixed tree (8 per thread pairwise, the wave by xor
//     shuffles, the 4 waves pairwise: 11 levels) and stores its two fp32
//     partials to psum[v][block][2]. No atomics: bitwise reproducible.
//   sens_finalize: one block; folds the partials in double in a fixed order into
//     terms[v][2] and the fp64 accumulators acc[i] = {sum |d|, sum d, count},
//     then absolute = acc0 / (count * s_i), signed = acc1 / (count * s_i),
//     relative = absolute / sum absolute from the accumulators.
#include <math.h>
#include "nsm_common.h"

namespace nsm {

constexpr int SV_THREADS = 256;
constexpr int SR_THREADS = 256, SR_ELEMS = SR_THREADS * 8;  // elements of one reduce block

// slot g of the plan -> image b, and for a variant slot its index v, the
// position ii of its channel in the subset and its repeat r (v = -1: base or filler)
struct SensSlot {
  int b, v, ii, r;
};

__device__ __forceinline__ SensSlot sens_slot(int g, int B, int R, int V) {
  SensSlot s{0, -1, 0, 0};
  if (g < B) {
    s.b = g;
  } else if (g - B < V) {
    s.v = g - B;
    const int ir = s.v / B;
    s.b = s.v - ir * B;
    s.ii = ir / R;
    s.r = ir - s.ii * R;
  }
  return s;
}

// grid: x over the plane's pixels (4 per thread), y over the chunk's n * C planes.
// VEC: HW % 4 == 0 and 16-byte aligned buffers, one 16-byte access per thread.
template <bool VEC>
__global__ void __launch_bounds__(SV_THREADS)
    sens_variants_kernel(const float* __restrict__ x, const float* __restrict__ sigma,
                         const int* __restrict__ channels, const float* __restrict__ noises,
                         uint64_t seed, int B, int C, uint32_t HW, int R, int V, float factor,
                         int first, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int j = blockIdx.y / C, c = blockIdx.y - j * C;
  const SensSlot sl = sens_slot(first + j, B, R, V);
  const uint32_t p0 = (blockIdx.x * SV_THREADS + threadIdx.x) * 4u;
  if (p0 >= HW) return;
  const float* src = x + ((size_t)sl.b * C + c) * HW;
  float* dst = out + ((size_t)j * C + c) * HW;
  const int ch = sl.v >= 0 ? (channels ? channels[sl.ii] : sl.ii) : -1;
  const int cnt = VEC ? 4 : (int)min(4u, HW - p0);
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    const f32x4 q = *(const f32x4*)(src + p0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
    for (int k = 0; k < cnt; ++k) v[k] = src[p0 + k];
  }
  if (c == ch) {
    const float s = factor * sigma[ch];  // s_i, formed once in fp32
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (noises) {
      const float* nz = noises + (size_t)sl.v * HW;
      if (VEC) {
        const f32x4 q = *(const f32x4*)(nz + p0);
        z[0] = q.x, z[1] = q.y, z[2] = q.z, z[3] = q.w;
      } else {
        for (int k = 0; k < cnt; ++k) z[k] = nz[p0 + k];
      }
    } else {
      const uint64_t key = seed ^ mix64(((uint64_t)(uint32_t)ch << 32) | (uint32_t)sl.r);
      const uint64_t ctr = (uint64_t)sl.b * HW + p0;
#pragma unroll
      for (int k = 0; k < 4; ++k) z[k] = gauss_hash(key, ctr + k);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float e = z[k] * s;  // rounded before the add
      v[k] = v[k] + e;
    }
  }
  if (VEC) {
    *(f32x4*)(dst + p0) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
    for (int k = 0; k < cnt; ++k) dst[p0 + k] = v[k];
  }
}

// grid: (chunk slots) * per blocks; block blk of slot j folds the elements
// [blk * SR_ELEMS, (blk + 1) * SR_ELEMS) of the image's n: thread t the two
// quads at t * 4 and SR_ELEMS / 2 + t * 4 (0 past the end).
template <bool VEC>
__global__ void __launch_bounds__(SR_THREADS)
    sens_reduce_kernel(const float* __restrict__ out, const float* __restrict__ base, int first,
                       int B, int V, uint32_t n, int per, float* __restrict__ psum) {
#pragma clang fp contract(off)
  __shared__ float sha[SR_THREADS / 64], shd[SR_THREADS / 64];
  const int j = blockIdx.x / per, blk = blockIdx.x - j * per;
  const int g = first + j;
  if (g < B || g - B >= V) return;  // a base or filler slot: uniform over the block
  const int v = g - B, b = v % B;
  const float* o = out + (size_t)j * n;
  const float* q = base + (size_t)b * n;
  float d[8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t e0 = (uint32_t)blk * SR_ELEMS + h * (SR_ELEMS / 2) + threadIdx.x * 4u;
    if (VEC) {
      f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, c = a;
      if (e0 < n) {
        a = *(const f32x4*)(o + e0);
        c = *(const f32x4*)(q + e0);
      }
      const f32x4 t = a - c;
      d[4 * h] = t.x, d[4 * h + 1] = t.y, d[4 * h + 2] = t.z, d[4 * h + 3] = t.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) d[4 * h + k] = e0 + k < n ? o[e0 + k] - q[e0 + k] : 0.f;
    }
  }
  float sa = ((fabsf(d[0]) + fabsf(d[1])) + (fabsf(d[2]) + fabsf(d[3]))) +
             ((fabsf(d[4]) + fabsf(d[5])) + (fabsf(d[6]) + fabsf(d[7])));
  float sd = ((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7]));
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    sa += __shfl_xor(sa, w, 64);
    sd += __shfl_xor(sd, w, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sha[threadIdx.x >> 6] = sa;
    shd[threadIdx.x >> 6] = sd;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* p = psum + ((size_t)v * per + blk) * 2;
    p[0] = (sha[0] + sha[1]) + (sha[2] + sha[3]);
    p[1] = (shd[0] + shd[1]) + (shd[2] + shd[3]);
  }
}

// One block. Wave w folds the channels w, w + 4, ...: per variant (r, b) the
// per-block partials over its lanes, in double, then the variants in order.
__global__ void __launch_bounds__(SR_THREADS)
    sens_finalize_kernel(const float* __restrict__ psum, int Cs, int R, int B, int per,
                         double count, const float* __restrict__ sigma,
                         const int* __restrict__ channels, float factor, float* __restrict__ terms,
                         double* acc, float* __restrict__ absolute, float* __restrict__ sgn,
                         float* __restrict__ relative) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int RB = R * B;
  for (int i = wave; i < Cs; i += SR_THREADS / 64) {
    double ca = 0.0, cd = 0.0;
    for (int rb = 0; rb < RB; ++rb) {
      const size_t v = (size_t)i * RB + rb;
      const float* p = psum + v * per * 2;
      double a = 0.0, d = 0.0;
      for (int k = lane; k < per; k += 64) {
        a += (double)p[2 * k];
        d += (double)p[2 * k + 1];
      }
#pragma unroll
      for (int w = 32; w > 0; w >>= 1) {
        a += __shfl_xor(a, w, 64);
        d += __shfl_xor(d, w, 64);
      }
      if (lane == 0 && terms) {
        terms[2 * v] = (float)a;
        terms[2 * v + 1] = (float)d;
      }
      ca += a;
      cd += d;
    }
    if (lane == 0) {
      acc[3 * i] += ca;
      acc[3 * i + 1] += cd;
      acc[3 * i + 2] += count;
    }
  }
  __syncthreads();  // the accumulators of every channel are written
  double total = 0.0;  // the same sum, in the same order, in every thread
  for (int i = 0; i < Cs; ++i) {
    const double s = (double)(factor * sigma[channels ? channels[i] : i]);
    total += acc[3 * i] / (acc[3 * i + 2] * s);
  }
  for (int i = threadIdx.x; i < Cs; i += SR_THREADS) {
    const double s = (double)(factor * sigma[channels ? channels[i] : i]);
    const double den = acc[3 * i + 2] * s;
    const double S = acc[3 * i] / den;
    absolute[i] = (float)S;
    sgn[i] = (float)(acc[3 * i + 1] / den);
    relative[i] = (float)(S / total);
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// every slot index, variant index and plane offset of a chunk stays in an int
static bool sens_plan_ok(int B, int Cs, int R) {
  return B > 0 && Cs > 0 && R > 0 && (long long)B * (1 + (long long)Cs * R) < (1ll << 31);
}

}  // namespace nsm

using namespace nsm;

extern "C" int nsm_sens_blocks(int64_t n) {
  if (n <= 0 || n > (1ll << 31) - SR_ELEMS) return 0;
  return ceil_div(n, SR_ELEMS);
}

extern "C" int nsm_sens_variants(const float* x, const float* sigma, const int* channels,
                                 const float* noises, uint64_t seed, int B, int C, int H, int W,
                                 int Cs, int R, float factor, int first, int n, float* out,
                                 void* stream) {
  NSM_CHECK_ARG(x && sigma && out, "sens_variants: null pointer");
  NSM_CHECK_ARG(C > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31) && sens_plan_ok(B, Cs, R),
                "sens_variants: shape %d x %d x %d x %d, %d channels x %d repeats", B, C, H, W, Cs,
                R);
  NSM_CHECK_ARG(Cs <= C || channels, "sens_variants: %d channels of %d without a subset", Cs, C);
  NSM_CHECK_ARG(factor > 0.f && first >= 0 && n > 0 && (long long)n * C <= 65535 &&
                    (long long)first + n < (1ll << 31),
                "sens_variants: factor %g, slots [%d, %d + %d), %d planes per slot", (double)factor,
                first, first, n, C);
  const uint32_t HW = (uint32_t)H * W;
  const int V = Cs * R * B;
  const dim3 grid(ceil_div(ceil_div(HW, 4), SV_THREADS), n * C);
  const bool vec = HW % 4 == 0 && aligned16(x) && aligned16(out) && (!noises || aligned16(noises));
  if (vec)
    hipLaunchKernelGGL(sens_variants_kernel<true>, grid, dim3(SV_THREADS), 0, as_stream(stream), x,
                       sigma, channels, noises, seed, B, C, HW, R, V, factor, first, out);
  else
    hipLaunchKernelGGL(sens_variants_kernel<false>, grid, dim3(SV_THREADS), 0, as_stream(stream),
                       x, sigma, channels, noises, seed, B, C, HW, R, V, factor, first, out);
  NSM_LAUNCH_CHECK("sens_variants");
  return 0;
}

extern "C" int nsm_sens_reduce(const float* out, const float* base, int first, int n_slots, int B,
                               int Cs, int R, int64_t n, float* psum, void* stream) {
  NSM_CHECK_ARG(out && base && psum, "sens_reduce: null pointer");
  const int per = nsm_sens_blocks(n);
  NSM_CHECK_ARG(per > 0 && sens_plan_ok(B, Cs, R) && first >= 0 && n_slots > 0 &&
                    (long long)first + n_slots < (1ll << 31) &&
                    (long long)n_slots * per < (1ll << 31),
                "sens_reduce: slots [%d, %d + %d) of %lld elements", first, first, n_slots,
                (long long)n);
  const bool vec = n % 4 == 0 && aligned16(out) && aligned16(base);
  const int V = Cs * R * B;
  if (vec)
    hipLaunchKernelGGL(sens_reduce_kernel<true>, dim3(n_slots * per), dim3(SR_THREADS), 0,
                       as_stream(stream), out, base, first, B, V, (uint32_t)n, per, psum);
  else
    hipLaunchKernelGGL(sens_reduce_kernel<false>, dim3(n_slots * per), dim3(SR_THREADS), 0,
                       as_stream(stream), out, base, first, B, V, (uint32_t)n, per, psum);
  NSM_LAUNCH_CHECK("sens_reduce");
  return 0;
}

extern "C" int nsm_sens_finalize(const float* psum, int Cs, int R, int B, int64_t n,
                                 const float* sigma, const int* channels, float factor,
                                 float* terms, double* acc, float* absolute, float* sgn,
                                 float* relative, void* stream) {
  NSM_CHECK_ARG(psum && sigma && acc && absolute && sgn && relative,
                "sens_finalize: null pointer");
  const int per = nsm_sens_blocks(n);
  NSM_CHECK_ARG(per > 0 && sens_plan_ok(B, Cs, R) && factor > 0.f,
                "sens_finalize: %d channels x %d repeats x %d images of %lld elements", Cs, R, B,
                (long long)n);
  hipLaunchKernelGGL(sens_finalize_kernel, dim3(1), dim3(SR_THREADS), 0, as_stream(stream), psum,
                     Cs, R, B, per, (double)R * (double)B * (double)n, sigma, channels, factor,
                     terms, acc, absolute, sgn, relative);
  NSM_LAUNCH_CHECK("sens_finalize");
  return 0;
}
