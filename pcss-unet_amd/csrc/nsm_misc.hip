// Small boundary kernels of the drop-in surface:
//  * NCHW <-> NHWC layout changes for a standalone DoubleConv call
//    (Unetmodel.py:32-33: `DoubleConv.forward(x)` on an NCHW tensor), tiled
//    through LDS so both the NCHW rows and the NHWC pixel vectors are coalesced;
//  * the output-range assertion of CustomLoss / PerturbationLoss
//    (customLoss.py:131, pert_loss.py:131: min >= 0 and max <= 1, NaN fails)
//    as a sticky device flag, so the check costs no host synchronisation;
//  * max|x| of a tensor (nsm_absmax*: the scale source of a GEMM operand whose
//    producer does not record it) and the counter-calibration launches
//    (nsm_pmc_calib).
#include <algorithm>
#include "nsm_common.h"

namespace nsm {

constexpr int LT_P = 64;  // pixels per tile
constexpr int LT_C = 32;  // channels per tile

// x [B][C][HW] fp32 -> y [B*HW][cp] (T), channels C..cp-1 written as 0.
template <typename T>
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* __restrict__ x, int C,
                                                           int HW, int cp, T* __restrict__ y,
                                                           int ldy) {
  __shared__ float tile[LT_C][LT_P + 1];
  const int b = blockIdx.z, c0 = blockIdx.y * LT_C, p0 = blockIdx.x * LT_P;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 64 x 4
  for (int cc = ty; cc < LT_C; cc += 4) {
    const int c = c0 + cc, p = p0 + tx;
    float v = 0.f;
    if (c < C && p < HW) v = x[((size_t)b * C + c) * HW + p];
    tile[cc][tx] = v;
  }
  __syncthreads();
  const int lc = threadIdx.x & 31, lp = threadIdx.x >> 5;  // 32 x 8
  for (int pp = lp; pp < LT_P; pp += 8) {
    const int p = p0 + pp, c = c0 + lc;
    if (p < HW && c < cp) st1(y + ((size_t)b * HW + p) * ldy + c, tile[lc][pp]);
  }
}

// z [B*HW][ld] (T) -> x [B][C][HW] fp32 (first C channels)
template <typename T>
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const T* __restrict__ z, int ldz, int C,
                                                           int HW, float* __restrict__ x) {
  __shared__ float tile[LT_C][LT_P + 1];
  const int b = blockIdx.z, c0 = blockIdx.y * LT_C, p0 = blockIdx.x * LT_P;
  const int lc = threadIdx.x & 31, lp = threadIdx.x >> 5;
  for (int pp = lp; pp < LT_P; pp += 8) {
    const int p = p0 + pp, c = c0 + lc;
    tile[lc][pp] = (p < HW && c < C) ? ld1(z + ((size_t)b * HW + p) * ldz + c) : 0.f;
  }
  __syncthreads();
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int cc = ty; cc < LT_C; cc += 4) {
    const int c = c0 + cc, p = p0 + tx;
    if (c < C && p < HW) x[((size_t)b * C + c) * HW + p] = tile[cc][tx];
  }
}

// flag[0] = 1 if any o[i] < lo, o[i] > hi or o[i] is NaN; never written 0
__global__ void __launch_bounds__(256) range_flag_kernel(const float* __restrict__ o, int64_t n,
                                                         float lo, float hi, int* flag) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float v = o[i];
    bad |= !(v >= lo && v <= hi);
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) flag[0] = 1;
}

// Dropout2d masks of every block of one forward in ONE launch: job j covers
// rows [B] x channels [cp_j] at offset off_j of `out`; m = (u < keep) / keep
// for c < c_real, 0 in the padded channels; u from a counter-based hash of
// (seed, job, b, c). desc[j] = {offset, c_real, cp, keep (float bits)}.
__device__ __forceinline__ uint32_t hash32(uint64_t x) {
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33;
  return (uint32_t)x;
}

// seed_dev (nsm_dropout_masks_dev): the seed read from device memory, so a
// captured graph draws new masks on every replay (torch's graph-safe generator
// writes it there)
__global__ void __launch_bounds__(256) dropout_masks_kernel(const int* __restrict__ desc, int njobs,
                                                            int B, uint64_t seed,
                                                            float* __restrict__ out,
                                                            const int64_t* __restrict__ seed_dev) {
  const int j = blockIdx.y;
  if (j >= njobs) return;
  if (seed_dev) seed = (uint64_t)seed_dev[0];
  const int off = desc[4 * j], creal = desc[4 * j + 1], cp = desc[4 * j + 2];
  const float keep = __int_as_float(desc[4 * j + 3]);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * cp; i += gridDim.x * blockDim.x) {
    const int c = i % cp, b = i / cp;
    float v = 0.f;
    if (c < creal) {
      const uint32_t h = hash32(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(((uint64_t)j << 40) |
                                                                      ((uint64_t)b << 20) | c));
      const float u = (float)(h >> 8) * (1.f / 16777216.f);  // [0, 1)
      v = u < keep ? 1.f / keep : 0.f;
    }
    out[off + i] = v;
  }
}

// profiling marker (nsm_stage_mark): no work, its grid encodes the stage
__global__ void __launch_bounds__(64) stage_mark_kernel(int code) {}

__global__ void __launch_bounds__(256) zero_u32_kernel(uint32_t* __restrict__ p, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    p[i] = 0u;
}


// max|x| over n floats -> atomic max into the bits at *out (zero it first):
// the scale source of a GEMM operand whose producer does not record it
__global__ void __launch_bounds__(256) absmax_kernel(const float* __restrict__ x, long long n,
                                                     uint32_t* __restrict__ out) {
  uint32_t m = 0;
  const long long n4 = n >> 2;
  const f32x4* x4 = (const f32x4*)x;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4;
       i += (long long)gridDim.x * 256)
    amax_fold(m, x4[i]);
  for (long long i = (n4 << 2) + (long long)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (long long)gridDim.x * 256)
    amax_fold(m, x[i]);
  amax_flush(m, out);
}

// the same over bf16 words (a bf16 value's magnitude bits are the top half of
// its fp32 widening): 8 values per 16-B load
__global__ void __launch_bounds__(256) absmax_bf16_kernel(const bf16_t* __restrict__ x, long long n,
                                                          uint32_t* __restrict__ out) {
  uint32_t m = 0;
  const long long n8 = n >> 3;
  const u32x4* x8 = (const u32x4*)x;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8;
       i += (long long)gridDim.x * 256) {
    const u32x4 w = x8[i];
    amax_fold(m, f32x4{bf_lo(w.x), bf_hi(w.x), bf_lo(w.y), bf_hi(w.y)});
    amax_fold(m, f32x4{bf_lo(w.z), bf_hi(w.z), bf_lo(w.w), bf_hi(w.w)});
  }
  for (long long i = (n8 << 3) + (long long)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (long long)gridDim.x * 256)
    amax_fold(m, __uint_as_float((uint32_t)x[i] << 16));
  amax_flush(m, out);
}

}  // namespace nsm

using namespace nsm;

extern "C" int nsm_stage_mark(int code, void* stream) {
  NSM_CHECK_ARG(code >= 0 && code < 4096, "stage_mark: bad code");
  hipLaunchKernelGGL(stage_mark_kernel, dim3(code + 1), dim3(64), 0, as_stream(stream), code);
  NSM_LAUNCH_CHECK("stage_mark");
  return 0;
}

extern "C" int nsm_zero_u32(uint32_t* p, int64_t n, void* stream) {
  NSM_CHECK_ARG(p && n > 0, "zero_u32: bad args");
  const long long g = std::min<long long>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(zero_u32_kernel, dim3((unsigned)g), dim3(256), 0, as_stream(stream), p,
                     (long long)n);
  NSM_LAUNCH_CHECK("zero_u32");
  return 0;
}

extern "C" int nsm_dropout_masks(const int* desc, int njobs, int B, uint64_t seed, float* out,
                                 void* stream) {
  NSM_CHECK_ARG(desc && out && njobs > 0 && B > 0, "dropout_masks: bad args");
  hipLaunchKernelGGL(dropout_masks_kernel, dim3(8, njobs), dim3(256), 0, as_stream(stream), desc,
                     njobs, B, seed, out, nullptr);
  NSM_LAUNCH_CHECK("dropout_masks");
  return 0;
}

extern "C" int nsm_dropout_masks_dev(const int* desc, int njobs, int B, const int64_t* seed,
                                     float* out, void* stream) {
  NSM_CHECK_ARG(desc && out && seed && njobs > 0 && B > 0, "dropout_masks_dev: bad args");
  hipLaunchKernelGGL(dropout_masks_kernel, dim3(8, njobs), dim3(256), 0, as_stream(stream), desc,
                     njobs, B, 0ull, out, seed);
  NSM_LAUNCH_CHECK("dropout_masks_dev");
  return 0;
}

extern "C" int nsm_nchw_to_nhwc(const float* x, int B, int C, int H, int W, void* y, int cp,
                                int ldy, int dtype, void* stream) {
  NSM_CHECK_ARG(x && y && B > 0 && C > 0 && cp >= C && ldy >= cp && H * W > 0,
                "nchw_to_nhwc: bad args");
  const int HW = H * W;
  dim3 grid((HW + LT_P - 1) / LT_P, (cp + LT_C - 1) / LT_C, B);
  hipStream_t s = as_stream(stream);
  return for_dtype(dtype, "nchw_to_nhwc", [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<T>, grid, dim3(256), 0, s, x, C, HW, cp, (T*)y, ldy);
    NSM_LAUNCH_CHECK("nchw_to_nhwc");
    return 0;
  });
}

extern "C" int nsm_nhwc_to_nchw(const void* z, int ldz, int B, int C, int H, int W, float* x,
                                int dtype, void* stream) {
  NSM_CHECK_ARG(z && x && B > 0 && C > 0 && ldz >= C && H * W > 0, "nhwc_to_nchw: bad args");
  const int HW = H * W;
  dim3 grid((HW + LT_P - 1) / LT_P, (C + LT_C - 1) / LT_C, B);
  hipStream_t s = as_stream(stream);
  return for_dtype(dtype, "nhwc_to_nchw", [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel<T>, grid, dim3(256), 0, s, (const T*)z, ldz, C, HW, x);
    NSM_LAUNCH_CHECK("nhwc_to_nchw");
    return 0;
  });
}

extern "C" int nsm_range_flag(const float* o, int64_t n, float lo, float hi, int* flag,
                              void* stream) {
  NSM_CHECK_ARG(o && flag && n > 0, "range_flag: bad args");
  long long g = (n + 255) / 256;
  if (g > 1024) g = 1024;
  hipLaunchKernelGGL(range_flag_kernel, dim3((int)g), dim3(256), 0, as_stream(stream), o, n, lo, hi,
                     flag);
  NSM_LAUNCH_CHECK("range_flag");
  return 0;
}

extern "C" int nsm_absmax(const float* x, int64_t n, uint32_t* out, void* stream) {
  NSM_CHECK_ARG(x && out && n > 0, "absmax: bad args");
  const long long g = std::min<long long>(ceil_div(n, 1024), 2048);
  hipLaunchKernelGGL(absmax_kernel, dim3((int)g), dim3(256), 0, as_stream(stream), x,
                     (long long)n, out);
  NSM_LAUNCH_CHECK("absmax");
  return 0;
}

extern "C" int nsm_absmax_bf16(const void* x, int64_t n, uint32_t* out, void* stream) {
  NSM_CHECK_ARG(x && out && n > 0 && ((uintptr_t)x % 16) == 0, "absmax_bf16: bad args");
  const long long g = std::min<long long>(ceil_div(n, 2048), 2048);
  hipLaunchKernelGGL(absmax_bf16_kernel, dim3((int)g), dim3(256), 0, as_stream(stream),
                     (const bf16_t*)x, (long long)n, out);
  NSM_LAUNCH_CHECK("absmax_bf16");
  return 0;
}

// ---- PMC calibration (tools/pmc_calib.py) -----------------------------------
// Launches of KNOWN byte counts in the access patterns of this library's
// kernels, so a rocprofv3 counter (WRITE_SIZE, FETCH_SIZE, TCC_EA0_RDREQ*) can
// be read against the bytes it should report before it is used on them
// (MI355X_MICROARCH.md §HBM calibrates only 16-B/lane global loads/stores).
// kind 0: read-only, global_load_dwordx4 (16 B/lane)
//      1: read-only, buffer_load ... lds (LDS-DMA, 16 B/lane; the GEMM loaders)
//      2: write-only, global_store_dwordx4
//      3: write-only, rows staged in LDS then raw_buffer_store_b128 (the
//         persistent h2 GEMM's fp32 epilogue)
//      4: write-only, raw_buffer_store_b64 (its f16-M epilogue)
//      5: write-only, global_store_dword (4 B/lane)
//      6: write-only, global_store_dwordx2 (8 B/lane)
// A read-only kernel writes one dword per block (its checksum) to dst.
__global__ void __launch_bounds__(256) pmc_calib_kernel(int kind, const u32x4* __restrict__ src,
                                                        u32x4* __restrict__ dst, long long n16) {
  typedef __attribute__((address_space(3))) void lds_void;
  __shared__ __attribute__((aligned(16))) bf16_t lds[256 * 8];
  const long long stride = (long long)gridDim.x * 256;
  const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x;
  unsigned acc = 0;
  if (kind == 0) {
    for (long long i = i0; i < n16; i += stride) {
      const u32x4 v = src[i];
      acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
  } else if (kind == 1) {
    // every wave DMAs 64 x 16 B per trip into its own LDS slice
    const __amdgpu_buffer_rsrc_t r =
        __builtin_amdgcn_make_buffer_rsrc((void*)src, (short)0, 0x7FFFFFFF, 0x00020000);
    bf16_t* my = lds + (threadIdx.x >> 6) * 512;
    for (long long b = (long long)blockIdx.x * 256; b < n16; b += stride) {
      // wave-uniform chunk base; the byte offset of this lane's 16 B (< 2 GB)
      const long long wb = b + (threadIdx.x & ~63);
      if (wb < n16) {
        const uint32_t off = (uint32_t)((wb + (threadIdx.x & 63)) * 16);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void*)my, 16, off, 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const u32x4 v = *(const u32x4*)&lds[threadIdx.x * 8];
    acc = v.x ^ v.y ^ v.z ^ v.w;
  } else if (kind == 2) {
    for (long long i = i0; i < n16; i += stride) dst[i] = u32x4{(unsigned)i, 1u, 2u, 3u};
  } else if (kind == 3 || kind == 4) {
    // 16 rows x 64 fp32 per wave staged in LDS (as the epilogue), then the
    // buffer stores of 16 B (kind 3) or of 8 B f16x4 (kind 4) per lane
    float* stg = (float*)lds + (threadIdx.x >> 6) * 256;
    const __amdgpu_buffer_rsrc_t r =
        __builtin_amdgcn_make_buffer_rsrc((void*)dst, (short)0, 0x7FFFFFFF, 0x00020000);
    const long long per = kind == 3 ? 1 : 2;  // lanes per 16 B of output
    const long long nl = n16 * per;           // lane-stores in total
    for (long long i = i0; i < nl; i += stride) {
      stg[(threadIdx.x & 63) * 4 + 0] = (float)i;
      __builtin_amdgcn_wave_barrier();
      const f32x4 v = *(const f32x4*)&stg[(threadIdx.x & 63) * 4];
      if (kind == 3)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (uint32_t)(i * 16), 0,
                                               0);
      else
        __builtin_amdgcn_raw_buffer_store_b64(pack_f16x4(v), r, (uint32_t)(i * 8), 0, 0);
    }
  } else if (kind == 5) {
    unsigned* d = (unsigned*)dst;
    for (long long i = i0; i < n16 * 4; i += stride) d[i] = (unsigned)i;
  } else if (kind == 6) {
    u32x2* d = (u32x2*)dst;
    for (long long i = i0; i < n16 * 2; i += stride) d[i] = u32x2{(unsigned)i, 7u};
  }
  if (kind <= 1) {
    for (int o = 32; o > 0; o >>= 1) acc ^= (unsigned)__shfl_xor((int)acc, o);
    if ((threadIdx.x & 63) == 0 && acc == 0x9E3779B9u) ((unsigned*)dst)[blockIdx.x] = acc;
  }
}

extern "C" int nsm_pmc_calib(int kind, const void* src, void* dst, int64_t bytes, void* stream) {
  NSM_CHECK_ARG(kind >= 0 && kind <= 6 && bytes > 0 && bytes % 4096 == 0 && bytes < (1ll << 31),
                "pmc_calib: kind 0..6, bytes a multiple of 4096 below 2 GB");
  NSM_CHECK_ARG(dst && (kind >= 2 || src), "pmc_calib: null pointer");
  const long long n16 = bytes / 16;
  hipLaunchKernelGGL(pmc_calib_kernel, dim3(2048), dim3(256), 0, as_stream(stream), kind,
                     (const u32x4*)src, (u32x4*)dst, n16);
  NSM_LAUNCH_CHECK("pmc_calib");
  return 0;
}
