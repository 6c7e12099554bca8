// What the frame passes share (nsm_frame.hip, nsm_features.hip): the scrub and
// the census. A pass runs blocks of FR_THREADS threads, each block writes three
// counts to its own slot of a partial buffer, and frame_census adds an image's
// slots in a fixed order: whole numbers, no atomics, no second pass over the frame.
#pragma once
#include "nsm_common.h"

namespace nsm {

constexpr int FR_THREADS = 256;

// torch.nan_to_num(nan=0.0, posinf=1.0, neginf=0.0): selects only, so every
// finite value (-0.0, denormals, FLT_MAX) keeps its bits
__device__ __forceinline__ float frame_scrub(float v) {
  const uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) < 0x7f800000u) return v;
  return u == 0x7f800000u ? 1.f : 0.f;
}

// the three counts of a block -> part[0..2]; every thread of the block calls
__device__ __forceinline__ void frame_block_counts(uint32_t a, uint32_t b, uint32_t c,
                                                   uint32_t* __restrict__ part) {
  __shared__ uint32_t sh[FR_THREADS / 64][3];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
    c += __shfl_down(c, off, 64);
  }
  const int t = threadIdx.x;
  if ((t & 63) == 0) sh[t >> 6][0] = a, sh[t >> 6][1] = b, sh[t >> 6][2] = c;
  __syncthreads();
  if (t < 3) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < FR_THREADS / 64; ++w) s += sh[w][t];
    part[t] = s;
  }
}

// grid: B blocks. report[b][off .. off + 2] = the sums of image b's `per` triples
static __global__ void __launch_bounds__(FR_THREADS)
    frame_census_kernel(const uint32_t* __restrict__ part, int per, int off,
                        int32_t* __restrict__ report) {
  const uint32_t* p = part + (size_t)blockIdx.x * per * 3;
  uint32_t s[3] = {0, 0, 0};
  for (int i = threadIdx.x; i < per; i += FR_THREADS) {
    s[0] += p[3 * i], s[1] += p[3 * i + 1], s[2] += p[3 * i + 2];
  }
  frame_block_counts(s[0], s[1], s[2], (uint32_t*)report + (size_t)blockIdx.x * 6 + off);
}

static void frame_census(const uint32_t* part, int B, int per, int off, int32_t* report,
                         hipStream_t st) {
  hipLaunchKernelGGL(frame_census_kernel, dim3((unsigned)B), dim3(FR_THREADS), 0, st, part, per,
                     off, report);
}

}  // namespace nsm
