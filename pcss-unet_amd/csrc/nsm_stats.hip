// Per-channel dataset statistics of raw input frames (what FrameLoader and
// MmapLiverDataset normalise with, and the sigma of the paper's Eq. 1): count,
// mean, variance, min, max and the number of non-finite samples of every
// channel, over every pixel of every frame fed in, in one read of each batch.
//
// A record is 6 doubles: {count, mean, M2, min, max, nonfinite}. count and
// nonfinite are whole numbers; M2 is the sum of squared deviations from the
// record's own mean; a record of no finite sample is {0, 0, 0, +inf, -inf, k}.
// Non-finite samples are counted and left out of the other five. Two records
// merge by Chan's rule (mean += d * nb / n, M2 += M2b + d^2 * na * nb / n), which
// never subtracts two large sums, so the result does not cancel however far the
// channel sits from zero.
//
//   stats_partial: x [B][C][HW] fp32 as nsm_loader_next delivers it. Block blk of
//     plane (b, c) covers the elements [blk * ST_SPAN, (blk + 1) * ST_SPAN) of the
//     plane and writes records[(b * C + c) * per + blk]. The span's address need
//     not be 16-byte aligned (a plane of 130 floats is only every other time): up
//     to 3 head elements reach the next 16-byte boundary and up to 3 tail elements
//     follow the last whole quad; the threads 0..5 take them one each, and the
//     body goes through 16-byte loads. A thread folds a tile of 4 quads (stride
//     ST_THREADS quads, so a wave's load is 1 KiB contiguous) in two sweeps over
//     its registers: the fp64 sum and the mean, then the squared deviations from
//     that mean (a whole tile of finite samples, told by one unsigned maximum,
//     takes a path without selects); its 8 tiles, then the ragged element, merge
//     by Chan's rule, the wave by shuffles (lane i takes lane i + off: a fixed
//     tree), the 4 waves through LDS in order. No atomics. Where both sides of a
//     merge hold counts in a known ratio (tile k + 1 against k tiles, the two
//     halves of a tree level) the quotient nb / n is a constant and the fp64
//     division, most of a merge's instructions, is skipped; the bits are the same.
//   stats_merge: one block per channel, one wave per frame, rounds of ST_MWAVES
//     frames. A wave folds the plane's `per` records: each lane a contiguous run
//     in index order, the lanes by the same tree of neighbours. Lane 0 writes the
//     frame's record to frames [B][C][6] (when given); wave 0 then folds the
//     round's frames, a lane each in frame order, by that tree, and merges the
//     round into state [C][6], which persists across batches. The order is
//     fixed, so the same call sequence gives the same bits.
#include <math.h>
#include "nsm_common.h"

namespace nsm {

constexpr int ST_THREADS = 256, ST_TILE = 4;            // quads of one thread's tile
constexpr int ST_TILES = 8;                             // tiles of one thread (even)
constexpr int ST_SPAN = ST_THREADS * 4 * ST_TILE * ST_TILES;  // elements of one block: 32768
constexpr int ST_MWAVES = 8, ST_REC = 6;
static_assert(ST_TILES <= 8 && ST_TILES % 2 == 0, "ST_RCP holds 1 / (k + 1) up to k = 7");

// 1 / (k + 1), correctly rounded (the compiler's constant division)
__constant__ const double ST_RCP[8] = {1.0, 1.0 / 2, 1.0 / 3, 1.0 / 4, 1.0 / 5, 1.0 / 6, 1.0 / 7, 1.0 / 8};

struct Mom {
  double n, mean, m2, mn, mx, bad;
};

__device__ __forceinline__ Mom mom_empty() {
  return Mom{0.0, 0.0, 0.0, (double)INFINITY, (double)-INFINITY, 0.0};
}

// a then b. An empty a gives b's mean and M2 bit for bit (r = 1, a.mean = 0), an
// empty b leaves a's (r = 0), and two empty records stay empty.
// When a holds k times b's count, b.n / n is 1 / (k + 1): the caller passes that
// quotient, correctly rounded, as rk. It and the two empty cases are the bits
// the division would give, and a wave whose lanes all qualify skips the
// division: it is most of a merge's cost.
__device__ __forceinline__ Mom mom_merge(const Mom& a, const Mom& b, double k = 1.0,
                                         double rk = 0.5) {
  Mom o;
  o.n = a.n + b.n;
  double r = rk;
  if (b.n == 0.0)
    r = 0.0;
  else if (a.n == 0.0)
    r = 1.0;
  else if (a.n != k * b.n)
    r = b.n / o.n;
  const double d = b.mean - a.mean;
  o.mean = a.mean + d * r;
  o.m2 = a.m2 + b.m2 + d * d * a.n * r;
  o.mn = fmin(a.mn, b.mn);
  o.mx = fmax(a.mx, b.mx);
  o.bad = a.bad + b.bad;
  return o;
}

__device__ __forceinline__ Mom mom_shfl_down(const Mom& a, int off) {
  return Mom{__shfl_down(a.n, off, 64),  __shfl_down(a.mean, off, 64), __shfl_down(a.m2, off, 64),
             __shfl_down(a.mn, off, 64), __shfl_down(a.mx, off, 64),   __shfl_down(a.bad, off, 64)};
}

// lane 0 ends with the lanes' records merged in lane order
__device__ __forceinline__ Mom mom_wave_fold(Mom a) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) a = mom_merge(a, mom_shfl_down(a, off));
  return a;
}

__device__ __forceinline__ Mom mom_load(const double* p) {
  return Mom{p[0], p[1], p[2], p[3], p[4], p[5]};
}
__device__ __forceinline__ void mom_store(double* p, const Mom& a) {
  p[0] = a.n, p[1] = a.mean, p[2] = a.m2, p[3] = a.mn, p[4] = a.mx, p[5] = a.bad;
}

__device__ __forceinline__ bool finite_f(float f) { return fabsf(f) < INFINITY; }  // NaN: false

// one sample as a record
__device__ __forceinline__ Mom mom_of(float f) {
  Mom o = mom_empty();
  if (finite_f(f)) {
    o.n = 1.0, o.mean = (double)f, o.mn = (double)f, o.mx = (double)f;
  } else {
    o.bad = 1.0;
  }
  return o;
}

// the quads q[k] with ok[k] as one record: two sweeps over the registers
__device__ __forceinline__ Mom mom_of_tile(const f32x4 (&q)[ST_TILE], const bool (&ok)[ST_TILE]) {
  constexpr int N = 4 * ST_TILE;
  float v[N];
#pragma unroll
  for (int k = 0; k < ST_TILE; ++k) v[4 * k] = q[k].x, v[4 * k + 1] = q[k].y, v[4 * k + 2] = q[k].z, v[4 * k + 3] = q[k].w;
  uint32_t top = 0;  // fp32 bit patterns of |x| compare as unsigned, Inf and NaN on top
#pragma unroll
  for (int e = 0; e < N; ++e) top = max(top, __float_as_uint(v[e]) & 0x7fffffffu);
  if (ok[ST_TILE - 1] && top < 0x7f800000u) {  // a whole tile of finite samples: no selects
    double s = 0.0;
    float mn = v[0], mx = v[0];
#pragma unroll
    for (int e = 0; e < N; ++e) {
      s += (double)v[e];
      mn = fminf(mn, v[e]);
      mx = fmaxf(mx, v[e]);
    }
    const double mean = s * (1.0 / N);
    double m2 = 0.0;
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const double d = (double)v[e] - mean;
      m2 = fma(d, d, m2);
    }
    return Mom{(double)N, mean, m2, (double)mn, (double)mx, 0.0};
  }
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  int cnt = 0, bad = 0;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const bool fin = ok[e / 4] && finite_f(v[e]);
    bad += ok[e / 4] && !fin;
    cnt += fin;
    s += fin ? (double)v[e] : 0.0;
    mn = fin ? fminf(mn, v[e]) : mn;
    mx = fin ? fmaxf(mx, v[e]) : mx;
  }
  // the sum of 16 floats is exact in fp64 short of a 2^29 spread; a whole tile
  // divides by a power of two
  const double mean = cnt == N ? s * (1.0 / N) : (cnt ? s / (double)cnt : 0.0);
  double m2 = 0.0;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const bool fin = ok[e / 4] && finite_f(v[e]);
    const double d = fin ? (double)v[e] - mean : 0.0;
    m2 = fma(d, d, m2);
  }
  return Mom{(double)cnt, mean, m2, (double)mn, (double)mx, (double)bad};
}

// grid: B * C * per blocks
__global__ void __launch_bounds__(ST_THREADS)
    stats_partial_kernel(const float* __restrict__ x, int64_t HW, int per,
                         double* __restrict__ records) {
  __shared__ double sh[ST_THREADS / 64][ST_REC];
  const size_t plane = blockIdx.x / (unsigned)per;
  const int blk = (int)(blockIdx.x - plane * (unsigned)per);
  const int64_t s0 = (int64_t)blk * ST_SPAN;
  const int len = (int)min((int64_t)ST_SPAN, HW - s0);  // >= 1: per = ceil(HW / ST_SPAN)
  const float* p = x + plane * (size_t)HW + s0;
  const int t = threadIdx.x;

  // floats up to the next 16-byte boundary, whole quads, floats after them
  const int head = min((int)((0u - (unsigned)((uintptr_t)p >> 2)) & 3u), len);
  const int nq = (len - head) >> 2;
  const int tail = len - head - 4 * nq;
  const f32x4* body = (const f32x4*)(p + head);

  // quad slot (it * ST_TILE + k) * ST_THREADS + t: at most ST_SPAN / 4 slots.
  // Tile `it` meets the `it` whole tiles before it: the ratio is 1 / (it + 1).
  // A slot past the body loads the 16-byte granule that holds p[0] instead (in
  // bounds of the same page, value unused), so no load sits behind a branch and
  // the next tile's four loads are in flight while this one is folded.
  const f32x4* safe = (const f32x4*)(p - (((uintptr_t)p >> 2) & 3u));
  auto load = [&](int it, f32x4(&q)[ST_TILE], bool(&ok)[ST_TILE]) {
#pragma unroll
    for (int k = 0; k < ST_TILE; ++k) {
      const int i = (it * ST_TILE + k) * ST_THREADS + t;
      ok[k] = i < nq;
      q[k] = *(ok[k] ? body + i : safe);
    }
  };
  Mom acc = mom_empty();
  auto fold = [&](int it, const f32x4(&q)[ST_TILE], const bool(&ok)[ST_TILE]) {
    if (ok[0]) acc = mom_merge(acc, mom_of_tile(q, ok), (double)it, ST_RCP[it]);  // ok[k] implies ok[0]
  };
  f32x4 qa[ST_TILE], qb[ST_TILE];
  bool oka[ST_TILE], okb[ST_TILE];
  load(0, qa, oka);
#pragma unroll 1
  for (int it = 0; it < ST_TILES && it * ST_TILE * ST_THREADS < nq; it += 2) {  // uniform
    load(it + 1, qb, okb);
    fold(it, qa, oka);
    load(it + 2, qa, oka);  // tile ST_TILES is past every span: four loads of the granule
    fold(it + 1, qb, okb);
  }
  // the ragged elements last, so that they do not unsettle the ratios above
  if (t < head)
    acc = mom_merge(acc, mom_of(p[t]));
  else if (t < head + tail)
    acc = mom_merge(acc, mom_of(p[head + 4 * nq + (t - head)]));

  acc = mom_wave_fold(acc);
  if ((t & 63) == 0) mom_store(sh[t >> 6], acc);
  __syncthreads();
  if (t == 0) {
    Mom o = mom_load(sh[0]);
#pragma unroll
    for (int w = 1; w < ST_THREADS / 64; ++w) o = mom_merge(o, mom_load(sh[w]));
    mom_store(records + (size_t)blockIdx.x * ST_REC, o);
  }
}

// grid: C blocks of ST_MWAVES waves
__global__ void __launch_bounds__(ST_MWAVES * 64)
    stats_merge_kernel(const double* __restrict__ records, int B, int C, int per,
                       double* __restrict__ frames, double* __restrict__ state) {
  __shared__ double sh[ST_MWAVES][ST_REC];
  const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int run = (per + 63) / 64;  // records of one lane, contiguous
  Mom total = mom_empty();
  if (threadIdx.x == 0) total = mom_load(state + (size_t)c * ST_REC);
  for (int b0 = 0; b0 < B; b0 += ST_MWAVES) {
    const int b = b0 + wave;
    if (b < B) {  // uniform over the wave
      const double* r = records + ((size_t)b * C + c) * per * ST_REC;
      Mom a = mom_empty();
      for (int k = lane * run; k < min(per, (lane + 1) * run); ++k)
        a = mom_merge(a, mom_load(r + (size_t)k * ST_REC));
      a = mom_wave_fold(a);
      if (lane == 0) {
        mom_store(sh[wave], a);
        if (frames) mom_store(frames + ((size_t)b * C + c) * ST_REC, a);
      }
    }
    __syncthreads();
    if (wave == 0) {  // the round's frames: lane w holds frame b0 + w
      Mom f = lane < min(ST_MWAVES, B - b0) ? mom_load(sh[lane]) : mom_empty();
      f = mom_wave_fold(f);
      if (lane == 0) total = mom_merge(total, f);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) mom_store(state + (size_t)c * ST_REC, total);
}

}  // namespace nsm

using namespace nsm;

extern "C" int nsm_stats_blocks(int64_t hw) {
  if (hw <= 0 || hw >= (1ll << 31)) return 0;
  return ceil_div(hw, ST_SPAN);
}

extern "C" int nsm_stats_partial(const float* x, int B, int C, int64_t HW, double* records,
                                 void* stream) {
  NSM_CHECK_ARG(x && records, "stats_partial: null pointer");
  const int per = nsm_stats_blocks(HW);
  NSM_CHECK_ARG(B > 0 && C > 0 && per > 0 && (long long)B * C * per < (1ll << 31),
                "stats_partial: shape %d x %d x %lld", B, C, (long long)HW);
  NSM_CHECK_ARG(((uintptr_t)x & 3u) == 0, "stats_partial: x is not 4-byte aligned");
  hipLaunchKernelGGL(stats_partial_kernel, dim3((unsigned)(B * C * per)), dim3(ST_THREADS), 0,
                     as_stream(stream), x, HW, per, records);
  NSM_LAUNCH_CHECK("stats_partial");
  return 0;
}

extern "C" int nsm_stats_merge(const double* records, int B, int C, int per, double* frames,
                               double* state, void* stream) {
  NSM_CHECK_ARG(records && state, "stats_merge: null pointer");
  NSM_CHECK_ARG(B > 0 && C > 0 && per > 0 && (long long)B * C * per < (1ll << 31),
                "stats_merge: %d frames x %d channels x %d records", B, C, per);
  hipLaunchKernelGGL(stats_merge_kernel, dim3(C), dim3(ST_MWAVES * 64), 0, as_stream(stream),
                     records, B, C, per, frames, state);
  NSM_LAUNCH_CHECK("stats_merge");
  return 0;
}
