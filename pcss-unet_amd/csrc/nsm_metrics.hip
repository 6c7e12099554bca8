// Image-error metrics of the validation pass (main.py:583-664, validate_direct;
// validate_consistency.py:119-120, MSE and PSNR): per image, over the pairs of an
// output o and a target t, one record of 6 doubles
//   {count, sum|d|, sum d^2, max|d|, nonfinite, out_of_range},  d = (double)o - (double)t.
// A pair in which either sample is NaN or +-Inf is counted in `nonfinite` and
// left out of the other five; `out_of_range` counts the o of the remaining pairs
// outside [lo, hi]. A record without a finite pair is {0, 0, 0, 0, k, 0}. Two
// records merge by adding (the maximum by fmax), so every summed term is >= 0
// and any order is within n * 2^-53 relative of the exact sum; the order here
// is fixed, so the same call sequence gives the same bits. No atomics.
//
//   metrics_partial: o, t [B][n] fp32. Block blk of image b covers the elements
//     [blk * MT_SPAN, (blk + 1) * MT_SPAN) of the image and writes
//     records[b * per + blk]. o's span need not start on a 16-byte boundary (an
//     image of 91 floats does only every fourth time): up to 3 head elements reach
//     the next boundary and up to 3 tail elements follow the last whole quad; the
//     threads 0..5 take them one each, and the body of o goes through 16-byte
//     loads. t's body does too where the same element of t sits on a 16-byte
//     boundary (uniform over the block), else through 4-byte loads. A thread's
//     MT_QUADS quads are MT_THREADS quads apart (a wave's load is 1 KiB
//     contiguous); a slot past the body loads quad 0 again, unused, so that no
//     load sits behind a branch. The thread accumulates in fp64 in slot order,
//     the wave folds by shuffles (lane i takes lane i + off: a fixed tree), the
//     4 waves through LDS in order.
//   metrics_merge: one block of MT_MWAVES waves, one wave per image, rounds of
//     MT_MWAVES images. A wave folds the image's `per` records: each lane a
//     contiguous run in index order, the lanes by the same tree. Lane 0 writes
//     the image's record to frames [B][6] and to the log (when given); thread 0
//     then folds the round's images in order into state [6], which persists
//     across batches, and into the batch's own record, from which the batch's
//     L1 joins the accumulator with the criterion's device scalars.
#include <math.h>
#include "nsm_common.h"

namespace nsm {

constexpr int MT_THREADS = 256, MT_QUADS = 8;          // quads of one thread
constexpr int MT_SPAN = MT_THREADS * 4 * MT_QUADS;     // elements of one block: 8192
constexpr int MT_MWAVES = 8, MT_REC = 6;

struct Err {
  double n, s1, s2, mx, bad, oor;
};

__device__ __forceinline__ Err err_empty() { return Err{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

// a then b
__device__ __forceinline__ Err err_merge(const Err& a, const Err& b) {
  return Err{a.n + b.n, a.s1 + b.s1, a.s2 + b.s2, fmax(a.mx, b.mx), a.bad + b.bad, a.oor + b.oor};
}

__device__ __forceinline__ Err err_shfl_down(const Err& a, int off) {
  return Err{__shfl_down(a.n, off, 64),  __shfl_down(a.s1, off, 64),  __shfl_down(a.s2, off, 64),
             __shfl_down(a.mx, off, 64), __shfl_down(a.bad, off, 64), __shfl_down(a.oor, off, 64)};
}

// lane 0 ends with the lanes' records merged in lane order
__device__ __forceinline__ Err err_wave_fold(Err a) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) a = err_merge(a, err_shfl_down(a, off));
  return a;
}

__device__ __forceinline__ Err err_load(const double* p) {
  return Err{p[0], p[1], p[2], p[3], p[4], p[5]};
}
__device__ __forceinline__ void err_store(double* p, const Err& a) {
  p[0] = a.n, p[1] = a.s1, p[2] = a.s2, p[3] = a.mx, p[4] = a.bad, p[5] = a.oor;
}

__device__ __forceinline__ bool mt_finite(float f) { return fabsf(f) < INFINITY; }  // NaN: false

// a thread's running figures: the whole numbers as integers (at most 38 pairs)
struct ErrAcc {
  double s1 = 0.0, s2 = 0.0, mx = 0.0;
  int n = 0, bad = 0, oor = 0;

  __device__ __forceinline__ void add(float o, float t, bool valid, float lo, float hi) {
    const bool fin = mt_finite(o) && mt_finite(t);
    const bool ok = valid && fin;
    const double d = ok ? fabs((double)o - (double)t) : 0.0;
    s1 += d;
    s2 = fma(d, d, s2);
    mx = fmax(mx, d);
    n += ok;
    bad += valid && !fin;
    oor += ok && (o < lo || o > hi);
  }
  __device__ __forceinline__ void add4(f32x4 o, f32x4 t, bool valid, float lo, float hi) {
    add(o.x, t.x, valid, lo, hi);
    add(o.y, t.y, valid, lo, hi);
    add(o.z, t.z, valid, lo, hi);
    add(o.w, t.w, valid, lo, hi);
  }
  __device__ __forceinline__ Err record() const {
    return Err{(double)n, s1, s2, mx, (double)bad, (double)oor};
  }
};

// grid: B * per blocks
__global__ void __launch_bounds__(MT_THREADS)
    metrics_partial_kernel(const float* __restrict__ o, const float* __restrict__ t, int64_t n,
                           int per, float lo, float hi, double* __restrict__ records) {
  __shared__ double sh[MT_THREADS / 64][MT_REC];
  const size_t img = blockIdx.x / (unsigned)per;
  const int blk = (int)(blockIdx.x - img * (unsigned)per);
  const int64_t s0 = (int64_t)blk * MT_SPAN;
  const int len = (int)min((int64_t)MT_SPAN, n - s0);  // >= 1: per = ceil(n / MT_SPAN)
  const float* po = o + img * (size_t)n + s0;
  const float* pt = t + img * (size_t)n + s0;
  const int tid = threadIdx.x;

  // floats up to o's next 16-byte boundary, whole quads, floats after them
  const int head = min((int)((0u - (unsigned)((uintptr_t)po >> 2)) & 3u), len);
  const int nq = (len - head) >> 2;
  const int tail = len - head - 4 * nq;
  const float* bo = po + head;
  const float* bt = pt + head;
  const bool tvec = ((uintptr_t)bt & 15u) == 0;  // uniform over the block

  ErrAcc acc;
  if (nq > 0) {  // uniform
    f32x4 qo[MT_QUADS], qt[MT_QUADS];
    bool ok[MT_QUADS];
#pragma unroll
    for (int k = 0; k < MT_QUADS; ++k) {
      const int i = k * MT_THREADS + tid;  // < MT_SPAN / 4
      ok[k] = i < nq;
      const size_t e = 4 * (size_t)(ok[k] ? i : 0);  // quad 0 exists: nq > 0
      qo[k] = *(const f32x4*)(bo + e);
      if (tvec)
        qt[k] = *(const f32x4*)(bt + e);
      else
        qt[k] = f32x4{bt[e], bt[e + 1], bt[e + 2], bt[e + 3]};
    }
#pragma unroll
    for (int k = 0; k < MT_QUADS; ++k) acc.add4(qo[k], qt[k], ok[k], lo, hi);
  }
  if (tid < head)
    acc.add(po[tid], pt[tid], true, lo, hi);
  else if (tid < head + tail)
    acc.add(po[head + 4 * nq + (tid - head)], pt[head + 4 * nq + (tid - head)], true, lo, hi);

  Err r = err_wave_fold(acc.record());
  if ((tid & 63) == 0) err_store(sh[tid >> 6], r);
  __syncthreads();
  if (tid == 0) {
    Err a = err_load(sh[0]);
#pragma unroll
    for (int w = 1; w < MT_THREADS / 64; ++w) a = err_merge(a, err_load(sh[w]));
    err_store(records + (size_t)blockIdx.x * MT_REC, a);
  }
}

// the criterion's device scalars, by value in the kernel arguments (capturable:
// no device-side pointer table to upload)
struct ScalarPtrs {
  const float* p[NSM_METRICS_SCALARS];
};

// grid: one block of MT_MWAVES waves
__global__ void __launch_bounds__(MT_MWAVES * 64)
    metrics_merge_kernel(const double* __restrict__ records, int B, int per, ScalarPtrs sp, int K,
                         double* __restrict__ frames, double* __restrict__ log,
                         int64_t log_capacity, double* __restrict__ state,
                         double* __restrict__ acc) {
  __shared__ double sh[MT_MWAVES][MT_REC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int run = (per + 63) / 64;  // records of one lane, contiguous
  // images seen before this batch: a whole number below 2^53; read by lane 0 of
  // each wave before thread 0 rewrites it behind the last barrier
  int64_t seen = 0;
  if (acc && log && lane == 0) seen = (int64_t)acc[2 + K];
  Err total = err_empty(), batch = err_empty();
  if (threadIdx.x == 0) total = err_load(state);
  for (int b0 = 0; b0 < B; b0 += MT_MWAVES) {
    const int b = b0 + wave;
    if (b < B) {  // uniform over the wave
      const double* r = records + (size_t)b * per * MT_REC;
      Err a = err_empty();
      for (int k = lane * run; k < min(per, (lane + 1) * run); ++k)
        a = err_merge(a, err_load(r + (size_t)k * MT_REC));
      a = err_wave_fold(a);
      if (lane == 0) {
        err_store(sh[wave], a);
        if (frames) err_store(frames + (size_t)b * MT_REC, a);
        if (acc && log && seen + b < log_capacity) err_store(log + (size_t)(seen + b) * MT_REC, a);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 0; w < min(MT_MWAVES, B - b0); ++w) {
        const Err f = err_load(sh[w]);
        total = err_merge(total, f);
        batch = err_merge(batch, f);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    err_store(state, total);
    if (acc) {
      acc[0] += 1.0;
#pragma unroll
      for (int k = 0; k < NSM_METRICS_SCALARS; ++k)
        if (k < K) acc[1 + k] += (double)sp.p[k][0];
      acc[1 + K] += batch.n > 0.0 ? batch.s1 / batch.n : (double)NAN;
      acc[2 + K] += (double)B;
    }
  }
}

}  // namespace nsm

using namespace nsm;

extern "C" int nsm_metrics_blocks(int64_t n) {
  if (n < 1 || n >= (1ll << 31)) return 0;
  return ceil_div(n, MT_SPAN);
}

extern "C" int nsm_metrics_partial(const float* o, const float* t, int B, int64_t n, float lo,
                                   float hi, double* records, void* stream) {
  NSM_CHECK_ARG(o && t && records, "metrics_partial: null pointer");
  const int per = nsm_metrics_blocks(n);
  NSM_CHECK_ARG(B > 0 && per > 0 && (long long)B * per < (1ll << 31),
                "metrics_partial: shape %d x %lld", B, (long long)n);
  NSM_CHECK_ARG((((uintptr_t)o | (uintptr_t)t) & 3u) == 0,
                "metrics_partial: o or t is not 4-byte aligned");
  NSM_CHECK_ARG(lo <= hi, "metrics_partial: range [%g, %g]", (double)lo, (double)hi);
  hipLaunchKernelGGL(metrics_partial_kernel, dim3((unsigned)(B * per)), dim3(MT_THREADS), 0,
                     as_stream(stream), o, t, n, per, lo, hi, records);
  NSM_LAUNCH_CHECK("metrics_partial");
  return 0;
}

extern "C" int nsm_metrics_merge(const double* records, int B, int per,
                                 const float* const* scalars, int K, double* frames, double* log,
                                 int64_t log_capacity, double* state, double* acc, void* stream) {
  NSM_CHECK_ARG(records && state, "metrics_merge: null pointer");
  NSM_CHECK_ARG(B > 0 && per > 0 && (long long)B * per < (1ll << 31),
                "metrics_merge: %d images x %d records", B, per);
  NSM_CHECK_ARG(K >= 0 && K <= NSM_METRICS_SCALARS && (K == 0 || (scalars && acc)),
                "metrics_merge: %d scalars (0..%d, with an accumulator)", K, NSM_METRICS_SCALARS);
  NSM_CHECK_ARG(log_capacity >= 0 && (!log || log_capacity == 0 || acc),
                "metrics_merge: a log of %lld images needs an accumulator",
                (long long)log_capacity);
  ScalarPtrs sp;
  for (int k = 0; k < NSM_METRICS_SCALARS; ++k) sp.p[k] = nullptr;
  for (int k = 0; k < K; ++k) {
    NSM_CHECK_ARG(scalars[k], "metrics_merge: null scalar %d", k);
    sp.p[k] = scalars[k];
  }
  if (log_capacity == 0) log = nullptr;
  hipLaunchKernelGGL(metrics_merge_kernel, dim3(1), dim3(MT_MWAVES * 64), 0, as_stream(stream),
                     records, B, per, sp, K, frames, log, (int64_t)log_capacity, state, acc);
  NSM_LAUNCH_CHECK("metrics_merge");
  return 0;
}
