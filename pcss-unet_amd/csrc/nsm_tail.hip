// Train-step tail of main.py:287-423 on the device, with no host
// synchronisation: gradient sanitising (NaN/Inf census, >20 % skip, repair),
// the per-parameter pre-unscale clip to 1000*scale, the per-parameter 1e5 skip /
// 1e3 rescale, clip_grad_norm_(max_norm), the post-clip max-norm > 10 skip, and
// an AdamW (or Adam, or SGD: main.py:952-957) step that honours the device skip
// flag.
//
// The gradient is ONE flat fp32 buffer holding the module's parameters in
// order; `seg_off[nseg+1]` delimits the parameters ("segments"). Work is cut
// into blocks that never straddle a segment (nsm_tail_plan), so every
// per-parameter statistic is a deterministic fixed-order reduction of
// per-block partials. Decisions the reference takes on the host (`.item()`,
// `continue`) become device flags read by the kernels that follow, so the whole
// tail is a fixed launch sequence (hipGraph-capturable).
//
// Rounding follows the reference's fp32 op sequence: grads are multiplied by the
// pre-clip factor, then the 1e3 rescale, then the clip coefficient (three
// separate fp32 products, exactly like the three mul_ calls), and AdamW is
// torch's single-tensor AdamW. FP contraction is off in this file so no FMA
// merges two of those roundings.
#include <cfloat>
#include <math.h>

#include "nsm_common.h"

#pragma clang fp contract(off)

namespace nsm {

constexpr int TAIL_THREADS = 256;
constexpr int64_t TAIL_CHUNK = 8192;  // elements per block (32 per thread)

// workspace layout (all offsets 8-byte aligned)
struct TailWs {
  double* blk_d;    // [nblk][2]  sum, sumsq of finite values (pre-repair)
  int* blk_i;       // [nblk][2]  nan count, inf count
  float* blk_max;   // [nblk]     max |finite|
  double* rep_d;    // [nblk]     sumsq after repair
  int* rep_i;       // [nblk]     non-finite count after repair
  double* seg_d;    // [nseg][4]  mean, std, maxabs, sumsq
  int* seg_i;       // [nseg][2]  invalid count, zeroed
  int* ctl;         // [4]        0: repair needed, 1: severe
};

static inline size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

static size_t tail_ws_layout(int nseg, int nblk, char* base, TailWs* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t o = off;
    off = align8(off + bytes);
    return base ? base + o : nullptr;
  };
  char* p;
  p = take(sizeof(double) * 2 * nblk);
  if (w) w->blk_d = (double*)p;
  p = take(sizeof(int) * 2 * nblk);
  if (w) w->blk_i = (int*)p;
  p = take(sizeof(float) * nblk);
  if (w) w->blk_max = (float*)p;
  p = take(sizeof(double) * nblk);
  if (w) w->rep_d = (double*)p;
  p = take(sizeof(int) * nblk);
  if (w) w->rep_i = (int*)p;
  p = take(sizeof(double) * 4 * nseg);
  if (w) w->seg_d = (double*)p;
  p = take(sizeof(int) * 2 * nseg);
  if (w) w->seg_i = (int*)p;
  p = take(sizeof(int) * 4);
  if (w) w->ctl = (int*)p;
  return off;
}

__device__ __forceinline__ bool is_finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }

template <typename T>
__device__ __forceinline__ T wave_red_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_red_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// block of 256 threads: sum over the block, result valid in thread 0
template <typename T>
__device__ __forceinline__ T block_red_sum(T v, T* sh) {
  v = wave_red_sum(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) sh[wv] = v;
  __syncthreads();
  T r = 0;
  if (threadIdx.x == 0)
    for (int k = 0; k < TAIL_THREADS / 64; ++k) r += sh[k];
  __syncthreads();
  return r;
}

__device__ __forceinline__ float block_red_max(float v, float* sh) {
  v = wave_red_max(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) sh[wv] = v;
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x == 0)
    for (int k = 0; k < TAIL_THREADS / 64; ++k) r = fmaxf(r, sh[k]);
  __syncthreads();
  return r;
}

// ---- K1: per-block census of the (rank-averaged) gradient --------------------
// main.py:295-312: isnan / isinf counts per parameter; the finite values'
// sum, sum of squares and max |.| feed the repair statistics (:326-346) and the
// per-parameter norm (:365). With inv_world != 1 the DP sum is turned into the
// mean in place first (the tail then sees what a single process would).
__global__ void __launch_bounds__(TAIL_THREADS) tail_stats_kernel(
    float* __restrict__ g, const int64_t* __restrict__ blk_lo, const int64_t* __restrict__ blk_hi,
    float inv_world, TailWs w) {
  __shared__ double shd[4];
  __shared__ int shi[4];
  __shared__ float shf[4];
  const int b = blockIdx.x;
  const int64_t lo = blk_lo[b], hi = blk_hi[b];
  double s = 0.0, s2 = 0.0;
  int nn = 0, ni = 0;
  float mx = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += TAIL_THREADS) {
    float v = g[i];
    if (inv_world != 1.f) {
      v = v * inv_world;
      g[i] = v;
    }
    if (v != v) {
      ++nn;
    } else if (!is_finite_f(v)) {
      ++ni;
    } else {
      s += (double)v;
      s2 += (double)v * (double)v;
      mx = fmaxf(mx, fabsf(v));
    }
  }
  s = block_red_sum(s, shd);
  s2 = block_red_sum(s2, shd);
  nn = block_red_sum(nn, shi);
  ni = block_red_sum(ni, shi);
  mx = block_red_max(mx, shf);
  if (threadIdx.x == 0) {
    w.blk_d[2 * b] = s;
    w.blk_d[2 * b + 1] = s2;
    w.blk_i[2 * b] = nn;
    w.blk_i[2 * b + 1] = ni;
    w.blk_max[b] = mx;
  }
}

// ---- K2: per-parameter statistics + the skip / repair decision ---------------
// One block; wave k reduces segments k, k+16, ... over their blocks in order.
// severe (main.py:305-317): some parameter has (nan+inf)/numel > 0.2 -> skip.
// fixable (:311,320): some parameter has an invalid value -> repair all.
__global__ void __launch_bounds__(1024) tail_decide_kernel(const int64_t* __restrict__ seg_off,
                                                           const int* __restrict__ seg_blk,
                                                           int nseg, TailWs w) {
  __shared__ int sh_sev[16], sh_fix[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int sev = 0, fix = 0;
  for (int sgi = wv; sgi < nseg; sgi += 16) {
    const int b0 = seg_blk[sgi], b1 = seg_blk[sgi + 1];
    double s = 0.0, s2 = 0.0;
    long long nn = 0, ni = 0;
    float mx = 0.f;
    for (int b = b0 + lane; b < b1; b += 64) {
      s += w.blk_d[2 * b];
      s2 += w.blk_d[2 * b + 1];
      nn += w.blk_i[2 * b];
      ni += w.blk_i[2 * b + 1];
      mx = fmaxf(mx, w.blk_max[b]);
    }
    s = wave_red_sum(s);
    s2 = wave_red_sum(s2);
    nn = wave_red_sum(nn);
    ni = wave_red_sum(ni);
    mx = wave_red_max(mx);
    if (lane == 0) {
      const long long numel = seg_off[sgi + 1] - seg_off[sgi];
      const long long bad = nn + ni;
      const long long nv = numel - bad;
      // torch: valid_grads.mean() / .std() (unbiased; 0.01 when one value)
      const double mean = nv > 0 ? s / (double)nv : 0.0;
      double var = nv > 1 ? (s2 - s * mean) / (double)(nv - 1) : 0.0;
      if (var < 0.0) var = 0.0;
      w.seg_d[4 * sgi + 0] = mean;
      w.seg_d[4 * sgi + 1] = nv > 1 ? sqrt(var) : 0.01;
      w.seg_d[4 * sgi + 2] = (double)mx;
      w.seg_d[4 * sgi + 3] = s2;
      w.seg_i[2 * sgi + 0] = (int)(bad < 0x7fffffff ? bad : 0x7fffffff);
      w.seg_i[2 * sgi + 1] = 0;
      if (bad > 0) {
        fix = 1;
        // (nan.sum() + inf.sum()).item() / numel > 0.2, in double as in Python
        if ((double)bad / (double)numel > 0.2) sev = 1;
      }
    }
  }
  if (lane == 0) {
    sh_sev[wv] = sev;
    sh_fix[wv] = fix;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int S = 0, X = 0;
    for (int k = 0; k < 16; ++k) {
      S |= sh_sev[k];
      X |= sh_fix[k];
    }
    w.ctl[0] = (X && !S) ? 1 : 0;  // repair
    w.ctl[1] = S;                  // severe skip
  }
}

// ---- K3: repair (main.py:320-354), only when K2 decided so -------------------
// NaN -> mean + randn * std * 0.1 ; +-Inf -> sign * max|valid| * 10.
// `noise` (optional, flat like g) supplies the randn values for parity tests;
// otherwise a counter-based generator keyed by (seed, step, index) is used.
__global__ void __launch_bounds__(TAIL_THREADS) tail_repair_kernel(
    float* __restrict__ g, const int* __restrict__ blk_seg, const int64_t* __restrict__ blk_lo,
    const int64_t* __restrict__ blk_hi, const float* __restrict__ noise, uint64_t seed,
    const int* __restrict__ step, TailWs w) {
  __shared__ double shd[4];
  __shared__ int shi[4];
  if (w.ctl[0] == 0) return;  // uniform across the grid
  const int b = blockIdx.x, sgi = blk_seg[b];
  const int64_t lo = blk_lo[b], hi = blk_hi[b];
  const float mean = (float)w.seg_d[4 * sgi + 0];
  const float stdv = (float)w.seg_d[4 * sgi + 1];
  const float mx = (float)w.seg_d[4 * sgi + 2];
  // keyed by the tail-call counter step[1] (advances on every call, skipped
  // steps included), so consecutive repairs draw independent normals
  const uint64_t key = seed ^ ((uint64_t)(uint32_t)step[1] << 40);
  double s2 = 0.0;
  int bad = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += TAIL_THREADS) {
    float v = g[i];
    if (v != v) {
      const float z = noise ? noise[i] : gauss_hash(key, (uint64_t)i);
      v = mean + (z * stdv) * 0.1f;  // valid_mean + randn * valid_std * 0.1
      g[i] = v;
    } else if (!is_finite_f(v)) {
      v = (v > 0.f ? mx : -mx) * 10.f;  // sign * max_valid * 10.0
      g[i] = v;
    }
    if (!is_finite_f(v))
      ++bad;
    else
      s2 += (double)v * (double)v;
  }
  s2 = block_red_sum(s2, shd);
  bad = block_red_sum(bad, shi);
  if (threadIdx.x == 0) {
    w.rep_d[b] = s2;
    w.rep_i[b] = bad;
  }
}

// ---- K4: norms, factors and the step decision (main.py:357-418) --------------
// seg_coef[s] = {f1 (pre-unscale clip), f2 (1e3 rescale), c (clip_grad_norm_),
// zero}; stat = {total norm, clip coef, max_norm, max post-clip norm};
// flags = {skip, repaired, severe, nonfinite, huge (>1e5), postclip (>10),
// n rescaled, n zeroed}; step[0] += !skip.
//
// DYN = false is the static loss scale (the kernel argument `scale`). DYN = true
// (nsm_grad_tail_scaled) reads the scale from the scaler state sc.state[0], the
// value the loss backward of this step was seeded with, and, once the flags are
// known, thread 0 applies torch.amp.GradScaler's update rule to the state
// (torch._amp_update_scale_). found_inf = the census saw a NaN or Inf in the
// (rank-averaged) scaled gradient, or a non-finite norm survived (flags[3]); with
// on_overflow == 1 it also skips the step. A step skipped for another reason
// (huge, postclip: the reference `continue`s before scaler.update()) leaves the
// scale and the tracker alone. Everything before the update is the same
// arithmetic in both instantiations, so at an equal scale seg_coef, stat and
// flags are bitwise equal (tests/test_gpu_loss_scale.py).
struct TailScaler {
  int* state;  // NSM_SCALER_WORDS words: scale (fp32 bits), tracker, found_inf, overflows, growths
  float growth, backoff;
  int interval, on_overflow;
};

// The hyper block (nsm_hyper_set) holds the two hyper-parameters a schedule
// moves, so a captured tail follows them without a new capture. lr is a double
// because the Adam kernels form 1 - lr*wd and lr/bc1 in double from the double
// the host holds; max_norm is the float this kernel takes (+inf: no clipping).
// HDEV = false takes them as kernel arguments; HDEV = true reads them from the
// block, one uniform load per block before any other work, and then runs the
// same arithmetic: equal values give equal bits.
struct TailHyper {
  double lr;
  float max_norm;
  float pad;
};
static_assert(sizeof(TailHyper) == 16, "the hyper block is 16 bytes");

template <bool DYN, bool HDEV>
__global__ void __launch_bounds__(1024) tail_finalize_kernel(
    const int* __restrict__ seg_blk, int nseg, float scale, TailScaler sc, float max_norm,
    const TailHyper* __restrict__ hyper, TailWs w, float* __restrict__ seg_coef,
    float* __restrict__ stat, int* __restrict__ flags, int* __restrict__ step) {
  if (HDEV) max_norm = hyper->max_norm;
  // the pre-update scale, the same word in every thread (only thread 0 writes
  // the state, after the block's last barrier). The words the update rewrites
  // are read here too, so their latency hides behind the per-segment work
  // instead of adding three dependent loads after the flags are known.
  int tracker0 = 0, overflows0 = 0, growths0 = 0;
  if (DYN) {
    scale = __int_as_float(sc.state[0]);
    tracker0 = sc.state[1];
    overflows0 = sc.state[3];
    growths0 = sc.state[4];
  }
  __shared__ double sh_tot[16];
  __shared__ float sh_mx[16];
  __shared__ int sh_f[16][4];
  __shared__ float s_clip;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool repaired = w.ctl[0] != 0;
  double tot = 0.0;  // sum of squared per-parameter norms after f1, f2
  int nonfin = 0, huge = 0, nresc = 0, nzero = 0;
  for (int sgi = wv; sgi < nseg; sgi += 16) {
    double s2 = w.seg_d[4 * sgi + 3];
    int zero = 0;
    if (repaired) {
      const int b0 = seg_blk[sgi], b1 = seg_blk[sgi + 1];
      double r = 0.0;
      long long bad = 0;
      for (int b = b0 + lane; b < b1; b += 64) {
        r += w.rep_d[b];
        bad += w.rep_i[b];
      }
      r = wave_red_sum(r);
      bad = wave_red_sum(bad);
      s2 = r;
      if (bad > 0) {  // main.py:352-354: repair failed -> zero the gradient
        zero = 1;
        s2 = 0.0;
      }
    }
    if (lane == 0) {
      // the fp32 norm: the squares are summed in double and rounded to fp32,
      // except that a sum of squares above FLT_MAX reads +inf, as an fp32
      // accumulation of them does (the reference's device, main.py:95,
      // torch.norm on CUDA; and the CPU kernels of most hosts)
      const float n1 = s2 > (double)FLT_MAX ? __builtin_inff() : (float)sqrt(s2);
      // main.py:365: g *= clamp(1 / max(1, |g| / (1000*scale)), max=1)
      const float t = n1 / (float)(1000.0 * (double)scale);
      float f1 = t > 1.f ? 1.f / t : 1.f;
      f1 = fminf(f1, 1.f);
      // main.py:368 unscale_ (x 1/scale), then :371-397 on the unscaled grad
      const float inv_s = (float)(1.0 / (double)scale);
      float n2 = (n1 * f1) * inv_s;
      // A norm above ~1.8e19 (sum of squares > FLT_MAX) reads +inf (above).
      // Then the reference's factor 1/max(1, inf) = 0 zeroes the gradient,
      // whose norm is 0 and the step goes on (main.py:361-365); inf * 0 is NaN
      // here, so n2 is set to 0 (tests/test_gpu_tail.py::
      // test_large_finite_norm_zeroes_like_fp32_norm).
      if (n1 == __builtin_inff()) n2 = 0.f;
      // a non-finite survivor of the repair (:374-381) is impossible once
      // zeroed; only an infinite norm (overflowed sum of squares) is left
      if (!zero && !(n2 == n2)) ++nonfin;
      float f2 = 1.f;
      if (n2 > 1e3f) {
        if (n2 > 1e5f)
          ++huge;                      // :388-391 skip
        else {
          f2 = fminf(1.f, 1e3f / n2);  // :396-397
          ++nresc;
        }
      }
      const float n3 = n2 * f2;
      tot += (double)n3 * (double)n3;
      nzero += zero;
      seg_coef[4 * sgi + 0] = f1 * inv_s;  // unscale folded into the pre-clip factor
      seg_coef[4 * sgi + 1] = f2;
      seg_coef[4 * sgi + 3] = (float)zero;
      // stash n3 for the post-clip check
      seg_coef[4 * sgi + 2] = n3;
    }
  }
  if (lane == 0) {
    sh_tot[wv] = tot;
    sh_f[wv][0] = nonfin;
    sh_f[wv][1] = huge;
    sh_f[wv][2] = nresc;
    sh_f[wv][3] = nzero;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double T = 0.0;
    for (int k = 0; k < 16; ++k) T += sh_tot[k];
    // clip_grad_norm_: total = ||stack(norms)||, coef = max_norm / (total + 1e-6), clamp 1
    const float total = (float)sqrt(T);
    float c = max_norm / (total + 1e-6f);
    c = fminf(c, 1.f);
    s_clip = c;
    stat[0] = total;
    stat[1] = c;
    stat[2] = max_norm;
  }
  __syncthreads();
  const float c = s_clip;
  float mxn = 0.f;
  for (int sgi = threadIdx.x; sgi < nseg; sgi += blockDim.x) {
    const float n3 = seg_coef[4 * sgi + 2];
    mxn = fmaxf(mxn, n3 * c);
    seg_coef[4 * sgi + 2] = c;
  }
  mxn = wave_red_max(mxn);
  if (lane == 0) sh_mx[wv] = mxn;
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = 0.f;
    int nonfin_t = 0, huge_t = 0, nresc_t = 0, nzero_t = 0;
    for (int k = 0; k < 16; ++k) {
      M = fmaxf(M, sh_mx[k]);
      nonfin_t += sh_f[k][0];
      huge_t += sh_f[k][1];
      nresc_t += sh_f[k][2];
      nzero_t += sh_f[k][3];
    }
    stat[3] = M;
    const int severe = w.ctl[1];
    const int postclip = M > 10.f ? 1 : 0;  // main.py:408-418
    int skip = (severe || nonfin_t || huge_t || postclip) ? 1 : 0;
    if (DYN) {
      const int found_inf = (repaired || severe || nonfin_t) ? 1 : 0;
      int tracker = tracker0, grew = 0;
      if (found_inf) {
        scale = scale * sc.backoff;
        tracker = 0;
      } else if (!skip) {
        const int n = tracker + 1;
        if (n == sc.interval) {
          const float s2 = scale * sc.growth;
          if (is_finite_f(s2)) {  // false for NaN too
            scale = s2;
            grew = 1;
          }
          tracker = 0;
        } else {
          tracker = n;
        }
      }
      if (found_inf && sc.on_overflow) skip = 1;
      sc.state[0] = __float_as_int(scale);
      sc.state[1] = tracker;
      sc.state[2] = found_inf;
      sc.state[3] = overflows0 + found_inf;
      sc.state[4] = growths0 + grew;
    }
    flags[0] = skip;
    flags[1] = repaired ? 1 : 0;
    flags[2] = severe;
    flags[3] = nonfin_t ? 1 : 0;
    flags[4] = huge_t ? 1 : 0;
    flags[5] = postclip;
    flags[6] = nresc_t;
    flags[7] = nzero_t;
    if (!skip) step[0] = step[0] + 1;
    step[1] = step[1] + 1;  // tail calls (the repair-noise key)
  }
}

// ---- K5: AdamW (torch.optim.AdamW, single-tensor path) honouring the skip ----
// p *= 1 - lr*wd; m = lerp(m, g, 1-b1); v = v*b2 + (1-b2)*g*g;
// p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps); g = ((g*f1)*f2)*c (or 0 if zeroed)
template <bool HDEV>
__global__ void __launch_bounds__(TAIL_THREADS) tail_adamw_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, const int* __restrict__ blk_seg, const int64_t* __restrict__ blk_lo,
    const int64_t* __restrict__ blk_hi, const float* __restrict__ seg_coef,
    const int* __restrict__ flags, const int* __restrict__ step, double lr,
    const TailHyper* __restrict__ hyper, double beta1, double beta2, float eps,
    double weight_decay) {
  if (HDEV) lr = hyper->lr;  // the block's double, then the argument path's arithmetic
  if (flags[0]) return;  // main.py:317/402/418 `continue`: no optimizer step
  const int b = blockIdx.x, sgi = blk_seg[b];
  const int64_t lo = blk_lo[b], hi = blk_hi[b];
  const float f1 = seg_coef[4 * sgi + 0], f2 = seg_coef[4 * sgi + 1], c = seg_coef[4 * sgi + 2];
  const bool zero = seg_coef[4 * sgi + 3] != 0.f;
  const double t = (double)step[0];
  const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
  const float decay = (float)(1.0 - lr * weight_decay);
  const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2);
  const float step_size = (float)(lr / bc1), bc2s = (float)sqrt(bc2);
  for (int64_t i = lo + threadIdx.x; i < hi; i += TAIL_THREADS) {
    float gi = 0.f;
    if (!zero) gi = ((g[i] * f1) * f2) * c;
    float pi = p[i] * decay;
    float mi = m[i];
    mi = mi + w1 * (gi - mi);
    float vi = v[i] * b2;
    vi = vi + (w2 * gi) * gi;
    const float denom = sqrtf(vi) / bc2s + eps;
    pi = pi - step_size * (mi / denom);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
  }
}

// ---- K5': Adam (torch.optim.Adam, single-tensor path, L2 weight decay) --------
// g = ((g*f1)*f2)*c (or 0 if zeroed); g += wd*p; m = lerp(m, g, 1-b1);
// v = v*b2 + (1-b2)*g*g; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps).
// 28 B per element, like AdamW: p, m, v read and written, g read.
template <bool HDEV>
__global__ void __launch_bounds__(TAIL_THREADS) tail_adam_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, const int* __restrict__ blk_seg, const int64_t* __restrict__ blk_lo,
    const int64_t* __restrict__ blk_hi, const float* __restrict__ seg_coef,
    const int* __restrict__ flags, const int* __restrict__ step, double lr,
    const TailHyper* __restrict__ hyper, double beta1, double beta2, float eps,
    double weight_decay) {
  if (HDEV) lr = hyper->lr;  // the block's double, then the argument path's arithmetic
  if (flags[0]) return;  // skipped step
  const int b = blockIdx.x, sgi = blk_seg[b];
  const int64_t lo = blk_lo[b], hi = blk_hi[b];
  const float f1 = seg_coef[4 * sgi + 0], f2 = seg_coef[4 * sgi + 1], c = seg_coef[4 * sgi + 2];
  const bool zero = seg_coef[4 * sgi + 3] != 0.f;
  const double t = (double)step[0];
  const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
  const float wd = (float)weight_decay;
  const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2);
  const float step_size = (float)(lr / bc1), bc2s = (float)sqrt(bc2);
  for (int64_t i = lo + threadIdx.x; i < hi; i += TAIL_THREADS) {
    float gi = 0.f;
    if (!zero) gi = ((g[i] * f1) * f2) * c;
    float pi = p[i];
    gi = gi + wd * pi;  // grad.add(param, alpha=weight_decay)
    float mi = m[i];
    mi = mi + w1 * (gi - mi);
    float vi = v[i] * b2;
    vi = vi + (w2 * gi) * gi;
    const float denom = sqrtf(vi) / bc2s + eps;
    pi = pi - step_size * (mi / denom);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
  }
}

// ---- K5'': SGD (torch.optim.SGD, momentum, dampening 0, no Nesterov) ----------
// g = ((g*f1)*f2)*c (or 0 if zeroed); g += wd*p; buf = g on the first step
// taken (step[0] == 1: torch clones the first stepped gradient into the
// buffer, and a skipped step does not advance step[0]), else buf = mu*buf + g;
// p -= lr*buf. 20 B per element (p read and written, buf read and written, g
// read; the first step does not read buf). MOMENTUM = false is p -= lr*g with
// no buffer at all: 12 B per element.
template <bool MOMENTUM, bool HDEV>
__global__ void __launch_bounds__(TAIL_THREADS) tail_sgd_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
    const int* __restrict__ blk_seg, const int64_t* __restrict__ blk_lo,
    const int64_t* __restrict__ blk_hi, const float* __restrict__ seg_coef,
    const int* __restrict__ flags, const int* __restrict__ step, float lr,
    const TailHyper* __restrict__ hyper, float momentum, float weight_decay) {
  if (HDEV) lr = (float)hyper->lr;  // the cast nsm_sgd_tail makes on the host
  if (flags[0]) return;  // skipped step
  const int b = blockIdx.x, sgi = blk_seg[b];
  const int64_t lo = blk_lo[b], hi = blk_hi[b];
  const float f1 = seg_coef[4 * sgi + 0], f2 = seg_coef[4 * sgi + 1], c = seg_coef[4 * sgi + 2];
  const bool zero = seg_coef[4 * sgi + 3] != 0.f;
  const bool first = step[0] == 1;  // uniform across the grid
  for (int64_t i = lo + threadIdx.x; i < hi; i += TAIL_THREADS) {
    float gi = 0.f;
    if (!zero) gi = ((g[i] * f1) * f2) * c;
    float pi = p[i];
    gi = gi + weight_decay * pi;
    if (MOMENTUM) {
      if (!first) gi = buf[i] * momentum + gi;  // buf.mul_(momentum).add_(grad)
      buf[i] = gi;
    }
    p[i] = pi - lr * gi;
  }
}

}  // namespace nsm

using namespace nsm;

// ============================== C ABI ======================================
extern "C" int64_t nsm_tail_chunk(void) { return TAIL_CHUNK; }

extern "C" int nsm_tail_plan(const int64_t* seg_off, int nseg, int* blk_seg, int64_t* blk_lo,
                             int64_t* blk_hi, int* seg_blk, int cap) {
  if (!seg_off || nseg <= 0) return -1;
  int nb = 0;
  for (int s = 0; s < nseg; ++s) {
    if (seg_blk) seg_blk[s] = nb;
    const int64_t a = seg_off[s], e = seg_off[s + 1];
    if (e < a) return -1;
    for (int64_t lo = a; lo < e; lo += TAIL_CHUNK) {
      if (blk_seg && nb < cap) {
        blk_seg[nb] = s;
        blk_lo[nb] = lo;
        blk_hi[nb] = lo + TAIL_CHUNK < e ? lo + TAIL_CHUNK : e;
      }
      ++nb;
    }
  }
  if (seg_blk) seg_blk[nseg] = nb;
  return nb;
}

extern "C" size_t nsm_tail_ws_bytes(int nseg, int nblk) {
  return tail_ws_layout(nseg, nblk, nullptr, nullptr);
}

// the launch sequence of the four entries: sc.state == NULL is the static
// scale; hyper != NULL reads max_norm from the hyper block (the argument is
// then unused)
static int grad_tail_launch(float* g, int nseg, const int64_t* seg_off, const int* seg_blk,
                            const int* blk_seg, const int64_t* blk_lo, const int64_t* blk_hi,
                            int nblk, float inv_world, float scale, TailScaler sc, float max_norm,
                            const TailHyper* hyper, const float* noise, uint64_t seed, void* ws,
                            size_t ws_bytes, float* seg_coef, float* stat, int* flags, int* step,
                            void* stream) {
  NSM_CHECK_ARG(g && seg_off && seg_blk && blk_seg && blk_lo && blk_hi && ws && seg_coef && stat &&
                    flags && step && nseg > 0 && nblk > 0,
                "grad_tail: bad args");
  NSM_CHECK_ARG(ws_bytes >= nsm_tail_ws_bytes(nseg, nblk), "grad_tail: workspace too small");
  TailWs w;
  tail_ws_layout(nseg, nblk, (char*)ws, &w);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(tail_stats_kernel, dim3(nblk), dim3(TAIL_THREADS), 0, s, g, blk_lo, blk_hi,
                     inv_world, w);
  NSM_LAUNCH_CHECK("tail_stats");
  hipLaunchKernelGGL(tail_decide_kernel, dim3(1), dim3(1024), 0, s, seg_off, seg_blk, nseg, w);
  NSM_LAUNCH_CHECK("tail_decide");
  hipLaunchKernelGGL(tail_repair_kernel, dim3(nblk), dim3(TAIL_THREADS), 0, s, g, blk_seg, blk_lo,
                     blk_hi, noise, seed, step, w);
  NSM_LAUNCH_CHECK("tail_repair");
  auto fin = sc.state ? (hyper ? tail_finalize_kernel<true, true> : tail_finalize_kernel<true, false>)
                      : (hyper ? tail_finalize_kernel<false, true>
                               : tail_finalize_kernel<false, false>);
  hipLaunchKernelGGL(fin, dim3(1), dim3(1024), 0, s, seg_blk, nseg, scale, sc, max_norm, hyper, w,
                     seg_coef, stat, flags, step);
  NSM_LAUNCH_CHECK("tail_finalize");
  return 0;
}

static const TailScaler kNoScaler{nullptr, 1.f, 1.f, 0, 0};

static bool scaler_args_ok(const void* state, float growth, float backoff, int interval,
                           int on_overflow) {
  return state && growth > 1.f && backoff > 0.f && backoff < 1.f && interval > 0 &&
         (on_overflow == 0 || on_overflow == 1);
}

extern "C" int nsm_grad_tail(float* g, int nseg, const int64_t* seg_off, const int* seg_blk,
                             const int* blk_seg, const int64_t* blk_lo, const int64_t* blk_hi,
                             int nblk, float inv_world, float scale, float max_norm,
                             const float* noise, uint64_t seed, void* ws, size_t ws_bytes,
                             float* seg_coef, float* stat, int* flags, int* step, void* stream) {
  NSM_CHECK_ARG(scale > 0.f, "grad_tail: bad args");
  return grad_tail_launch(g, nseg, seg_off, seg_blk, blk_seg, blk_lo, blk_hi, nblk, inv_world,
                          scale, kNoScaler, max_norm, nullptr, noise, seed, ws, ws_bytes, seg_coef,
                          stat, flags, step, stream);
}

extern "C" int nsm_grad_tail_dev(float* g, int nseg, const int64_t* seg_off, const int* seg_blk,
                                 const int* blk_seg, const int64_t* blk_lo, const int64_t* blk_hi,
                                 int nblk, float inv_world, float scale, const void* hyper,
                                 const float* noise, uint64_t seed, void* ws, size_t ws_bytes,
                                 float* seg_coef, float* stat, int* flags, int* step,
                                 void* stream) {
  NSM_CHECK_ARG(scale > 0.f, "grad_tail_dev: bad args");
  NSM_CHECK_ARG(hyper, "grad_tail_dev: null hyper block");
  return grad_tail_launch(g, nseg, seg_off, seg_blk, blk_seg, blk_lo, blk_hi, nblk, inv_world,
                          scale, kNoScaler, 0.f, (const TailHyper*)hyper, noise, seed, ws, ws_bytes,
                          seg_coef, stat, flags, step, stream);
}

extern "C" int nsm_grad_tail_scaled(float* g, int nseg, const int64_t* seg_off, const int* seg_blk,
                                    const int* blk_seg, const int64_t* blk_lo,
                                    const int64_t* blk_hi, int nblk, float inv_world,
                                    void* scaler_state, float max_norm, const float* noise,
                                    uint64_t seed, void* ws, size_t ws_bytes, float* seg_coef,
                                    float* stat, int* flags, int* step, float growth_factor,
                                    float backoff_factor, int growth_interval, int on_overflow,
                                    void* stream) {
  NSM_CHECK_ARG(scaler_args_ok(scaler_state, growth_factor, backoff_factor, growth_interval,
                               on_overflow),
                "grad_tail_scaled: bad scaler args");
  return grad_tail_launch(g, nseg, seg_off, seg_blk, blk_seg, blk_lo, blk_hi, nblk, inv_world, 0.f,
                          TailScaler{(int*)scaler_state, growth_factor, backoff_factor,
                                     growth_interval, on_overflow},
                          max_norm, nullptr, noise, seed, ws, ws_bytes, seg_coef, stat, flags, step,
                          stream);
}

extern "C" int nsm_grad_tail_scaled_dev(float* g, int nseg, const int64_t* seg_off,
                                        const int* seg_blk, const int* blk_seg,
                                        const int64_t* blk_lo, const int64_t* blk_hi, int nblk,
                                        float inv_world, void* scaler_state, const void* hyper,
                                        const float* noise, uint64_t seed, void* ws,
                                        size_t ws_bytes, float* seg_coef, float* stat, int* flags,
                                        int* step, float growth_factor, float backoff_factor,
                                        int growth_interval, int on_overflow, void* stream) {
  NSM_CHECK_ARG(scaler_args_ok(scaler_state, growth_factor, backoff_factor, growth_interval,
                               on_overflow),
                "grad_tail_scaled_dev: bad scaler args");
  NSM_CHECK_ARG(hyper, "grad_tail_scaled_dev: null hyper block");
  return grad_tail_launch(g, nseg, seg_off, seg_blk, blk_seg, blk_lo, blk_hi, nblk, inv_world, 0.f,
                          TailScaler{(int*)scaler_state, growth_factor, backoff_factor,
                                     growth_interval, on_overflow},
                          0.f, (const TailHyper*)hyper, noise, seed, ws, ws_bytes, seg_coef, stat,
                          flags, step, stream);
}

// hyper block <- {lr, max_norm}. The two values are arguments of this launch,
// not words of a host staging buffer: each queued set carries its own pair, so
// sets and replays may alternate on a stream with no host wait between them.
// One thread, plain stores.
__global__ void hyper_set_kernel(TailHyper* hyper, double lr, float max_norm) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    hyper->lr = lr;
    hyper->max_norm = max_norm;
  }
}

extern "C" size_t nsm_hyper_bytes(void) { return sizeof(TailHyper); }

extern "C" int nsm_hyper_set(void* hyper, double lr, float max_norm, void* stream) {
  NSM_CHECK_ARG(lr >= 0.0 && lr <= DBL_MAX, "hyper_set: lr must be finite and >= 0 (got %g)", lr);
  NSM_CHECK_ARG(max_norm >= 0.f, "hyper_set: max_norm must be >= 0 or +inf, not NaN (got %g)",
                (double)max_norm);
  NSM_CHECK_ARG(hyper, "hyper_set: null hyper block");
  hipLaunchKernelGGL(hyper_set_kernel, dim3(1), dim3(64), 0, as_stream(stream), (TailHyper*)hyper,
                     lr, max_norm);
  NSM_LAUNCH_CHECK("hyper_set");
  return 0;
}

// scaler state <- {scale, tracker}; the other words (found_inf, the two
// counters, the reserved ones) keep their values. One thread, plain stores.
__global__ void scaler_set_kernel(int* state, float scale, int tracker) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    state[0] = __float_as_int(scale);
    state[1] = tracker;
  }
}

extern "C" int nsm_scaler_set(void* scaler_state, float scale, int tracker, void* stream) {
  NSM_CHECK_ARG(scaler_state && scale > 0.f && scale <= FLT_MAX && tracker >= 0,
                "scaler_set: bad args");
  hipLaunchKernelGGL(scaler_set_kernel, dim3(1), dim3(64), 0, as_stream(stream),
                     (int*)scaler_state, scale, tracker);
  NSM_LAUNCH_CHECK("scaler_set");
  return 0;
}

// Adam-type update launch of the four entries: hyper != NULL reads lr from the
// hyper block (the argument is then unused)
static int adam_family_launch(bool decoupled, const char* what, float* p, const float* g, float* m,
                              float* v, const int* blk_seg, const int64_t* blk_lo,
                              const int64_t* blk_hi, int nblk, const float* seg_coef,
                              const int* flags, const int* step, double lr, const TailHyper* hyper,
                              double beta1, double beta2, double eps, double weight_decay,
                              void* stream) {
  NSM_CHECK_ARG(p && g && m && v && blk_seg && blk_lo && blk_hi && seg_coef && flags && step &&
                    nblk > 0,
                "%s: bad args", what);
  auto k = decoupled ? (hyper ? tail_adamw_kernel<true> : tail_adamw_kernel<false>)
                     : (hyper ? tail_adam_kernel<true> : tail_adam_kernel<false>);
  hipLaunchKernelGGL(k, dim3(nblk), dim3(TAIL_THREADS), 0, as_stream(stream), p, g, m, v, blk_seg,
                     blk_lo, blk_hi, seg_coef, flags, step, lr, hyper, beta1, beta2, (float)eps,
                     weight_decay);
  NSM_LAUNCH_CHECK(what);
  return 0;
}

extern "C" int nsm_adamw_tail(float* p, const float* g, float* m, float* v, const int* blk_seg,
                              const int64_t* blk_lo, const int64_t* blk_hi, int nblk,
                              const float* seg_coef, const int* flags, const int* step, double lr,
                              double beta1, double beta2, double eps, double weight_decay,
                              void* stream) {
  return adam_family_launch(true, "adamw_tail", p, g, m, v, blk_seg, blk_lo, blk_hi, nblk, seg_coef,
                            flags, step, lr, nullptr, beta1, beta2, eps, weight_decay, stream);
}

extern "C" int nsm_adam_tail(float* p, const float* g, float* m, float* v, const int* blk_seg,
                             const int64_t* blk_lo, const int64_t* blk_hi, int nblk,
                             const float* seg_coef, const int* flags, const int* step, double lr,
                             double beta1, double beta2, double eps, double weight_decay,
                             void* stream) {
  return adam_family_launch(false, "adam_tail", p, g, m, v, blk_seg, blk_lo, blk_hi, nblk, seg_coef,
                            flags, step, lr, nullptr, beta1, beta2, eps, weight_decay, stream);
}

extern "C" int nsm_adamw_tail_dev(float* p, const float* g, float* m, float* v, const int* blk_seg,
                                  const int64_t* blk_lo, const int64_t* blk_hi, int nblk,
                                  const float* seg_coef, const int* flags, const int* step,
                                  const void* hyper, double beta1, double beta2, double eps,
                                  double weight_decay, void* stream) {
  NSM_CHECK_ARG(hyper, "adamw_tail_dev: null hyper block");
  return adam_family_launch(true, "adamw_tail_dev", p, g, m, v, blk_seg, blk_lo, blk_hi, nblk,
                            seg_coef, flags, step, 0.0, (const TailHyper*)hyper, beta1, beta2, eps,
                            weight_decay, stream);
}

extern "C" int nsm_adam_tail_dev(float* p, const float* g, float* m, float* v, const int* blk_seg,
                                 const int64_t* blk_lo, const int64_t* blk_hi, int nblk,
                                 const float* seg_coef, const int* flags, const int* step,
                                 const void* hyper, double beta1, double beta2, double eps,
                                 double weight_decay, void* stream) {
  NSM_CHECK_ARG(hyper, "adam_tail_dev: null hyper block");
  return adam_family_launch(false, "adam_tail_dev", p, g, m, v, blk_seg, blk_lo, blk_hi, nblk,
                            seg_coef, flags, step, 0.0, (const TailHyper*)hyper, beta1, beta2, eps,
                            weight_decay, stream);
}

static int sgd_launch(const char* what, float* p, const float* g, float* buf, const int* blk_seg,
                      const int64_t* blk_lo, const int64_t* blk_hi, int nblk,
                      const float* seg_coef, const int* flags, const int* step, double lr,
                      const TailHyper* hyper, double momentum, double weight_decay, void* stream) {
  NSM_CHECK_ARG(p && g && blk_seg && blk_lo && blk_hi && seg_coef && flags && step && nblk > 0 &&
                    (buf || momentum == 0.0),
                "%s: bad args", what);
  const bool mom = momentum != 0.0;
  auto k = mom ? (hyper ? tail_sgd_kernel<true, true> : tail_sgd_kernel<true, false>)
               : (hyper ? tail_sgd_kernel<false, true> : tail_sgd_kernel<false, false>);
  hipLaunchKernelGGL(k, dim3(nblk), dim3(TAIL_THREADS), 0, as_stream(stream), p, g,
                     mom ? buf : (float*)nullptr, blk_seg, blk_lo, blk_hi, seg_coef, flags, step,
                     (float)lr, hyper, mom ? (float)momentum : 0.f, (float)weight_decay);
  NSM_LAUNCH_CHECK(what);
  return 0;
}

extern "C" int nsm_sgd_tail(float* p, const float* g, float* buf, const int* blk_seg,
                            const int64_t* blk_lo, const int64_t* blk_hi, int nblk,
                            const float* seg_coef, const int* flags, const int* step, double lr,
                            double momentum, double weight_decay, void* stream) {
  return sgd_launch("sgd_tail", p, g, buf, blk_seg, blk_lo, blk_hi, nblk, seg_coef, flags, step,
                    lr, nullptr, momentum, weight_decay, stream);
}

extern "C" int nsm_sgd_tail_dev(float* p, const float* g, float* buf, const int* blk_seg,
                                const int64_t* blk_lo, const int64_t* blk_hi, int nblk,
                                const float* seg_coef, const int* flags, const int* step,
                                const void* hyper, double momentum, double weight_decay,
                                void* stream) {
  NSM_CHECK_ARG(hyper, "sgd_tail_dev: null hyper block");
  return sgd_launch("sgd_tail_dev", p, g, buf, blk_seg, blk_lo, blk_hi, nblk, seg_coef, flags,
                    step, 0.0, (const TailHyper*)hyper, momentum, weight_decay, stream);
}
