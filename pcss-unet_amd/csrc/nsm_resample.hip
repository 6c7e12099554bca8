// Pooling and bilinear resampling of NHWC activations ("Element-wise
// sources"): AvgPool2d(2) forward / backward and its fusion with the BN apply,
// the align_corners=True resize and the x2 + match composite in their
// per-element, row-blocked and separable forms, the act-on-load (`_act`)
// forwards and the backward forms that carry the next BN-backward reduction
// (`_bnred`), with the plan and the environment knobs that pick a form.
#include <algorithm>

#include "nsm_elem.h"

namespace nsm {

// ---------------------------------------------------------------------------
// AvgPool2d(2), floor mode
// ---------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) avgpool2_fwd_kernel(const T* __restrict__ x, int B, int H,
                                                           int W, int C8, FastDiv fdC8,
                                                           FastDiv fdWo, FastDiv fdHo,
                                                           T* __restrict__ y) {
  const int Ho = H / 2, Wo = W / 2, C = C8 * 8;
  const uint32_t total = (uint32_t)B * Ho * Wo * C8;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const uint32_t p = fdiv(i, fdC8);
    const int c = (int)(i - p * (uint32_t)C8) * 8;
    const uint32_t t = fdiv(p, fdWo);
    const int ox = (int)(p - t * Wo);
    const uint32_t b = fdiv(t, fdHo);
    const int oy = (int)(t - b * Ho);
    const T* base = x + (((size_t)b * H + 2 * oy) * W + 2 * ox) * C + c;
    const size_t rs = (size_t)W * C;
    F8 s = ld8(base);
    s += ld8(base + C);
    s += ld8(base + rs);
    s += ld8(base + rs + C);
    st8(y + (size_t)p * C + c, 0.25f * s);
  }
}

// The encoder block output z = lrelu(bn2(Y2)) (Unetmodel.py:27-28) and its
// AvgPool2d(2) (:105,108,111) from one read of Y2: each thread takes a 2x2
// pixel quad (ceil grid, so odd rows / columns still get their z) of one
// 8-channel group, writes the quad's z (the skip tensor) and, inside the floor
// grid, their mean from the stored values (as avgpool2_fwd would read them).
template <typename T>
__global__ void __launch_bounds__(256) bn_act_pool_kernel(const T* __restrict__ y, int B, int H,
                                                          int W, int C8, FastDiv fdC8,
                                                          FastDiv fdWc, FastDiv fdHc,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ shift,
                                                          float slope, T* __restrict__ z,
                                                          T* __restrict__ pooled,
                                                          uint32_t* __restrict__ amax) {
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2, Ho = H / 2, Wo = W / 2, C = C8 * 8;
  uint32_t am = 0;  // max|pooled| (the next Winograd conv's h2 scale source)
  const uint32_t total = (uint32_t)B * Hc * Wc * C8;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const uint32_t p = fdiv(i, fdC8);
    const int c = (int)(i - p * (uint32_t)C8) * 8;
    const uint32_t t = fdiv(p, fdWc);
    const int cx = (int)(p - t * Wc);
    const uint32_t b = fdiv(t, fdHc);
    const int cy = (int)(t - b * Hc);
    const F8 sc = ldf8(scale + c), sh = ldf8(shift + c);
    F8 q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int yy = 2 * cy + (k >> 1), xx = 2 * cx + (k & 1);
      q[k] = f8zero();
      if (yy < H && xx < W) {
        const size_t off = (((size_t)b * H + yy) * W + xx) * C + c;
        q[k] = as_stored8<T>(lrelu8(ld8(y + off) * sc + sh, slope));
        st8(z + off, q[k]);
      }
    }
    if (cy < Ho && cx < Wo) {
      F8 sum = q[0];
      sum += q[1];
      sum += q[2];
      sum += q[3];
      const F8 pv = 0.25f * sum;
      st8(pooled + (((size_t)b * Ho + cy) * Wo + cx) * C + c, pv);
      if (amax) {
        amax_fold(am, pv.a);
        amax_fold(am, pv.b);
      }
    }
  }
  amax_flush(am, amax);
}

template <typename T, bool RED>
__global__ void __launch_bounds__(256) avgpool2_bwd_add_kernel(const T* __restrict__ dy, int B,
                                                               int H, int W, int C8, FastDiv fdC8,
                                                               FastDiv fdW, FastDiv fdH,
                                                               const T* __restrict__ skip,
                                                               T* __restrict__ dx, BnRedP rp) {
  const int Ho = H / 2, Wo = W / 2, C = C8 * 8;
  const uint32_t total = (uint32_t)B * H * W * C8;
  BnRedAcc ra;
  if (RED) ra.init(rp, (threadIdx.x % C8) * 8);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const uint32_t p = fdiv(i, fdC8);
    const int c = (int)(i - p * (uint32_t)C8) * 8;
    const uint32_t t = fdiv(p, fdW);
    const int xx = (int)(p - t * W);
    const uint32_t b = fdiv(t, fdH);
    const int yy = (int)(t - b * H);
    F8 v = skip ? ld8(skip + (size_t)p * C + c) : f8zero();
    const int oy = yy >> 1, ox = xx >> 1;
    if (oy < Ho && ox < Wo) v += 0.25f * ld8(dy + (((size_t)b * Ho + oy) * Wo + ox) * C + c);
    st8(dx + (size_t)p * C + c, v);
    if (RED) ra.add<T>(rp, as_stored8<T>(v), p, C, c);
  }
  if (RED) ra.write(rp, C8);
}

// ---------------------------------------------------------------------------
// Bilinear resize, align_corners=True (ATen upsample_bilinear2d semantics:
// scale=(in-1)/(out-1) in fp32, src=scale*dst, i0=floor, i1=i0+(i0<in-1),
// l1=src-i0, l0=1-l1).
// ---------------------------------------------------------------------------
// lin_idx / ac_scale: nsm_common.h

// (pixel, 8-channel group) of a flat index over [B][H][W][C8] (32-bit fast division)
struct Pix8 {
  int b, y, x, c;
};
__device__ __forceinline__ Pix8 pix8(uint32_t i, int C8, int H, int W, const FastDiv& fdC8,
                                     const FastDiv& fdW, const FastDiv& fdH, uint32_t& p) {
  Pix8 r;
  p = fdiv(i, fdC8);
  r.c = (int)(i - p * (uint32_t)C8) * 8;
  const uint32_t t = fdiv(p, fdW);
  r.x = (int)(p - t * (uint32_t)W);
  const uint32_t b = fdiv(t, fdH);
  r.y = (int)(t - b * (uint32_t)H);
  r.b = (int)b;
  return r;
}

// XCD-local block order for the resampling gathers: consecutive blocks are
// dispatched round-robin over the 8 XCDs (separate L2s); renumber so each XCD
// sweeps a contiguous slice of every grid-stride window and the rows its
// neighbours share stay in its own L2 (grid % 8 == 0, see xcd_grid)
__device__ __forceinline__ uint32_t xcd_block() {
  const uint32_t per = gridDim.x >> 3;
  return (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
}

// 8 channels (one 16-B bf16 vector / two fp32 vectors) per lane: the model's
// activations (C % 8 == 0)
// ACT ("act on load"): the source is not materialised — every tap is the
// decoder block output z = lrelu(Y2*scale+shift) (+ skip), rounded as bn_act
// stores it (Unetmodel.py:27-28,125-137 then :122-141's upsample), so z is
// never written or re-read. ActSrc carries Y2's BN vectors and the skip.
struct ActSrc {
  const float* scale;
  const float* shift;
  const void* res;
  float slope;
};
template <typename T, bool ACT>
__device__ __forceinline__ F8 src8(const T* x, size_t off, const ActSrc& a, int c) {
  if constexpr (!ACT) {
    return ld8(x + off);
  } else {
    F8 o = lrelu8(ld8(x + off) * ldf8(a.scale + c) + ldf8(a.shift + c), a.slope);
    if (a.res) o += ld8((const T*)a.res + off);
    return as_stored8<T>(o);
  }
}

template <typename T, bool ACT = false>
__global__ void __launch_bounds__(256) resize_fwd8_kernel(const T* __restrict__ x, int Hi, int Wi,
                                                          int C8, uint32_t total, FastDiv fdC8,
                                                          FastDiv fdWo, FastDiv fdHo,
                                                          T* __restrict__ y, int Ho, int Wo,
                                                          float sh, float sw,
                                                          ActSrc act = ActSrc{}) {
  const int C = C8 * 8;
  for (uint32_t i = xcd_block() * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    uint32_t p;
    const Pix8 q = pix8(i, C8, Ho, Wo, fdC8, fdWo, fdHo, p);
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    lin_idx(sh, q.y, Hi, y0, y1, ly0, ly1);
    lin_idx(sw, q.x, Wi, x0, x1, lx0, lx1);
    const size_t rb = (size_t)q.b * Hi;
    const size_t r0 = (rb + y0) * Wi * C + q.c, r1 = (rb + y1) * Wi * C + q.c;
    const F8 v = ly0 * (lx0 * src8<T, ACT>(x, r0 + x0 * C, act, q.c) +
                        lx1 * src8<T, ACT>(x, r0 + x1 * C, act, q.c)) +
                 ly1 * (lx0 * src8<T, ACT>(x, r1 + x0 * C, act, q.c) +
                        lx1 * src8<T, ACT>(x, r1 + x1 * C, act, q.c));
    st8(y + (size_t)p * C + q.c, v);
  }
}

// any C: the odd-size input guard (Unetmodel.py:94-97) runs on [B*C][H][W][1]
template <typename T>
__global__ void resize_fwd1_kernel(const T* __restrict__ x, int B, int Hi, int Wi, int C,
                                   T* __restrict__ y, int Ho, int Wo, float sh, float sw) {
  long long total = (long long)B * Ho * Wo * C;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    int c = (int)(i % C);
    long long t = i / C;
    int ox = (int)(t % Wo);
    t /= Wo;
    int oy = (int)(t % Ho);
    int b = (int)(t / Ho);
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    lin_idx(sh, oy, Hi, y0, y1, ly0, ly1);
    lin_idx(sw, ox, Wi, x0, x1, lx0, lx1);
    const size_t rb = (size_t)b * Hi;
    float v = ly0 * (lx0 * ld1(x + ((rb + y0) * Wi + x0) * C + c) +
                     lx1 * ld1(x + ((rb + y0) * Wi + x1) * C + c)) +
              ly1 * (lx0 * ld1(x + ((rb + y1) * Wi + x0) * C + c) +
                     lx1 * ld1(x + ((rb + y1) * Wi + x1) * C + c));
    st1(y + i, v);
  }
}

// weight of output index `o` on input index `i` (0 if none)
__device__ __forceinline__ float lin_w(float scale, int o, int in, int i) {
  int i0, i1;
  float l0, l1;
  lin_idx(scale, o, in, i0, i1, l0, l1);
  return (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f);
}

__device__ __forceinline__ void cand_range(float scale, int i, int out, int& lo, int& hi) {
  if (scale <= 0.f) {
    lo = 0;
    hi = out - 1;
    return;
  }
  lo = max(0, (int)floorf((float)(i - 1) / scale) - 1);
  hi = min(out - 1, (int)ceilf((float)(i + 1) / scale) + 1);
}

// The backward gathers: per axis, the candidate window is trimmed to the
// outputs with a non-zero weight (4-5 for a x2 upsample); the x weights and
// clamped column indices of a lane sit in fully unrolled register arrays, and
// each output row's loads are issued together, unconditionally, so a row costs
// one memory latency (a load under a per-lane branch would wait alone). Zero
// weights are skipped by select, exactly as a skipped term. Wider windows
// (strong downsizing) take the plain loop.
constexpr int RS_W = 6;

template <typename WF>
__device__ __forceinline__ void trim_range(int& lo, int& hi, WF w) {
  while (lo < hi && w(lo) == 0.f) ++lo;
  while (hi > lo && w(hi) == 0.f) --hi;
}

template <typename T>
__device__ __forceinline__ void gather_row(F8& acc, const T* __restrict__ row, int C, float wy,
                                           const float (&wx)[RS_W], const int (&xo)[RS_W]) {
  F8 v[RS_W];
#pragma unroll
  for (int k = 0; k < RS_W; ++k) v[k] = ld8(row + (size_t)xo[k] * C);
#pragma unroll
  for (int k = 0; k < RS_W; ++k) {
    const float w = wy * wx[k];
    const F8 t = acc + w * v[k];
    acc.a = wx[k] != 0.f ? t.a : acc.a;
    acc.b = wx[k] != 0.f ? t.b : acc.b;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) resize_bwd8_kernel(const T* __restrict__ dy, int Hi, int Wi,
                                                          int C8, uint32_t total, FastDiv fdC8,
                                                          FastDiv fdWi, FastDiv fdHi,
                                                          T* __restrict__ dx, int Ho, int Wo,
                                                          float sh, float sw) {
  const int C = C8 * 8;
  for (uint32_t i = xcd_block() * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    uint32_t p;
    const Pix8 q = pix8(i, C8, Hi, Wi, fdC8, fdWi, fdHi, p);
    int ylo, yhi, xlo, xhi;
    cand_range(sh, q.y, Ho, ylo, yhi);
    cand_range(sw, q.x, Wo, xlo, xhi);
    trim_range(ylo, yhi, [&](int o) { return lin_w(sh, o, Hi, q.y); });
    trim_range(xlo, xhi, [&](int o) { return lin_w(sw, o, Wi, q.x); });
    const T* base = dy + (size_t)q.b * Ho * Wo * C + q.c;
    F8 acc = f8zero();
    if (xhi - xlo < RS_W) {
      float wx[RS_W];
      int xo[RS_W];
#pragma unroll
      for (int k = 0; k < RS_W; ++k) {
        xo[k] = min(xlo + k, xhi);
        wx[k] = xlo + k <= xhi ? lin_w(sw, xlo + k, Wi, q.x) : 0.f;
      }
      for (int oy = ylo; oy <= yhi; ++oy) {
        const float wy = lin_w(sh, oy, Hi, q.y);
        if (wy != 0.f) gather_row(acc, base + (size_t)oy * Wo * C, C, wy, wx, xo);
      }
    } else {
      for (int oy = ylo; oy <= yhi; ++oy) {
        const float wy = lin_w(sh, oy, Hi, q.y);
        if (wy == 0.f) continue;
        const T* row = base + (size_t)oy * Wo * C;
        for (int ox = xlo; ox <= xhi; ++ox) {
          const float w = lin_w(sw, ox, Wi, q.x);
          if (w != 0.f) acc += (wy * w) * ld8(row + (size_t)ox * C);
        }
      }
    }
    st8(dx + (size_t)p * C + q.c, acc);
  }
}

template <typename T>
__global__ void resize_bwd1_kernel(const T* __restrict__ dy, int B, int Hi, int Wi, int C,
                                   T* __restrict__ dx, int Ho, int Wo, float sh, float sw) {
  long long total = (long long)B * Hi * Wi * C;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    int c = (int)(i % C);
    long long t = i / C;
    int ix = (int)(t % Wi);
    t /= Wi;
    int iy = (int)(t % Hi);
    int b = (int)(t / Hi);
    int ylo, yhi, xlo, xhi;
    cand_range(sh, iy, Ho, ylo, yhi);
    cand_range(sw, ix, Wo, xlo, xhi);
    float acc = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
      const float wy = lin_w(sh, oy, Hi, iy);
      if (wy == 0.f) continue;
      const T* row = dy + ((size_t)b * Ho + oy) * Wo * C;
      for (int ox = xlo; ox <= xhi; ++ox) {
        const float w = lin_w(sw, ox, Wi, ix);
        if (w != 0.f) acc += (wy * w) * ld1(row + (size_t)ox * C + c);
      }
    }
    st1(dx + i, acc);
  }
}

// ---------------------------------------------------------------------------
// Composite: nn.Upsample(x2) to (2h,2w) followed by _upsample_and_match to
// (th,tw) (Unetmodel.py:140-141, the up9 "blur"), without materialising the
// 4x intermediate. The row-blocked forward (used for rows up to U2_MAXW)
// applies the separable combined weights as a 3x3 stencil; the per-element
// fallback evaluates the intermediate samples as the two-step path rounds
// them (fp32 per sample). Backward uses the combined weights
// W[o->i] = sum_m w2(o->m) w1(m->i).
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ F8 up_sample8(const T* __restrict__ x, size_t rb, int h, int w, int C,
                                         int c, float s1h, float s1w, int my, int mx) {
  int y0, y1, x0, x1;
  float a0, a1, b0, b1;
  lin_idx(s1h, my, h, y0, y1, a0, a1);
  lin_idx(s1w, mx, w, x0, x1, b0, b1);
  const T* r0 = x + (rb + y0) * w * C + c;
  const T* r1 = x + (rb + y1) * w * C + c;
  return a0 * (b0 * ld8(r0 + x0 * C) + b1 * ld8(r0 + x1 * C)) +
         a1 * (b0 * ld8(r1 + x0 * C) + b1 * ld8(r1 + x1 * C));
}

template <typename T>
__global__ void __launch_bounds__(256) up2_resize_fwd8_kernel(const T* __restrict__ x, int h, int w,
                                                              int C8, uint32_t total,
                                                              FastDiv fdC8, FastDiv fdtw,
                                                              FastDiv fdth, T* __restrict__ y,
                                                              int th, int tw, float s1h, float s1w,
                                                              float s2h, float s2w) {
  const int C = C8 * 8, h2 = 2 * h, w2 = 2 * w;
  for (uint32_t i = xcd_block() * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    uint32_t p;
    const Pix8 q = pix8(i, C8, th, tw, fdC8, fdtw, fdth, p);
    int m0, m1, n0, n1;
    float l0, l1, k0, k1;
    lin_idx(s2h, q.y, h2, m0, m1, l0, l1);
    lin_idx(s2w, q.x, w2, n0, n1, k0, k1);
    const size_t rb = (size_t)q.b * h;
    const F8 u00 = up_sample8(x, rb, h, w, C, q.c, s1h, s1w, m0, n0);
    const F8 u01 = up_sample8(x, rb, h, w, C, q.c, s1h, s1w, m0, n1);
    const F8 u10 = up_sample8(x, rb, h, w, C, q.c, s1h, s1w, m1, n0);
    const F8 u11 = up_sample8(x, rb, h, w, C, q.c, s1h, s1w, m1, n1);
    st8(y + (size_t)p * C + q.c, l0 * (k0 * u00 + k1 * u01) + l1 * (k0 * u10 + k1 * u11));
  }
}

// Row-blocked forward of the composite: one block per output row (b, oy). Per
// axis the two bilinear steps collapse to at most 3 consecutive input taps
// (m1 = m0 + 1 and each step spreads by < 1 input), so an output is a 3x3
// stencil: 9 loads instead of the 16 of evaluating the 4 intermediate samples.
// The taps and combined weights of every column live in LDS, the row's in
// registers (fp32 combination: within an ulp of the two-step rounding).
__device__ __forceinline__ int comb3(float s2, int o, int n2, float s1, int n1, float* wk) {
  int m0, m1, i00, i01, i10, i11;
  float l0, l1, a00, a01, a10, a11;
  lin_idx(s2, o, n2, m0, m1, l0, l1);
  lin_idx(s1, m0, n1, i00, i01, a00, a01);
  lin_idx(s1, m1, n1, i10, i11, a10, a11);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = i00 + k;
    wk[k] = l0 * ((i00 == i ? a00 : 0.f) + (i01 == i ? a01 : 0.f)) +
            l1 * ((i10 == i ? a10 : 0.f) + (i11 == i ? a11 : 0.f));
  }
  return i00;
}

template <typename T, bool ACT = false>
__global__ void __launch_bounds__(256) up2_resize_fwd_rows_kernel(
    const T* __restrict__ x, int h, int w, int C8, FastDiv fdC8, T* __restrict__ y, int th, int tw,
    float s1h, float s1w, float s2h, float s2w, ActSrc act = ActSrc{}) {
  extern __shared__ float u2f_tables[];  // [tw][3] weights, [tw] first tap
  float* xw = u2f_tables;
  int* xb = (int*)(u2f_tables + (size_t)tw * 3);
  const int C = C8 * 8;
  const int b = blockIdx.x / th, oy = blockIdx.x - b * th;
  for (int ox = threadIdx.x; ox < tw; ox += blockDim.x) xb[ox] = comb3(s2w, ox, 2 * w, s1w, w, xw + ox * 3);
  float wy[3];
  const int yb = comb3(s2h, oy, 2 * h, s1h, h, wy);
  __syncthreads();
  size_t rows[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) rows[a] = ((size_t)b * h + min(yb + a, h - 1)) * w * C;
  T* orow = y + ((size_t)b * th + oy) * tw * C;
  // gridDim.y segments per row (small batches: enough blocks for the chip)
  const uint32_t items = (uint32_t)tw * (uint32_t)C8;
  const uint32_t seg = (items + gridDim.y - 1) / gridDim.y;
  const uint32_t i0 = blockIdx.y * seg, i1 = min(items, i0 + seg);
  for (uint32_t it = i0 + threadIdx.x; it < i1; it += blockDim.x) {
    const int ox = (int)fdiv(it, fdC8);
    const int c = (int)(it - (uint32_t)ox * (uint32_t)C8) * 8;
    const int x0 = xb[ox];
    const float wx0 = xw[ox * 3], wx1 = xw[ox * 3 + 1], wx2 = xw[ox * 3 + 2];
    const int c0 = x0 * C + c, c1 = min(x0 + 1, w - 1) * C + c, c2 = min(x0 + 2, w - 1) * C + c;
    F8 v[9];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[3 * a] = src8<T, ACT>(x, rows[a] + c0, act, c);
      v[3 * a + 1] = src8<T, ACT>(x, rows[a] + c1, act, c);
      v[3 * a + 2] = src8<T, ACT>(x, rows[a] + c2, act, c);
    }
    F8 acc = f8zero();
#pragma unroll
    for (int a = 0; a < 3; ++a)
      acc += wy[a] * (wx0 * v[3 * a] + wx1 * v[3 * a + 1] + wx2 * v[3 * a + 2]);
    st8(orow + (size_t)ox * C + c, acc);
  }
}

// Separable form of the row-blocked composite forward: grid = (output row,
// channel slice). Phase 1 combines the row's 3 source rows with the y weights
// into an fp32 LDS row [w][cb] (each source element loaded once per block);
// phase 2 takes the 3 x taps of every output column from LDS: 3 global vector
// loads per output instead of 9.
template <typename T, bool ACT = false>
__global__ void __launch_bounds__(256) up2_resize_fwd_sep_kernel(
    const T* __restrict__ x, int h, int w, int C, int lcb8, T* __restrict__ y, int th, int tw,
    float s1h, float s1w, float s2h, float s2w, ActSrc act = ActSrc{}) {
  extern __shared__ float u2s_lds[];  // [w][cb] column sums, [tw][3] x weights, [tw] first taps
  const int cb8 = 1 << lcb8, cb = cb8 * 8;
  float* vcol = u2s_lds;
  float* xw = vcol + (size_t)w * cb;
  int* xb = (int*)(xw + (size_t)tw * 3);
  const int tid = threadIdx.x;
  const int b = blockIdx.x / th, oy = blockIdx.x - b * th;
  const int c0 = blockIdx.y * cb;
  for (int ox = tid; ox < tw; ox += blockDim.x) xb[ox] = comb3(s2w, ox, 2 * w, s1w, w, xw + ox * 3);
  float wy[3];
  const int yb = comb3(s2h, oy, 2 * h, s1h, h, wy);
  size_t rows[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) rows[a] = ((size_t)b * h + min(yb + a, h - 1)) * w * C + c0;
  const uint32_t items1 = (uint32_t)w << lcb8;
  for (uint32_t it = tid; it < items1; it += blockDim.x) {
    const int xi = (int)(it >> lcb8), c = (int)(it & (cb8 - 1)) * 8;
    const size_t o = (size_t)xi * C + c;
    const F8 v0 = src8<T, ACT>(x, rows[0] + o, act, c0 + c);
    const F8 v1 = src8<T, ACT>(x, rows[1] + o, act, c0 + c);
    const F8 v2 = src8<T, ACT>(x, rows[2] + o, act, c0 + c);
    F8 acc = wy[0] * v0;
    acc += wy[1] * v1;
    acc += wy[2] * v2;
    *(f32x4*)&vcol[xi * cb + c] = acc.a;
    *(f32x4*)&vcol[xi * cb + c + 4] = acc.b;
  }
  __syncthreads();
  T* orow = y + ((size_t)b * th + oy) * tw * C + c0;
  const uint32_t items2 = (uint32_t)tw << lcb8;
  for (uint32_t it = tid; it < items2; it += blockDim.x) {
    const int ox = (int)(it >> lcb8), c = (int)(it & (cb8 - 1)) * 8;
    const int x0 = xb[ox];
    const float wx0 = xw[ox * 3], wx1 = xw[ox * 3 + 1], wx2 = xw[ox * 3 + 2];
    F8 acc = wx0 * ld8(&vcol[x0 * cb + c]);
    acc += wx1 * ld8(&vcol[min(x0 + 1, w - 1) * cb + c]);
    acc += wx2 * ld8(&vcol[min(x0 + 2, w - 1) * cb + c]);
    st8(orow + (size_t)ox * C + c, acc);
  }
}

// combined 1-D weight of final output index o on input index i
__device__ __forceinline__ float comb_w(float s2, int o, int n2, float s1, int n1, int i) {
  int m0, m1;
  float l0, l1;
  lin_idx(s2, o, n2, m0, m1, l0, l1);
  float wgt = 0.f;
  if (l0 != 0.f) wgt += l0 * lin_w(s1, m0, n1, i);
  if (l1 != 0.f) wgt += l1 * lin_w(s1, m1, n1, i);
  return wgt;
}

template <typename T>
__global__ void __launch_bounds__(256) up2_resize_bwd8_kernel(const T* __restrict__ dy, int h,
                                                              int w, int C8, uint32_t total,
                                                              FastDiv fdC8, FastDiv fdw,
                                                              FastDiv fdh, T* __restrict__ dx,
                                                              int th, int tw, float s1h, float s1w,
                                                              float s2h, float s2w) {
  const int C = C8 * 8, h2 = 2 * h, w2 = 2 * w;
  for (uint32_t i = xcd_block() * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    uint32_t p;
    const Pix8 q = pix8(i, C8, h, w, fdC8, fdw, fdh, p);
    // intermediate rows touching iy, then final rows touching those
    int mlo, mhi, olo, ohi, olo2, ohi2;
    cand_range(s1h, q.y, h2, mlo, mhi);
    cand_range(s2h, mlo, th, olo, ohi2);
    cand_range(s2h, mhi, th, olo2, ohi);
    olo = min(olo, olo2);
    ohi = max(ohi, ohi2);
    int nlo, nhi, plo, phi, plo2, phi2;
    cand_range(s1w, q.x, w2, nlo, nhi);
    cand_range(s2w, nlo, tw, plo, phi2);
    cand_range(s2w, nhi, tw, plo2, phi);
    plo = min(plo, plo2);
    phi = max(phi, phi2);
    trim_range(olo, ohi, [&](int o) { return comb_w(s2h, o, h2, s1h, h, q.y); });
    trim_range(plo, phi, [&](int o) { return comb_w(s2w, o, w2, s1w, w, q.x); });
    const T* base = dy + (size_t)q.b * th * tw * C + q.c;
    F8 acc = f8zero();
    if (phi - plo < RS_W) {
      float wx[RS_W];
      int xo[RS_W];
#pragma unroll
      for (int k = 0; k < RS_W; ++k) {
        xo[k] = min(plo + k, phi);
        wx[k] = plo + k <= phi ? comb_w(s2w, plo + k, w2, s1w, w, q.x) : 0.f;
      }
      for (int oy = olo; oy <= ohi; ++oy) {
        const float wy = comb_w(s2h, oy, h2, s1h, h, q.y);
        if (wy != 0.f) gather_row(acc, base + (size_t)oy * tw * C, C, wy, wx, xo);
      }
    } else {
      for (int oy = olo; oy <= ohi; ++oy) {
        const float wy = comb_w(s2h, oy, h2, s1h, h, q.y);
        if (wy == 0.f) continue;
        const T* row = base + (size_t)oy * tw * C;
        for (int ox = plo; ox <= phi; ++ox) {
          const float wxk = comb_w(s2w, ox, w2, s1w, w, q.x);
          if (wxk != 0.f) acc += (wy * wxk) * ld8(row + (size_t)ox * C);
        }
      }
    }
    st8(dx + (size_t)p * C + q.c, acc);
  }
}

// Row-blocked form of the composite backward: one block per input row (b, iy).
// The x-axis windows and combined weights of every column are built once per
// block into LDS (the per-element form recomputes ~25 composite weights per
// lane: ALU-bound), the row's y window once; the lanes then only gather.
constexpr int U2_MAXW = 2048;  // widest row the LDS tables hold

template <typename T, bool RED>
__global__ void __launch_bounds__(256) up2_resize_bwd_rows_kernel(
    const T* __restrict__ dy, int h, int w, int C8, FastDiv fdC8, T* __restrict__ dx, int th,
    int tw, float s1h, float s1w, float s2h, float s2w, BnRedP rp) {
  extern __shared__ float u2_tables[];  // [w][RS_W] weights, [w] window starts, [w] widths
  float* xw = u2_tables;
  int* xlo = (int*)(u2_tables + (size_t)w * RS_W);
  int* xn = xlo + w;
  __shared__ float yw[RS_W];
  __shared__ int ywin[2];
  const int C = C8 * 8, h2 = 2 * h, w2 = 2 * w;
  const int b = blockIdx.x / h, iy = blockIdx.x - b * h;
  for (int ix = threadIdx.x; ix < w; ix += blockDim.x) {
    int nlo, nhi, plo, phi, plo2, phi2;
    cand_range(s1w, ix, w2, nlo, nhi);
    cand_range(s2w, nlo, tw, plo, phi2);
    cand_range(s2w, nhi, tw, plo2, phi);
    plo = min(plo, plo2);
    phi = max(phi, phi2);
    trim_range(plo, phi, [&](int o) { return comb_w(s2w, o, w2, s1w, w, ix); });
    xlo[ix] = plo;
    xn[ix] = phi - plo + 1;
#pragma unroll
    for (int k = 0; k < RS_W; ++k)
      xw[ix * RS_W + k] = plo + k <= phi ? comb_w(s2w, plo + k, w2, s1w, w, ix) : 0.f;
  }
  if (threadIdx.x == 0) {
    int mlo, mhi, olo, ohi, olo2, ohi2;
    cand_range(s1h, iy, h2, mlo, mhi);
    cand_range(s2h, mlo, th, olo, ohi2);
    cand_range(s2h, mhi, th, olo2, ohi);
    olo = min(olo, olo2);
    ohi = max(ohi, ohi2);
    trim_range(olo, ohi, [&](int o) { return comb_w(s2h, o, h2, s1h, h, iy); });
    ywin[0] = olo;
    ywin[1] = ohi;
#pragma unroll
    for (int k = 0; k < RS_W; ++k) yw[k] = olo + k <= ohi ? comb_w(s2h, olo + k, h2, s1h, h, iy) : 0.f;
  }
  __syncthreads();
  const int olo = ywin[0], ohi = ywin[1];
  const T* base = dy + (size_t)b * th * tw * C;
  T* orow = dx + ((size_t)b * h + iy) * w * C;
  const uint32_t items = (uint32_t)w * (uint32_t)C8;
  BnRedAcc ra;
  if (RED) ra.init(rp, (threadIdx.x % C8) * 8);
  for (uint32_t it = threadIdx.x; it < items; it += blockDim.x) {
    const int ix = (int)fdiv(it, fdC8);
    const int c = (int)(it - (uint32_t)ix * (uint32_t)C8) * 8;
    const int plo = xlo[ix], n = xn[ix];
    F8 acc = f8zero();
    if (n <= RS_W && ohi - olo < RS_W) {
      float wx[RS_W];
      int xo[RS_W];
#pragma unroll
      for (int k = 0; k < RS_W; ++k) {
        wx[k] = xw[ix * RS_W + k];
        xo[k] = plo + min(k, n - 1);
      }
      for (int oy = olo; oy <= ohi; ++oy) {
        const float wy = yw[oy - olo];
        if (wy != 0.f) gather_row(acc, base + (size_t)oy * tw * C + c, C, wy, wx, xo);
      }
    } else {  // wide windows: weights on the fly, as the per-element kernel
      for (int oy = olo; oy <= ohi; ++oy) {
        const float wy = comb_w(s2h, oy, h2, s1h, h, iy);
        if (wy == 0.f) continue;
        const T* row = base + (size_t)oy * tw * C + c;
        for (int ox = plo; ox < plo + n; ++ox) {
          const float wxk = comb_w(s2w, ox, w2, s1w, w, ix);
          if (wxk != 0.f) acc += (wy * wxk) * ld8(row + (size_t)ox * C);
        }
      }
    }
    st8(orow + (size_t)ix * C + c, acc);
    if (RED) ra.add<T>(rp, as_stored8<T>(acc), ((size_t)b * h + iy) * w + ix, C, c);
  }
  if (RED) ra.write(rp, C8);
}

// Row-blocked single-step resize backward (same scheme as the composite's).
template <typename T, bool RED>
__global__ void __launch_bounds__(256) resize_bwd_rows_kernel(
    const T* __restrict__ dy, int h, int w, int C8, FastDiv fdC8, T* __restrict__ dx, int th,
    int tw, float sh, float sw, BnRedP rp) {
  extern __shared__ float rs_tables[];  // [w][RS_W] weights, [w] window starts, [w] widths
  float* xw = rs_tables;
  int* xlo = (int*)(rs_tables + (size_t)w * RS_W);
  int* xn = xlo + w;
  __shared__ float yw[RS_W];
  __shared__ int ywin[2];
  const int C = C8 * 8;
  const int b = blockIdx.x / h, iy = blockIdx.x - b * h;
  for (int ix = threadIdx.x; ix < w; ix += blockDim.x) {
    int plo, phi;
    cand_range(sw, ix, tw, plo, phi);
    trim_range(plo, phi, [&](int o) { return lin_w(sw, o, w, ix); });
    xlo[ix] = plo;
    xn[ix] = phi - plo + 1;
#pragma unroll
    for (int k = 0; k < RS_W; ++k)
      xw[ix * RS_W + k] = plo + k <= phi ? lin_w(sw, plo + k, w, ix) : 0.f;
  }
  if (threadIdx.x == 0) {
    int olo, ohi;
    cand_range(sh, iy, th, olo, ohi);
    trim_range(olo, ohi, [&](int o) { return lin_w(sh, o, h, iy); });
    ywin[0] = olo;
    ywin[1] = ohi;
#pragma unroll
    for (int k = 0; k < RS_W; ++k) yw[k] = olo + k <= ohi ? lin_w(sh, olo + k, h, iy) : 0.f;
  }
  __syncthreads();
  const int olo = ywin[0], ohi = ywin[1];
  const T* base = dy + (size_t)b * th * tw * C;
  T* orow = dx + ((size_t)b * h + iy) * w * C;
  const uint32_t items = (uint32_t)w * (uint32_t)C8;
  BnRedAcc ra;
  if (RED) ra.init(rp, (threadIdx.x % C8) * 8);
  for (uint32_t it = threadIdx.x; it < items; it += blockDim.x) {
    const int ix = (int)fdiv(it, fdC8);
    const int c = (int)(it - (uint32_t)ix * (uint32_t)C8) * 8;
    const int plo = xlo[ix], n = xn[ix];
    F8 acc = f8zero();
    if (n <= RS_W && ohi - olo < RS_W) {
      float wx[RS_W];
      int xo[RS_W];
#pragma unroll
      for (int k = 0; k < RS_W; ++k) {
        wx[k] = xw[ix * RS_W + k];
        xo[k] = plo + min(k, n - 1);
      }
      for (int oy = olo; oy <= ohi; ++oy) {
        const float wy = yw[oy - olo];
        if (wy != 0.f) gather_row(acc, base + (size_t)oy * tw * C + c, C, wy, wx, xo);
      }
    } else {  // wide windows: weights on the fly, as the per-element kernel
      for (int oy = olo; oy <= ohi; ++oy) {
        const float wy = lin_w(sh, oy, h, iy);
        if (wy == 0.f) continue;
        const T* row = base + (size_t)oy * tw * C + c;
        for (int ox = plo; ox < plo + n; ++ox) {
          const float wxk = lin_w(sw, ox, w, ix);
          if (wxk != 0.f) acc += (wy * wxk) * ld8(row + (size_t)ox * C);
        }
      }
    }
    st8(orow + (size_t)ix * C + c, acc);
    if (RED) ra.add<T>(rp, as_stored8<T>(acc), ((size_t)b * h + iy) * w + ix, C, c);
  }
  if (RED) ra.write(rp, C8);
}

// Separable row-blocked backward of a bilinear upsample: the single resize
// (COMP false: nn.Upsample x2, Unetmodel.py:122-134) or the x2 + match
// composite (COMP true: up9, :140-141). Grid = (input row, channel slice).
// Phase 1 sums the block's dY rows (its y window) with their weights into an
// fp32 LDS row [tw][cb] — every dY element is loaded once per block with
// 16-B vector loads; phase 2 gathers each input column's x window from LDS.
// The 2-D gather form issued RS_W x-taps per dY row per output (~24 vector
// loads per output) and was load-issue bound at 2.2-2.9 TB/s.
__device__ __forceinline__ void comp_window(float s1, float s2, int i, int n1, int out, int& lo,
                                            int& hi) {
  int mlo, mhi, lo2, hi2;
  cand_range(s1, i, 2 * n1, mlo, mhi);
  cand_range(s2, mlo, out, lo, hi2);
  cand_range(s2, mhi, out, lo2, hi);
  lo = min(lo, lo2);
  hi = max(hi, hi2);
}

template <bool COMP>
__device__ __forceinline__ float sep_w(float s1, float s2, int o, int n1, int i) {
  if constexpr (COMP) return comb_w(s2, o, 2 * n1, s1, n1, i);
  return lin_w(s1, o, n1, i);
}

template <bool COMP>
__device__ __forceinline__ void sep_window(float s1, float s2, int i, int n1, int out, int& lo,
                                           int& hi) {
  if constexpr (COMP) comp_window(s1, s2, i, n1, out, lo, hi);
  else cand_range(s1, i, out, lo, hi);
  trim_range(lo, hi, [&](int o) { return sep_w<COMP>(s1, s2, o, n1, i); });
}

constexpr int SEP_YW = 32;  // union-window y weights kept per row (wider: computed per use)

// R consecutive input rows per block share one pass over the dY rows of
// their union window: each dY row is loaded once per block (a x2 upsample
// spreads a dY row over 2 input rows, the composite over ~3, so one row per
// block re-read dY 2-3x) and accumulated into R LDS rows.
template <typename T, bool RED, bool COMP, int R>
__global__ void __launch_bounds__(256) resize_bwd_sep_kernel(
    const T* __restrict__ dy, int h, int w, int C, int lcb8, T* __restrict__ dx, int th, int tw,
    float s1h, float s1w, float s2h, float s2w, BnRedP rp) {
  // [R][tw][cb] row sums, [w][RS_W] x weights, [w] window starts, [w] widths
  extern __shared__ float sep_lds[];
  __shared__ float yw[R][SEP_YW];
  __shared__ int ywin[2];
  const int cb8 = 1 << lcb8, cb = cb8 * 8;
  float* vrow = sep_lds;
  float* xw = sep_lds + (size_t)R * tw * cb;
  int* xlo = (int*)(xw + (size_t)w * RS_W);
  int* xn = xlo + w;
  const int tid = threadIdx.x;
  const int hb = (h + R - 1) / R;
  const int b = blockIdx.x / hb, iy0 = (blockIdx.x - b * hb) * R;
  const int nr = min(R, h - iy0);
  const int c0 = blockIdx.y * cb;
  for (int ix = tid; ix < w; ix += blockDim.x) {
    int lo, hi;
    sep_window<COMP>(s1w, s2w, ix, w, tw, lo, hi);
    xlo[ix] = lo;
    xn[ix] = hi - lo + 1;
#pragma unroll
    for (int k = 0; k < RS_W; ++k)
      xw[ix * RS_W + k] = lo + k <= hi ? sep_w<COMP>(s1w, s2w, lo + k, w, ix) : 0.f;
  }
  if (tid == 0) {
    int lo, hi, lo2, hi2;
    sep_window<COMP>(s1h, s2h, iy0, h, th, lo, hi);
    sep_window<COMP>(s1h, s2h, iy0 + nr - 1, h, th, lo2, hi2);
    ywin[0] = min(lo, lo2);
    ywin[1] = max(hi, hi2);
  }
  __syncthreads();
  const int olo = ywin[0], ny = ywin[1] - ywin[0] + 1;
  // weight of union-window row k on input row iy0 + r (0 outside its window)
  if (tid < R * SEP_YW) {
    const int r = tid / SEP_YW, k = tid % SEP_YW;
    yw[r][k] = (r < nr && k < ny) ? sep_w<COMP>(s1h, s2h, olo + k, h, iy0 + r) : 0.f;
  }
  __syncthreads();
  // phase 1: vrow[r][ox][c] = sum_oy wy(oy, iy0 + r) dY[b][oy][ox][c0 + c]
  const T* base = dy + (size_t)b * th * tw * C + c0;
  const size_t rstride = (size_t)tw * C;
  const uint32_t items1 = (uint32_t)tw << lcb8;
  for (uint32_t it = tid; it < items1; it += blockDim.x) {
    const int ox = (int)(it >> lcb8), c = (int)(it & (cb8 - 1)) * 8;
    const T* p = base + (size_t)olo * rstride + (size_t)ox * C + c;
    F8 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = f8zero();
    auto add = [&](const F8& v, int k) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float wk = k < SEP_YW ? yw[r][k]
                                    : (r < nr ? sep_w<COMP>(s1h, s2h, olo + k, h, iy0 + r) : 0.f);
        const F8 t = acc[r] + wk * v;  // a zero weight must not pass an Inf / NaN on
        acc[r].a = wk != 0.f ? t.a : acc[r].a;
        acc[r].b = wk != 0.f ? t.b : acc[r].b;
      }
    };
    int k = 0;
    for (; k + 1 < ny; k += 2) {  // two rows' loads in flight
      const F8 v0 = ld8(p + (size_t)k * rstride), v1 = ld8(p + (size_t)(k + 1) * rstride);
      add(v0, k);
      add(v1, k + 1);
    }
    if (k < ny) add(ld8(p + (size_t)k * rstride), k);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float* q = &vrow[((size_t)r * tw + ox) * cb + c];
      *(f32x4*)q = acc[r].a;
      *(f32x4*)(q + 4) = acc[r].b;
    }
  }
  __syncthreads();
  // phase 2: dx[b][iy0 + r][ix][c0 + c] = sum_k wx(ix, k) vrow[r][xlo + k][c]
  const uint32_t items2 = (uint32_t)w << lcb8;
  for (int r = 0; r < nr; ++r) {
    const int iy = iy0 + r;
    T* orow = dx + ((size_t)b * h + iy) * w * C + c0;
    const float* vr = vrow + (size_t)r * tw * cb;
    BnRedAcc ra;
    if (RED) ra.init(rp, c0 + (tid & (cb8 - 1)) * 8);
    for (uint32_t it = tid; it < items2; it += blockDim.x) {
      const int ix = (int)(it >> lcb8), c = (int)(it & (cb8 - 1)) * 8;
      const int lo = xlo[ix], n = xn[ix];
      F8 acc = f8zero();
      if (n <= RS_W) {
#pragma unroll
        for (int k = 0; k < RS_W; ++k)
          if (k < n) acc += xw[ix * RS_W + k] * ld8(&vr[(lo + k) * cb + c]);
      } else {
        for (int k = 0; k < n; ++k)
          acc += sep_w<COMP>(s1w, s2w, lo + k, w, ix) * ld8(&vr[(lo + k) * cb + c]);
      }
      st8(orow + (size_t)ix * C + c, acc);
      if (RED) ra.add<T>(rp, as_stored8<T>(acc), ((size_t)b * h + iy) * w + ix, C, c0 + c);
    }
    // partial row b * h + iy (the B * h rows nsm_bnred_chunks reports)
    if (RED) ra.write_slice(rp, cb8, c0, C, b * h + iy);
  }
}

// channel slice of the separable kernels: the widest power-of-two multiple
// of 8 channels dividing C (at most 256 groups) whose fp32 LDS rows (rows x
// width x cb) fit `budget` bytes; -1 if 8 channels do not fit
static int sep_lcb8(int C, int width, int rows = 1, size_t budget = 32768) {
  int l = 0;
  while ((8 << (l + 1)) <= C && C % (8 << (l + 1)) == 0 &&
         (size_t)rows * width * (8 << (l + 1)) * 4 <= budget && (1 << (l + 1)) <= 256)
    ++l;
  if ((size_t)rows * width * (8 << l) * 4 > budget) return -1;
  return l;
}
// the backward's rows per block and channel slice: 4 rows where a 32-channel
// (fp32 128-B) slice still fits 48 KiB, else 2, else 1
struct SepPlan {
  int R, lcb8;
};
// NSM_SEP_RMAX: cap on the rows per block. 2 by measurement (tools/
// elem_bench_f32.py, B=8 fp32): R = 2 vs 1 cuts the x2 backward 126 -> 110 us
// (C=512), and R = 4 is no faster without the fused BN reduction and slower
// with it (124 -> 145 us: four partial-row reductions per block)
static int sep_rmax() { static const int v = (int)env_int("NSM_SEP_RMAX", 2); return v; }
// NSM_SEP_LDS_KB: the LDS budget of the backward's fp32 row sums per block
// (64 KiB: two blocks per CU; 16 / 32 measured slower, B=8 fp32 step)
static size_t sep_lds_budget() {
  static const size_t v = (size_t)(int)env_int("NSM_SEP_LDS_KB", 64) * 1024;
  return v;
}
static SepPlan sep_bwd_plan(int C, int tw) {
  const size_t budget = sep_lds_budget();
  for (int R : {4, 2}) {
    if (R > sep_rmax()) continue;
    const int l = sep_lcb8(C, tw, R, budget);
    if (l >= 2 || (l >= 0 && (8 << l) == C)) return SepPlan{R, l};
  }
  return SepPlan{1, sep_lcb8(C, tw, 1, budget)};
}
// dynamic LDS above the default 64 KiB (gfx950: 160 KiB per workgroup)
template <typename K>
static void allow_big_lds(K kernel) {
  static const bool once = [&] {
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              120 * 1024);
    return true;
  }();
  (void)once;
}
template <typename T, bool RED, bool COMP, int R>
static void launch_sep_bwd(dim3 g, size_t lds, hipStream_t s, const void* dy, int h, int w, int C,
                           int lcb8, void* dx, int th, int tw, float s1h, float s1w, float s2h,
                           float s2w, const BnRedP& rp) {
  auto k = resize_bwd_sep_kernel<T, RED, COMP, R>;
  allow_big_lds(k);
  hipLaunchKernelGGL(k, g, dim3(256), lds, s, (const T*)dy, h, w, C, lcb8, (T*)dx, th, tw, s1h,
                     s1w, s2h, s2w, rp);
}
// rp (the fused BN reduction) and the plan's rows per block as template arguments
template <typename T, bool COMP>
static void dispatch_sep_bwd(const SepPlan& pl, int B, size_t lds, hipStream_t s, const void* dy,
                             int h, int w, int C, void* dx, int th, int tw, float s1h, float s1w,
                             float s2h, float s2w, const BnRedP* rp) {
  const dim3 g((unsigned)(B * ((h + pl.R - 1) / pl.R)), (unsigned)(C >> (pl.lcb8 + 3)));
  const BnRedP r = rp ? *rp : BnRedP{};
  for_bool(rp != nullptr, [&](auto red) {
    auto rows = [&](auto R) {
      launch_sep_bwd<T, decltype(red)::value, COMP, decltype(R)::value>(
          g, lds, s, dy, h, w, C, pl.lcb8, dx, th, tw, s1h, s1w, s2h, s2w, r);
      return 0;
    };
    using std::integral_constant;
    return pl.R == 4   ? rows(integral_constant<int, 4>{})
           : pl.R == 2 ? rows(integral_constant<int, 2>{})
                       : rows(integral_constant<int, 1>{});
  });
}
// fp32 only: in bf16 (16-B lanes, half the bytes per pixel) the 2-D gather
// forms measured faster (B=64: x2 backward 401 vs 675 us, composite forward
// 366 vs 541 us; 1080p eval 505 vs 457 frames/s)
// (NSM_RESIZE_SEP=2: the separable forms for the 16-bit storage too; measured
// slower again in round 6: B=64 bf16 x2 backward 516 -> 773 us at conv8)
static int sep_resize_mode() { static const int v = (int)env_int("NSM_RESIZE_SEP", 1); return v; }
static bool sep_resize() { return sep_resize_mode() != 0; }
static bool sep_for(int dtype) { return dtype == NSM_F32 ? sep_resize() : sep_resize_mode() == 2; }

// grid for the xcd_block() kernels: a multiple of 8 blocks, <= 2048
static inline int xcd_grid(long long work) {
  long long g = (work + 255) / 256;
  g = g > 2048 ? 2048 : g;
  return (int)((g + 7) / 8 * 8);
}

}  // namespace nsm

using namespace nsm;

// ============================== C ABI ======================================
extern "C" int nsm_bn_act_pool(const void* y, int B, int H, int W, int C, const float* scale,
                               const float* shift, float slope, void* z, void* pooled, int dtype,
                               uint32_t* amax, void* stream) {
  NSM_CHECK_ARG(y && z && pooled && scale && shift && C % 8 == 0 && H >= 2 && W >= 2,
                "bn_act_pool: bad args");
  const long long work = (long long)B * ((H + 1) / 2) * ((W + 1) / 2) * (C / 8);
  NSM_CHECK_ARG(work < (1ll << 31), "bn_act_pool: too large");
  dim3 g(grid_for(work));
  const FastDiv f8 = make_fastdiv(C / 8), fw = make_fastdiv((W + 1) / 2),
                fh = make_fastdiv((H + 1) / 2);
  return for_dtype(dtype, "bn_act_pool", [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(bn_act_pool_kernel<T>, g, dim3(256), 0, as_stream(stream), (const T*)y, B,
                       H, W, C / 8, f8, fw, fh, scale, shift, slope, (T*)z, (T*)pooled, amax);
    NSM_LAUNCH_CHECK("bn_act_pool");
    return 0;
  });
}

extern "C" int nsm_avgpool2_fwd(const void* x, int B, int H, int W, int C, void* y, int dtype,
                                void* stream) {
  NSM_CHECK_ARG(x && y && C % 8 == 0 && H >= 2 && W >= 2, "avgpool2_fwd: bad args");
  long long work = (long long)B * (H / 2) * (W / 2) * (C / 8);
  NSM_CHECK_ARG(work < (1ll << 31), "avgpool2_fwd: too large");
  dim3 g(grid_for(work));
  const FastDiv f8 = make_fastdiv(C / 8), fw = make_fastdiv(W / 2), fh = make_fastdiv(H / 2);
  return for_dtype(dtype, "avgpool2_fwd", [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(avgpool2_fwd_kernel<T>, g, dim3(256), 0, as_stream(stream), (const T*)x, B,
                       H, W, C / 8, f8, fw, fh, (T*)y);
    NSM_LAUNCH_CHECK("avgpool2_fwd");
    return 0;
  });
}

// Blocks of the fused-reduction form: at most one chip-wide pass of 8 waves per
// SIMD (2048 blocks of 256), so every block folds several pixels into its
// partial row. At 8192 blocks the conv4-level call (64x64, 512 channels) ran one
// pixel per thread and wrote 4 KB of partials per block: 33.5 MB, half the size
// of dx, written and read back by the merge
static inline int pool_bnred_grid(long long work) { return grid_for(work, 256, 2048); }

static int avgpool2_bwd_add(const void* dy, int B, int H, int W, int C, const void* skip, void* dx,
                            int dtype, const BnRedP* rp, void* stream) {
  NSM_CHECK_ARG(dy && dx && C % 8 == 0, "avgpool2_bwd: bad args");
  long long work = (long long)B * H * W * (C / 8);
  NSM_CHECK_ARG(work < (1ll << 31), "avgpool2_bwd: too large");
  NSM_CHECK_ARG(!rp || 256 % (C / 8) == 0, "avgpool2_bwd: fused BN reduction needs C/8 | 256");
  dim3 g(rp ? pool_bnred_grid(work) : grid_for(work));  // rp: the rows nsm_bnred_chunks reports
  const FastDiv f8 = make_fastdiv(C / 8), fw = make_fastdiv(W), fh = make_fastdiv(H);
  const BnRedP r = rp ? *rp : BnRedP{};
  return for_dtype(dtype, "avgpool2_bwd", [&](auto t) {
    using T = typename decltype(t)::type;
    return for_bool(rp != nullptr, [&](auto red) {
      hipLaunchKernelGGL((avgpool2_bwd_add_kernel<T, decltype(red)::value>), g, dim3(256), 0,
                         as_stream(stream), (const T*)dy, B, H, W, C / 8, f8, fw, fh,
                         (const T*)skip, (T*)dx, r);
      NSM_LAUNCH_CHECK("avgpool2_bwd");
      return 0;
    });
  });
}

extern "C" int nsm_avgpool2_bwd_add(const void* dy, int B, int H, int W, int C, const void* skip,
                                    void* dx, int dtype, void* stream) {
  return avgpool2_bwd_add(dy, B, H, W, C, skip, dx, dtype, nullptr, stream);
}

// NSM_RESIZE_ROWS=0: per-element resize backward instead of the row-blocked one
static bool rows_resize() { static const bool v = env_flag("NSM_RESIZE_ROWS", true); return v; }

// 8-channel path when C % 8 == 0 (all model activations), scalar otherwise
extern "C" int nsm_resize_fwd(const void* x, int B, int Hi, int Wi, int C, void* y, int Ho, int Wo,
                              int dtype, void* stream) {
  NSM_CHECK_ARG(x && y && B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0,
                "resize_fwd: bad args");
  const float sh = ac_scale(Hi, Ho), sw = ac_scale(Wi, Wo);
  hipStream_t s = as_stream(stream);
  const long long tot8 = (long long)B * Ho * Wo * (C / 8);
  return for_dtype(dtype, "resize_fwd", [&](auto t) {
    using T = typename decltype(t)::type;
    if (C % 8 == 0 && tot8 < (1ll << 31)) {
      const FastDiv f8 = make_fastdiv(C / 8), fw = make_fastdiv(Wo), fh = make_fastdiv(Ho);
      hipLaunchKernelGGL(resize_fwd8_kernel<T>, dim3(xcd_grid(tot8)), dim3(256), 0, s,
                         (const T*)x, Hi, Wi, C / 8, (uint32_t)tot8, f8, fw, fh, (T*)y, Ho, Wo, sh,
                         sw);
    } else {
      hipLaunchKernelGGL(resize_fwd1_kernel<T>, dim3(grid_for((long long)B * Ho * Wo * C)),
                         dim3(256), 0, s, (const T*)x, B, Hi, Wi, C, (T*)y, Ho, Wo, sh, sw);
    }
    NSM_LAUNCH_CHECK("resize_fwd");
    return 0;
  });
}

static int resize_bwd(const void* dy, int B, int Hi, int Wi, int C, void* dx, int Ho, int Wo,
                      int dtype, const BnRedP* rp, void* stream) {
  NSM_CHECK_ARG(dy && dx && B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0,
                "resize_bwd: bad args");
  const float sh = ac_scale(Hi, Ho), sw = ac_scale(Wi, Wo);
  hipStream_t s = as_stream(stream);
  const long long tot8 = (long long)B * Hi * Wi * (C / 8);
  const BnRedP r = rp ? *rp : BnRedP{};
  return for_dtype(dtype, "resize_bwd", [&](auto t) {
    using T = typename decltype(t)::type;
    if (C % 8 == 0 && tot8 < (1ll << 31)) {
      const FastDiv f8 = make_fastdiv(C / 8), fw = make_fastdiv(Wi), fh = make_fastdiv(Hi);
      const SepPlan pl = sep_bwd_plan(C, Wo);
      const size_t slds = pl.lcb8 < 0 ? 0
                                      : (size_t)pl.R * Wo * (8 << pl.lcb8) * 4 +
                                            (size_t)Wi * (RS_W + 2) * 4;
      if (sep_for(dtype) && pl.lcb8 >= 0 && slds <= 96 * 1024 && (long long)B * Hi < (1ll << 31)) {
        dispatch_sep_bwd<T, false>(pl, B, slds, s, dy, Hi, Wi, C, dx, Ho, Wo, sh, sw, 0.f, 0.f, rp);
      } else if (Wi <= U2_MAXW && (long long)B * Hi < (1ll << 31) && rows_resize()) {
        NSM_CHECK_ARG(!rp || 256 % (C / 8) == 0, "resize_bwd: fused BN reduction needs C/8 | 256");
        const size_t lds = (size_t)Wi * (RS_W + 2) * 4;
        const dim3 gr((unsigned)(B * Hi));
        for_bool(rp != nullptr, [&](auto red) {
          hipLaunchKernelGGL((resize_bwd_rows_kernel<T, decltype(red)::value>), gr, dim3(256), lds,
                             s, (const T*)dy, Hi, Wi, C / 8, f8, (T*)dx, Ho, Wo, sh, sw, r);
          return 0;
        });
      } else {
        NSM_CHECK_ARG(!rp, "resize_bwd: fused BN reduction needs the row-blocked kernel");
        hipLaunchKernelGGL(resize_bwd8_kernel<T>, dim3(xcd_grid(tot8)), dim3(256), 0, s,
                           (const T*)dy, Hi, Wi, C / 8, (uint32_t)tot8, f8, fw, fh, (T*)dx, Ho, Wo,
                           sh, sw);
      }
    } else {
      NSM_CHECK_ARG(!rp, "resize_bwd: fused BN reduction needs C % 8 == 0");
      hipLaunchKernelGGL(resize_bwd1_kernel<T>, dim3(grid_for((long long)B * Hi * Wi * C)),
                         dim3(256), 0, s, (const T*)dy, B, Hi, Wi, C, (T*)dx, Ho, Wo, sh, sw);
    }
    NSM_LAUNCH_CHECK("resize_bwd");
    return 0;
  });
}

extern "C" int nsm_resize_bwd(const void* dy, int B, int Hi, int Wi, int C, void* dx, int Ho, int Wo,
                              int dtype, void* stream) {
  return resize_bwd(dy, B, Hi, Wi, C, dx, Ho, Wo, dtype, nullptr, stream);
}

// ---- upsample of a decoder block output that is never materialised ---------
extern "C" int nsm_resize_fwd_act(const void* y2, int B, int Hi, int Wi, int C, void* out, int Ho,
                                  int Wo, const float* scale, const float* shift, float slope,
                                  const void* res, int dtype, void* stream) {
  NSM_CHECK_ARG(y2 && out && scale && shift && B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 &&
                    C % 8 == 0, "resize_fwd_act: bad args");
  const long long tot8 = (long long)B * Ho * Wo * (C / 8);
  NSM_CHECK_ARG(tot8 < (1ll << 31), "resize_fwd_act: too large");
  const float sh = ac_scale(Hi, Ho), sw = ac_scale(Wi, Wo);
  dim3 g(xcd_grid(tot8));
  const FastDiv f8 = make_fastdiv(C / 8), fw = make_fastdiv(Wo), fh = make_fastdiv(Ho);
  const ActSrc act{scale, shift, res, slope};
  return for_dtype(dtype, "resize_fwd_act", [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((resize_fwd8_kernel<T, true>), g, dim3(256), 0, as_stream(stream),
                       (const T*)y2, Hi, Wi, C / 8, (uint32_t)tot8, f8, fw, fh, (T*)out, Ho, Wo,
                       sh, sw, act);
    NSM_LAUNCH_CHECK("resize_fwd_act");
    return 0;
  });
}

// The row-blocked composite forward (ACT: the `_act` entry's act-on-load
// source): the separable form where it applies, else the 3x3-stencil rows
template <typename T, bool ACT>
static void up2_fwd_rows(const void* x, int B, int h, int w, int C, void* y, int th, int tw,
                         float a, float b, float c, float d, const ActSrc& act, int dtype,
                         hipStream_t s) {
  const size_t lds = (size_t)tw * 4 * 4;
  // row segments: >= ~2048 blocks when B * th is small (1080p inference: 135 rows)
  const long long rows = (long long)B * th, per_row = (long long)tw * (C / 8);
  long long segs = (2048 + rows - 1) / rows;
  segs = std::max(1ll, std::min({segs, 16ll, (per_row + 1023) / 1024}));
  const dim3 gr((unsigned)rows, (unsigned)segs);
  const int lcb8 = sep_lcb8(C, w);
  const size_t slds = lcb8 < 0 ? 0 : (size_t)w * (8 << lcb8) * 4 + (size_t)tw * 16;
  if (sep_for(dtype) && lcb8 >= 0 && slds <= 65536) {
    const dim3 gs((unsigned)rows, (unsigned)(C / (8 << lcb8)));
    hipLaunchKernelGGL((up2_resize_fwd_sep_kernel<T, ACT>), gs, dim3(256), slds, s, (const T*)x, h,
                       w, C, lcb8, (T*)y, th, tw, a, b, c, d, act);
  } else {
    hipLaunchKernelGGL((up2_resize_fwd_rows_kernel<T, ACT>), gr, dim3(256), lds, s, (const T*)x, h,
                       w, C / 8, make_fastdiv(C / 8), (T*)y, th, tw, a, b, c, d, act);
  }
}

extern "C" int nsm_up2_resize_fwd_act(const void* y2, int B, int h, int w, int C, void* out,
                                      int th, int tw, const float* scale, const float* shift,
                                      float slope, const void* res, int dtype, void* stream) {
  NSM_CHECK_ARG(y2 && out && scale && shift && B > 0 && h > 0 && w > 0 && th > 0 && tw > 0 &&
                    C % 8 == 0, "up2_resize_fwd_act: bad args");
  const long long tot8 = (long long)B * th * tw * (C / 8);
  NSM_CHECK_ARG(tot8 < (1ll << 31), "up2_resize_fwd_act: too large");
  NSM_CHECK_ARG(tw <= U2_MAXW && (long long)B * th < (1ll << 31) && th * 2 >= 2 * h - 1 &&
                    tw * 2 >= 2 * w - 1, "up2_resize_fwd_act: needs the row-blocked kernel");
  const float a = ac_scale(h, 2 * h), b = ac_scale(w, 2 * w), c = ac_scale(2 * h, th),
              d = ac_scale(2 * w, tw);
  const ActSrc act{scale, shift, res, slope};
  return for_dtype(dtype, "up2_resize_fwd_act", [&](auto t) {
    using T = typename decltype(t)::type;
    up2_fwd_rows<T, true>(y2, B, h, w, C, out, th, tw, a, b, c, d, act, dtype, as_stream(stream));
    NSM_LAUNCH_CHECK("up2_resize_fwd_act");
    return 0;
  });
}

extern "C" int nsm_up2_resize_fwd(const void* x, int B, int h, int w, int C, void* y, int th,
                                  int tw, int dtype, void* stream) {
  NSM_CHECK_ARG(x && y && B > 0 && h > 0 && w > 0 && th > 0 && tw > 0 && C % 8 == 0,
                "up2_resize_fwd: bad args");
  const long long tot8 = (long long)B * th * tw * (C / 8);
  NSM_CHECK_ARG(tot8 < (1ll << 31), "up2_resize_fwd: too large");
  hipStream_t s = as_stream(stream);
  const float a = ac_scale(h, 2 * h), b = ac_scale(w, 2 * w), c = ac_scale(2 * h, th),
              d = ac_scale(2 * w, tw);
  return for_dtype(dtype, "up2_resize_fwd", [&](auto t) {
    using T = typename decltype(t)::type;
    if (tw <= U2_MAXW && (long long)B * th < (1ll << 31) && th * 2 >= 2 * h - 1 &&
        tw * 2 >= 2 * w - 1) {
      // second step downsizes (or keeps) the x2 grid: the 3-tap collapse holds
      up2_fwd_rows<T, false>(x, B, h, w, C, y, th, tw, a, b, c, d, ActSrc{}, dtype, s);
    } else {
      const FastDiv f8 = make_fastdiv(C / 8), fw = make_fastdiv(tw), fh = make_fastdiv(th);
      hipLaunchKernelGGL(up2_resize_fwd8_kernel<T>, dim3(xcd_grid(tot8)), dim3(256), 0, s,
                         (const T*)x, h, w, C / 8, (uint32_t)tot8, f8, fw, fh, (T*)y, th, tw, a, b,
                         c, d);
    }
    NSM_LAUNCH_CHECK("up2_resize_fwd");
    return 0;
  });
}

static int up2_resize_bwd(const void* dy, int B, int h, int w, int C, void* dx, int th, int tw,
                          int dtype, const BnRedP* rp, void* stream) {
  NSM_CHECK_ARG(dy && dx && B > 0 && h > 0 && w > 0 && th > 0 && tw > 0 && C % 8 == 0,
                "up2_resize_bwd: bad args");
  const long long tot8 = (long long)B * h * w * (C / 8);
  NSM_CHECK_ARG(tot8 < (1ll << 31), "up2_resize_bwd: too large");
  hipStream_t s = as_stream(stream);
  const float a = ac_scale(h, 2 * h), b = ac_scale(w, 2 * w), c = ac_scale(2 * h, th),
              d = ac_scale(2 * w, tw);
  const FastDiv f8 = make_fastdiv(C / 8), fw = make_fastdiv(w), fh = make_fastdiv(h);
  const BnRedP r = rp ? *rp : BnRedP{};
  const SepPlan pl = sep_bwd_plan(C, tw);
  const size_t slds = pl.lcb8 < 0 ? 0
                                  : (size_t)pl.R * tw * (8 << pl.lcb8) * 4 +
                                        (size_t)w * (RS_W + 2) * 4;
  return for_dtype(dtype, "up2_resize_bwd", [&](auto t) {
    using T = typename decltype(t)::type;
    if (sep_for(dtype) && pl.lcb8 >= 0 && slds <= 96 * 1024 && (long long)B * h < (1ll << 31)) {
      dispatch_sep_bwd<T, true>(pl, B, slds, s, dy, h, w, C, dx, th, tw, a, b, c, d, rp);
    } else if (w <= U2_MAXW && (long long)B * h < (1ll << 31)) {
      NSM_CHECK_ARG(!rp || 256 % (C / 8) == 0, "up2_resize_bwd: fused BN reduction needs C/8 | 256");
      const size_t lds = (size_t)w * (RS_W + 2) * 4;
      const dim3 gr((unsigned)(B * h));
      for_bool(rp != nullptr, [&](auto red) {
        hipLaunchKernelGGL((up2_resize_bwd_rows_kernel<T, decltype(red)::value>), gr, dim3(256),
                           lds, s, (const T*)dy, h, w, C / 8, f8, (T*)dx, th, tw, a, b, c, d, r);
        return 0;
      });
    } else {
      NSM_CHECK_ARG(!rp, "up2_resize_bwd: fused BN reduction needs the row-blocked kernel");
      hipLaunchKernelGGL(up2_resize_bwd8_kernel<T>, dim3(xcd_grid(tot8)), dim3(256), 0, s,
                         (const T*)dy, h, w, C / 8, (uint32_t)tot8, f8, fw, fh, (T*)dx, th, tw, a,
                         b, c, d);
    }
    NSM_LAUNCH_CHECK("up2_resize_bwd");
    return 0;
  });
}

extern "C" int nsm_up2_resize_bwd(const void* dy, int B, int h, int w, int C, void* dx, int th,
                                  int tw, int dtype, void* stream) {
  return up2_resize_bwd(dy, B, h, w, C, dx, th, tw, dtype, nullptr, stream);
}

// ---- gradient producers with the fused BN-backward reduction (BnRedP) ----
// kind 0: nsm_avgpool2_bwd_add (H, W: dx's size), 1: nsm_resize_bwd (Hi, Wi),
// 2: nsm_up2_resize_bwd (h, w). Partial rows the call writes; 0 = the fused
// form does not apply (use the plain call + nsm_bn_bwd_reduce).
extern "C" int nsm_bnred_chunks(int kind, int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C % 8 || 256 % (C / 8)) return 0;
  if (kind == 0) {
    const long long work = (long long)B * H * W * (C / 8);
    return work < (1ll << 31) ? pool_bnred_grid(work) : 0;
  }
  if (kind == 1 && !rows_resize()) return 0;
  if ((kind == 1 || kind == 2) && W <= U2_MAXW && (long long)B * H < (1ll << 31) &&
      (long long)B * H * W * (C / 8) < (1ll << 31))
    return B * H;
  return 0;
}

#define NSM_BNRED_ARGS                                                                  \
  const void *y2, const float *scale, const float *shift, const float *mean,            \
      const float *invstd, float slope, float *partial, uint32_t *amax_k1dz
#define NSM_BNRED_CHECK(what)                                                           \
  NSM_CHECK_ARG(y2 && scale && shift && mean && invstd && partial, what ": null BN args"); \
  const BnRedP rp{y2, scale, shift, mean, invstd, slope, partial, amax_k1dz}

extern "C" int nsm_avgpool2_bwd_add_bnred(const void* dy, int B, int H, int W, int C,
                                          const void* skip, void* dx, int dtype, NSM_BNRED_ARGS,
                                          void* stream) {
  NSM_BNRED_CHECK("avgpool2_bwd_add_bnred");
  return avgpool2_bwd_add(dy, B, H, W, C, skip, dx, dtype, &rp, stream);
}
extern "C" int nsm_resize_bwd_bnred(const void* dy, int B, int Hi, int Wi, int C, void* dx, int Ho,
                                    int Wo, int dtype, NSM_BNRED_ARGS, void* stream) {
  NSM_BNRED_CHECK("resize_bwd_bnred");
  return resize_bwd(dy, B, Hi, Wi, C, dx, Ho, Wo, dtype, &rp, stream);
}
extern "C" int nsm_up2_resize_bwd_bnred(const void* dy, int B, int h, int w, int C, void* dx,
                                        int th, int tw, int dtype, NSM_BNRED_ARGS, void* stream) {
  NSM_BNRED_CHECK("up2_resize_bwd_bnred");
  return up2_resize_bwd(dy, B, h, w, C, dx, th, tw, dtype, &rp, stream);
}
#undef NSM_BNRED_ARGS
#undef NSM_BNRED_CHECK
