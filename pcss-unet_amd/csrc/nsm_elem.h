// What more than one of the element-wise units shares ("Element-wise
// sources"): nsm_bn.hip, nsm_resample.hip, nsm_vgg.hip, nsm_elem.hip. Anything
// only one of them uses lives in that unit.
//
// Streaming layout: every lane moves 8 consecutive channels (F8: one 16-B
// vector of bf16, two of fp32) and all index math is 32-bit with
// multiply-high division (no 64-bit divides in the loops).
#pragma once
#include "nsm_common.h"

namespace nsm {

// reduce red[rl][cl] (F8) over rl; result valid in red[0][tc] for all tc.
__device__ __forceinline__ void col_tree_reduce(F8* red, int cl, int rl, int tid) {
  for (int s = rl / 2; s > 0; s >>= 1) {
    __syncthreads();
    int tr = tid / cl;
    if (tr < s) red[tid] += red[tid + s * cl];
  }
  __syncthreads();
}

__device__ __forceinline__ F8 ldf8(const float* p) { return ld8(p); }  // fp32 parameter vectors

__device__ __forceinline__ f32x4 lrelu4(f32x4 v, float slope) {
  return f32x4{lrelu(v.x, slope), lrelu(v.y, slope), lrelu(v.z, slope), lrelu(v.w, slope)};
}
__device__ __forceinline__ F8 lrelu8(F8 v, float slope) {
  return F8{lrelu4(v.a, slope), lrelu4(v.b, slope)};
}

// A1 = lrelu(y*scale+shift) (* mask[b][c], Dropout2d) of 8 channels as the h2
// words h, l at scale s: the arithmetic of nsm_bn_act_h2, which the fused 1x1
// forward (gemm_h2a_kernel, nsm_conv_h2d.inc) shares so that its A1 stays
// bitwise the same
__device__ __forceinline__ void bn_act_h2_8(F8 y, F8 sc, F8 sh, float slope, bool masked, F8 mk,
                                            float s, u32x4& h, u32x4& l) {
  F8 o = lrelu8(y * sc + sh, slope);
  if (masked) o = o * mk;
  h2_split8(o, s, h, l);
}

// dz = g * mask[b][c] * lrelu'(y*scale+shift)
__device__ __forceinline__ f32x4 lrelu_grad4(f32x4 z, float slope) {
  return f32x4{lrelu_grad(z.x, slope), lrelu_grad(z.y, slope), lrelu_grad(z.z, slope),
               lrelu_grad(z.w, slope)};
}
__device__ __forceinline__ F8 bn_dz8(const F8 g, const F8 v, const F8 sc, const F8 sh,
                                     float slope, const float* mask, int b, int C, int c) {
  const F8 z = v * sc + sh;
  F8 d{g.a * lrelu_grad4(z.a, slope), g.b * lrelu_grad4(z.b, slope)};
  // Dropout2d sits AFTER the LeakyReLU (Unetmodel.py:23-24): d(out)/d(z) =
  // mask * lrelu'(z); multiplication order does not matter for the value.
  if (mask) d = d * ld8(mask + (size_t)b * C + c);
  return d;
}

// BN-backward reduction fused into the kernel that PRODUCES a block output's
// gradient g (the pooling / resize backward): with y = that block's BN input
// Y2, {sum dz, sum dz*xhat} per channel of dz = g * lrelu'(y*scale+shift)
// (no dropout after the second BN, Unetmodel.py:27-28), summed over the
// kernel's block and written as partial row blockIdx.x of [gridDim.x][2][C]
// (the nsm_bn_bwd_reduce format) — the separate reduce pass and its read of g
// are gone. Each thread keeps ONE 8-channel group (C/8 divides 256).
struct BnRedP {
  const void* y;
  const float* scale;
  const float* shift;
  const float* mean;
  const float* invstd;
  float slope;
  float* partial;
  uint32_t* amax;  // max|scale * dz| (may be NULL): the k1 term of the dy bound (finalize)
};
template <typename T>
__device__ __forceinline__ F8 as_stored8(F8 v);
template <>
__device__ __forceinline__ F8 as_stored8<float>(F8 v) { return v; }
template <>
__device__ __forceinline__ F8 as_stored8<f16_t>(F8 v) {
  const u32x4 w = u32x4{pack_hh(v.a.x, v.a.y), pack_hh(v.a.z, v.a.w), pack_hh(v.b.x, v.b.y),
                        pack_hh(v.b.z, v.b.w)};
  return F8{f32x4{h_lo(w.x), h_hi(w.x), h_lo(w.y), h_hi(w.y)},
            f32x4{h_lo(w.z), h_hi(w.z), h_lo(w.w), h_hi(w.w)}};
}
template <>
__device__ __forceinline__ F8 as_stored8<bf16_t>(F8 v) {
  const u32x4 w = u32x4{pack_bf2(v.a.x, v.a.y), pack_bf2(v.a.z, v.a.w), pack_bf2(v.b.x, v.b.y),
                        pack_bf2(v.b.z, v.b.w)};
  return F8{f32x4{bf_lo(w.x), bf_hi(w.x), bf_lo(w.y), bf_hi(w.y)},
            f32x4{bf_lo(w.z), bf_hi(w.z), bf_lo(w.w), bf_hi(w.w)}};
}
struct BnRedAcc {
  F8 sc, sh, mu, is, s1, s2;
  uint32_t am;
  __device__ void init(const BnRedP& r, int c) {
    sc = ldf8(r.scale + c);
    sh = ldf8(r.shift + c);
    mu = ldf8(r.mean + c);
    is = ldf8(r.invstd + c);
    s1 = f8zero();
    s2 = f8zero();
    am = 0;
  }
  // g: the value as written (T-rounded); p: its pixel row in y
  template <typename T>
  __device__ void add(const BnRedP& r, F8 g, size_t p, int C, int c) {
    const F8 v = ld8((const T*)r.y + p * C + c);
    const F8 dz = bn_dz8(g, v, sc, sh, r.slope, nullptr, 0, C, c);
    s1 += dz;
    s2 += dz * ((v - mu) * is);
    if (r.amax) {
      amax_fold(am, sc.a * dz.a);
      amax_fold(am, sc.b * dz.b);
    }
  }
  // whole block (256 threads, group = tid % C8) -> partial row blockIdx.x
  __device__ void write(const BnRedP& r, int C8) {
    __shared__ F8 red[256];
    const int tid = threadIdx.x, rl = 256 / C8, tc = tid % C8, C = C8 * 8;
    red[tid] = s1;
    col_tree_reduce(red, C8, rl, tid);
    const F8 t1 = red[tc];
    __syncthreads();
    red[tid] = s2;
    col_tree_reduce(red, C8, rl, tid);
    if (tid < C8) {
      float* pr = r.partial + (size_t)blockIdx.x * 2 * C;
      st8(pr + tc * 8, t1);
      st8(pr + C + tc * 8, red[tc]);
    }
    amax_flush(am, r.amax);
  }
  // a block covering channels [c0, c0 + 8 G) of a C-channel tensor (group =
  // tid % G): its slice of partial row `row`
  __device__ void write_slice(const BnRedP& r, int G, int c0, int C, int row) {
    __shared__ F8 red[256];
    const int tid = threadIdx.x, rl = 256 / G, tc = tid % G;
    red[tid] = s1;
    col_tree_reduce(red, G, rl, tid);
    const F8 t1 = red[tc];
    __syncthreads();
    red[tid] = s2;
    col_tree_reduce(red, G, rl, tid);
    if (tid < G) {
      float* pr = r.partial + (size_t)row * 2 * C + c0;
      st8(pr + tc * 8, t1);
      st8(pr + C + tc * 8, red[tc]);
    }
    amax_flush(am, r.amax);
  }
};

static inline int grid_for(long long work, int per_block = 256, int cap = 8192) {
  long long g = (work + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

}  // namespace nsm
