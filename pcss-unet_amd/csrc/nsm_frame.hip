// The inference frame path around the eval forward (the reference's
// inference.py process_image / save_output): raw frame -> network input, and
// network output -> the 8-bit image and the clipped fp32 frame. Two streaming
// passes, each one read of its source and one write of each output.
//
// Both kernels work in units of 4 consecutive columns of one row: unit u of an
// image is row u / Q, columns 4 * (u % Q) .. + 3, Q = ceil(width / 4) (two
// divisions by launch constants, nsm::FastDiv). A block takes FR_UNITS
// consecutive units of one image, thread t the units t, t + 256, ... of them, so
// a wave's 16-byte accesses are 1 KiB contiguous. Nothing is assumed of a row's
// address beyond 4-byte alignment: a unit goes through one 16-byte load (store)
// when its four columns exist and its address is 16-byte aligned, and through
// up to four 4-byte ones otherwise. That decision is taken per unit on the real
// address, so rows of a frame whose width is no multiple of 4 (every other or
// three of four rows start unaligned), buffers that start inside another
// tensor, the reflected columns and the last unit of a ragged row all take the
// narrow path and nothing else does.
//
//   frame_prep: out[b,c,y,x] = f(x[b,c,ry,rx]), ry = y < H ? y : 2 (H - 1) - y
//     and rx likewise (nn.ReflectionPad2d((0, Wp - W, 0, Hp - H)),
//     inference.py:153-163); f scrubs (NaN -> 0, +Inf -> 1, -Inf -> 0,
//     inference.py:170-173) and then normalises (setdata.py:316, the expression
//     of normalize_frames_kernel in nsm_elem.hip). A unit wholly left of column
//     W reads its source with one 16-byte load when that address allows; a
//     unit that holds a reflected column reads its columns one by one.
//   frame_finish: v' = clip(scrub(v), 0, 1) (inference.py:199-202, :109) of the
//     top-left H x W of o [B][C][Hp][Wp]; a thread holds the C channels of its 4
//     pixels, so the channels-last bytes of a unit, (uint8_t)(v' * 255.0f)
//     (inference.py:115-125), are 4 * C contiguous bytes: C 32-bit stores when
//     the address is 4-byte aligned, single bytes otherwise.
//   Census: a thread counts its own samples (prep: the source samples only, a
//     padded copy is not one), the wave adds by shuffles, the block's 4 waves
//     through LDS, and the block writes 3 counts to part[(b * per + blk) * 3].
//     frame_census then adds an image's `per` triples, thread t the triples t,
//     t + 256, ..., and the threads by the same tree: whole numbers in a fixed
//     order, no atomics, and no second pass over the frame.
#include <math.h>
#include "nsm_frame.h"

namespace nsm {

// 2 units per thread: measured against 1 and 4 at 1080p ("Inference frame path")
constexpr int FR_PER_THREAD = 2;
constexpr int FR_UNITS = FR_THREADS * FR_PER_THREAD;  // units of one block: 2048 samples

struct PrepArgs {
  const float* x;
  float* out;
  const float* mean;
  const float* stdv;
  uint32_t* part;
  int C, H, W, Hp, Wp, per, scrub;
  float eps;
  FastDiv q, hp;  // units of a row, rows of a plane
};

// grid: B * per blocks
__global__ void __launch_bounds__(FR_THREADS) frame_prep_kernel(PrepArgs a) {
  const uint32_t b = blockIdx.x / (uint32_t)a.per;
  const uint32_t blk = blockIdx.x - b * (uint32_t)a.per;
  const uint32_t units = (uint32_t)a.C * a.Hp * a.q.d;
  const float* xb = a.x + (size_t)b * a.C * a.H * a.W;
  float* ob = a.out + (size_t)b * a.C * a.Hp * a.Wp;
  uint32_t n_nan = 0, n_pinf = 0, n_ninf = 0;
#pragma unroll
  for (int k = 0; k < FR_PER_THREAD; ++k) {
    const uint32_t u = blk * FR_UNITS + k * FR_THREADS + threadIdx.x;
    if (u >= units) break;
    const uint32_t row = fdiv(u, a.q), x0 = 4u * (u - row * a.q.d);
    const uint32_t c = fdiv(row, a.hp), y = row - c * a.hp.d;
    const bool own = y < (uint32_t)a.H;  // a source row, not a reflected copy
    const uint32_t ry = own ? y : 2u * (a.H - 1) - y;
    const float* src = xb + ((size_t)c * a.H + ry) * a.W;
    float* dst = ob + (size_t)row * a.Wp + x0;
    const int n = min(4, a.Wp - (int)x0);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (x0 + 4 <= (uint32_t)a.W && ((uintptr_t)(src + x0) & 15u) == 0) {
      const f32x4 q = *(const f32x4*)(src + x0);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t xx = x0 + e;
        if (e < n) v[e] = src[xx < (uint32_t)a.W ? xx : 2u * (a.W - 1) - xx];
      }
    }
    if (a.part && own) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t bits = __float_as_uint(v[e]);
        const bool in = x0 + e < (uint32_t)a.W;
        n_nan += in && (bits & 0x7fffffffu) > 0x7f800000u;
        n_pinf += in && bits == 0x7f800000u;
        n_ninf += in && bits == 0xff800000u;
      }
    }
    if (a.scrub) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = frame_scrub(v[e]);
    }
    if (a.mean) {
      const float m = a.mean[c], d = a.stdv[c] + a.eps;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (v[e] - m) / d;
    }
    if (n == 4 && ((uintptr_t)dst & 15u) == 0) {
      *(f32x4*)dst = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < n) dst[e] = v[e];
    }
  }
  if (a.part) frame_block_counts(n_nan, n_pinf, n_ninf, a.part + (size_t)blockIdx.x * 3);
}

struct FinishArgs {
  const float* o;
  uint8_t* u8;
  float* f32;
  uint32_t* part;
  int Hp, Wp, H, W, per;
  FastDiv q;  // units of a cropped row
};

// grid: B * per blocks
template <int C>
__global__ void __launch_bounds__(FR_THREADS) frame_finish_kernel(FinishArgs a) {
  const uint32_t b = blockIdx.x / (uint32_t)a.per;
  const uint32_t blk = blockIdx.x - b * (uint32_t)a.per;
  const uint32_t units = (uint32_t)a.H * a.q.d;
  const float* ob = a.o + (size_t)b * C * a.Hp * a.Wp;
  uint32_t n_bad = 0, n_neg = 0, n_big = 0;
#pragma unroll
  for (int k = 0; k < FR_PER_THREAD; ++k) {
    const uint32_t u = blk * FR_UNITS + k * FR_THREADS + threadIdx.x;
    if (u >= units) break;
    const uint32_t y = fdiv(u, a.q), x0 = 4u * (u - y * a.q.d);
    const int n = min(4, a.W - (int)x0);
    uint8_t px[4 * C];  // the unit's bytes in output order: pixel e, channel c at e * C + c
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float* src = ob + ((size_t)c * a.Hp + y) * a.Wp + x0;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (n == 4 && ((uintptr_t)src & 15u) == 0) {
        const f32x4 q = *(const f32x4*)src;
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < n) v[e] = src[e];
      }
      if (a.part) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // a slot past the row holds 0: counted nowhere
          n_bad += (__float_as_uint(v[e]) & 0x7fffffffu) >= 0x7f800000u;
          n_neg += v[e] < 0.f;
          n_big += v[e] > 1.f;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float s = frame_scrub(v[e]);
        v[e] = s < 0.f ? 0.f : (s > 1.f ? 1.f : s);
        px[e * C + c] = (uint8_t)(v[e] * 255.0f);
      }
      if (a.f32) {
        float* dst = a.f32 + (((size_t)b * C + c) * a.H + y) * a.W + x0;
        if (n == 4 && ((uintptr_t)dst & 15u) == 0) {
          *(f32x4*)dst = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (e < n) dst[e] = v[e];
        }
      }
    }
    if (a.u8) {
      uint8_t* dst = a.u8 + (((size_t)b * a.H + y) * a.W + x0) * C;
      if (n == 4 && ((uintptr_t)dst & 3u) == 0) {
#pragma unroll
        for (int w = 0; w < C; ++w)
          ((uint32_t*)dst)[w] = (uint32_t)px[4 * w] | (uint32_t)px[4 * w + 1] << 8 |
                                (uint32_t)px[4 * w + 2] << 16 | (uint32_t)px[4 * w + 3] << 24;
      } else {
#pragma unroll
        for (int i = 0; i < 4 * C; ++i)
          if (i < n * C) dst[i] = px[i];
      }
    }
  }
  if (a.part) frame_block_counts(n_bad, n_neg, n_big, a.part + (size_t)blockIdx.x * 3);
}

}  // namespace nsm

using namespace nsm;

extern "C" int nsm_frame_blocks(int C, int H, int W) {
  if (C <= 0 || H <= 0 || W <= 0) return 0;
  const long long units = (long long)C * H * ((W + 3) / 4);
  if ((long long)C * H * W >= (1ll << 31)) return 0;
  return ceil_div(units, FR_UNITS);
}

extern "C" int nsm_frame_prep(const float* x, int B, int C, int H, int W, int Hp, int Wp,
                              const float* mean, const float* stdv, float eps, int scrub,
                              float* out, uint32_t* partial, int32_t* report, void* stream) {
  NSM_CHECK_ARG(x && out, "frame_prep: null pointer");
  NSM_CHECK_ARG((mean == nullptr) == (stdv == nullptr),
                "frame_prep: mean and stdv go together (both or neither), got a null pointer");
  NSM_CHECK_ARG((partial == nullptr) == (report == nullptr),
                "frame_prep: the census needs partial and report (both or neither), got a null "
                "pointer");
  NSM_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "frame_prep: shape %d x %d x %d x %d", B, C, H, W);
  NSM_CHECK_ARG(Hp >= H && Wp >= W, "frame_prep: padded size %d x %d is smaller than %d x %d", Hp,
                Wp, H, W);
  NSM_CHECK_ARG(Hp - H < H, "frame_prep: reflect pad of %d rows needs a height above it, got %d",
                Hp - H, H);
  NSM_CHECK_ARG(Wp - W < W, "frame_prep: reflect pad of %d columns needs a width above it, got %d",
                Wp - W, W);
  const int per = nsm_frame_blocks(C, Hp, Wp);
  NSM_CHECK_ARG(per > 0 && (long long)B * per < (1ll << 31),
                "frame_prep: %d images of %d x %d x %d samples (an image holds fewer than 2^31)", B,
                C, Hp, Wp);
  NSM_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 3u) == 0, "frame_prep: unaligned pointer");
  PrepArgs a{x, out, mean, stdv, partial, C, H, W, Hp, Wp, per, scrub, eps,
             make_fastdiv((uint32_t)((Wp + 3) / 4)), make_fastdiv((uint32_t)Hp)};
  hipLaunchKernelGGL(frame_prep_kernel, dim3((unsigned)(B * per)), dim3(FR_THREADS), 0,
                     as_stream(stream), a);
  if (partial) frame_census(partial, B, per, 0, report, as_stream(stream));
  NSM_LAUNCH_CHECK("frame_prep");
  return 0;
}

extern "C" int nsm_frame_finish(const float* o, int B, int C, int Hp, int Wp, int H, int W,
                                uint8_t* u8, float* f32, uint32_t* partial, int32_t* report,
                                void* stream) {
  NSM_CHECK_ARG(o, "frame_finish: null pointer");
  NSM_CHECK_ARG(u8 || f32, "frame_finish: no output (u8 and f32 are both null pointers)");
  NSM_CHECK_ARG((partial == nullptr) == (report == nullptr),
                "frame_finish: the census needs partial and report (both or neither), got a null "
                "pointer");
  NSM_CHECK_ARG(C == 1 || C == 3 || C == 4, "frame_finish: %d channels (1, 3 or 4)", C);
  NSM_CHECK_ARG(B > 0 && H > 0 && W > 0, "frame_finish: shape %d x %d x %d x %d", B, C, H, W);
  NSM_CHECK_ARG(H <= Hp && W <= Wp, "frame_finish: crop %d x %d is larger than the source %d x %d",
                H, W, Hp, Wp);
  const int per = nsm_frame_blocks(1, H, W);
  NSM_CHECK_ARG(nsm_frame_blocks(C, Hp, Wp) > 0 && per > 0 && (long long)B * per < (1ll << 31),
                "frame_finish: %d images of %d x %d x %d samples (an image holds fewer than 2^31)",
                B, C, Hp, Wp);
  NSM_CHECK_ARG((((uintptr_t)o | (uintptr_t)f32) & 3u) == 0, "frame_finish: unaligned pointer");
  FinishArgs a{o, u8, f32, partial, Hp, Wp, H, W, per, make_fastdiv((uint32_t)((W + 3) / 4))};
  const dim3 grid((unsigned)(B * per)), block(FR_THREADS);
  hipStream_t st = as_stream(stream);
  if (C == 1)
    hipLaunchKernelGGL(frame_finish_kernel<1>, grid, block, 0, st, a);
  else if (C == 3)
    hipLaunchKernelGGL(frame_finish_kernel<3>, grid, block, 0, st, a);
  else
    hipLaunchKernelGGL(frame_finish_kernel<4>, grid, block, 0, st, a);
  if (partial) frame_census(partial, B, per, 3, report, st);
  NSM_LAUNCH_CHECK("frame_finish");
  return 0;
}
