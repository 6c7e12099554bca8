// G-buffer feature recipes: the network's input channels composed from the
// rasteriser's raw buffers (paper §3.2: z - z_f, z / z_f, c_c / d, n . n_e beside
// the raw ones), reflect-padded, scrubbed, offset by the emitter size (§3.1.1)
// and normalised in one streaming pass (nsm_amd/features.py, frames.py;
// DESIGN.md "G-buffer feature recipes").
//
//   x [B][Cin][H][W] f32 -> out [B][Cout][Hp][Wp] f32. Output channel c is term
//   (op, a, b) of the recipe over the raw values at the reflected source pixel
//   (ry = y < H ? y : 2 (H - 1) - y, rx likewise: frame_prep's indexing):
//     RAW    x[a]                                   (bits unchanged)
//     SUB    x[a] - x[b]
//     RATIO  |x[b]| <= floor ? +0.0 : x[a] / x[b]   (a NaN x[b] divides: NaN)
//     DOT3   ((x[a] x[b]) + (x[a+1] x[b+1])) + (x[a+2] x[b+2])
//   one IEEE fp32 operation per step, contraction off. Then, in this order: the
//   census (NaN / +Inf / -Inf among the composed values of an image's own H x W
//   pixels), the scrub (frame_scrub), v + emitter[b] on the emitter channel only,
//   and (v - mean[c]) / (stdv[c] + eps), the expression of normalize_frames_kernel.
//
// Work. A unit is 4 consecutive columns of one output row, as in nsm_frame.hip,
// but a thread produces all Cout channels of its unit: the raw planes a unit
// needs are fetched by one thread back to back, so a plane that several terms
// read comes from HBM once and from the cache afterwards, and the pass moves
// about (raw planes used + Cout) planes. Unit u of an image is row u / Q,
// columns 4 (u % Q) .. + 3, Q = ceil(Wp / 4); a block takes FT_UNITS consecutive
// units of one image. The recipe is run-time data in the kernel-argument block
// (one word per term, read with a wave-uniform index): one kernel for every
// recipe, no device table, and a captured graph holds the recipe by value.
// 16-byte loads and stores where the four columns exist and the address is
// 16-byte aligned, decided per access on the real address; 4-byte ones
// otherwise (rows of a width that is no multiple of 4, buffers that start
// inside another tensor, reflected columns, the ragged end of a row).
#include "nsm_frame.h"

#pragma clang fp contract(off)

namespace nsm {

constexpr int FT_MAX_OUT = 16, FT_MAX_IN = 64;
enum { FT_RAW = 0, FT_SUB = 1, FT_RATIO = 2, FT_DOT3 = 3 };

// units of a thread: measured at 1, 2 and 4 ("G-buffer feature recipes")
#ifndef NSM_FEATURE_PER_THREAD
#define NSM_FEATURE_PER_THREAD 1
#endif
constexpr int FT_PER_THREAD = NSM_FEATURE_PER_THREAD;
constexpr int FT_UNITS = FR_THREADS * FT_PER_THREAD;

struct FeatureArgs {
  const float* x;
  float* out;
  const float* mean;
  const float* stdv;
  const float* emitter;
  uint32_t* part;
  int Cin, Cout, H, W, Hp, Wp, per, scrub, echan;
  float eps, floor;
  FastDiv q;                  // units of a row
  uint32_t term[FT_MAX_OUT];  // op | a << 8 | b << 16
};

// the 4 values of plane p at the unit's (reflected) source pixels; a slot past
// the output row holds 0
__device__ __forceinline__ f32x4 feature_load(const float* __restrict__ row, bool wide, int n,
                                              const uint32_t (&cx)[4]) {
  if (wide && ((uintptr_t)(row + cx[0]) & 15u) == 0) return *(const f32x4*)(row + cx[0]);
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < n) v[e] = row[cx[e]];
  return f32x4{v[0], v[1], v[2], v[3]};
}

// grid: B * per blocks
__global__ void __launch_bounds__(FR_THREADS) feature_compose_kernel(FeatureArgs a) {
#pragma clang fp contract(off)
  const uint32_t b = blockIdx.x / (uint32_t)a.per;
  const uint32_t blk = blockIdx.x - b * (uint32_t)a.per;
  const uint32_t units = (uint32_t)a.Hp * a.q.d;
  const uint32_t HW = (uint32_t)a.H * a.W;
  const float* xb = a.x + (size_t)b * a.Cin * HW;
  float* ob = a.out + (size_t)b * a.Cout * a.Hp * a.Wp;
  const float em = a.emitter ? a.emitter[b] : 0.f;
  uint32_t n_nan = 0, n_pinf = 0, n_ninf = 0;
#pragma unroll
  for (int k = 0; k < FT_PER_THREAD; ++k) {
    const uint32_t u = blk * FT_UNITS + k * FR_THREADS + threadIdx.x;
    if (u >= units) break;
    const uint32_t y = fdiv(u, a.q), x0 = 4u * (u - y * a.q.d);
    const bool own = y < (uint32_t)a.H;  // a source row, not a reflected copy
    const uint32_t ry = own ? y : 2u * (a.H - 1) - y;
    const int n = min(4, a.Wp - (int)x0);
    const bool wide = x0 + 4 <= (uint32_t)a.W;  // four source columns, none reflected
    uint32_t cx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t xx = x0 + e;
      cx[e] = e < n ? (xx < (uint32_t)a.W ? xx : 2u * (a.W - 1) - xx) : 0u;
    }
    const float* src = xb + ry * (uint32_t)a.W;
    for (int c = 0; c < a.Cout; ++c) {
      const uint32_t term = a.term[c];
      const uint32_t op = term & 0xffu, pa = (term >> 8) & 0xffu, pb = (term >> 16) & 0xffu;
      f32x4 v = feature_load(src + pa * HW, wide, n, cx);
      if (op == FT_SUB) {
        v = v - feature_load(src + pb * HW, wide, n, cx);
      } else if (op == FT_RATIO) {
        const f32x4 d = feature_load(src + pb * HW, wide, n, cx);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fabsf(d[e]) <= a.floor ? 0.f : v[e] / d[e];
      } else if (op == FT_DOT3) {
        const f32x4 p0 = v * feature_load(src + pb * HW, wide, n, cx);
        const f32x4 p1 = feature_load(src + (pa + 1) * HW, wide, n, cx) *
                         feature_load(src + (pb + 1) * HW, wide, n, cx);
        const f32x4 p2 = feature_load(src + (pa + 2) * HW, wide, n, cx) *
                         feature_load(src + (pb + 2) * HW, wide, n, cx);
        v = (p0 + p1) + p2;
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
      if (c == a.echan) v = v + em;
      if (a.mean) {
        const float m = a.mean[c], d = a.stdv[c] + a.eps;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (v[e] - m) / d;
      }
      float* dst = ob + ((size_t)c * a.Hp + y) * a.Wp + x0;
      if (n == 4 && ((uintptr_t)dst & 15u) == 0) {
        *(f32x4*)dst = v;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < n) dst[e] = v[e];
      }
    }
  }
  if (a.part) frame_block_counts(n_nan, n_pinf, n_ninf, a.part + (size_t)blockIdx.x * 3);
}

}  // namespace nsm

using namespace nsm;

extern "C" int nsm_feature_blocks(int Cout, int Hp, int Wp) {
  if (Cout <= 0 || Cout > FT_MAX_OUT || Hp <= 0 || Wp <= 0) return 0;
  if ((long long)Cout * Hp * Wp >= (1ll << 31)) return 0;
  return ceil_div((long long)Hp * ((Wp + 3) / 4), FT_UNITS);
}

extern "C" int nsm_feature_compose(const float* x, int B, int Cin, int H, int W, int Hp, int Wp,
                                   const int32_t* recipe, int Cout, float ratio_floor,
                                   const float* mean, const float* stdv, float eps, int scrub,
                                   int emitter_channel, const float* emitter, float* out,
                                   uint32_t* partial, int32_t* report, void* stream) {
  NSM_CHECK_ARG(x && out && recipe, "feature_compose: null pointer");
  NSM_CHECK_ARG((mean == nullptr) == (stdv == nullptr),
                "feature_compose: mean and stdv go together (both or neither), got a null pointer");
  NSM_CHECK_ARG((partial == nullptr) == (report == nullptr),
                "feature_compose: the census needs partial and report (both or neither), got a "
                "null pointer");
  NSM_CHECK_ARG(B > 0 && Cin > 0 && H > 0 && W > 0, "feature_compose: shape %d x %d x %d x %d", B,
                Cin, H, W);
  NSM_CHECK_ARG(Cin <= FT_MAX_IN, "feature_compose: %d raw channels (at most %d)", Cin, FT_MAX_IN);
  NSM_CHECK_ARG(Cout >= 1 && Cout <= FT_MAX_OUT, "feature_compose: %d output channels (1 to %d)",
                Cout, FT_MAX_OUT);
  NSM_CHECK_ARG(ratio_floor >= 0.f, "feature_compose: ratio_floor %g (at least 0)",
                (double)ratio_floor);
  NSM_CHECK_ARG(Hp >= H && Wp >= W,
                "feature_compose: padded size %d x %d is smaller than %d x %d", Hp, Wp, H, W);
  NSM_CHECK_ARG(Hp - H < H,
                "feature_compose: reflect pad of %d rows needs a height above it, got %d", Hp - H, H);
  NSM_CHECK_ARG(Wp - W < W,
                "feature_compose: reflect pad of %d columns needs a width above it, got %d", Wp - W,
                W);
  NSM_CHECK_ARG(emitter_channel >= -1 && emitter_channel < Cout,
                "feature_compose: emitter_channel %d outside [-1, %d)", emitter_channel, Cout);
  NSM_CHECK_ARG((emitter_channel >= 0) == (emitter != nullptr),
                "feature_compose: emitter_channel and emitter go together (both or neither)");
  FeatureArgs a;
  for (int c = 0; c < Cout; ++c) {
    const int op = recipe[3 * c], i = recipe[3 * c + 1], j = recipe[3 * c + 2];
    NSM_CHECK_ARG(op >= FT_RAW && op <= FT_DOT3,
                  "feature_compose: bad table: term %d has op %d (0 raw, 1 sub, 2 ratio, 3 dot3)", c,
                  op);
    const int span = op == FT_DOT3 ? 3 : 1;
    NSM_CHECK_ARG(i >= 0 && i + span <= Cin,
                  "feature_compose: bad table: term %d (op %d) reads channel %d of %d", c, op, i,
                  Cin);
    NSM_CHECK_ARG(op == FT_RAW || (j >= 0 && j + span <= Cin),
                  "feature_compose: bad table: term %d (op %d) reads channel %d of %d", c, op, j,
                  Cin);
    a.term[c] = (uint32_t)op | (uint32_t)i << 8 | (uint32_t)(op == FT_RAW ? 0 : j) << 16;
  }
  for (int c = Cout; c < FT_MAX_OUT; ++c) a.term[c] = 0;
  const int per = nsm_feature_blocks(Cout, Hp, Wp);
  NSM_CHECK_ARG(per > 0 && (long long)Cin * H * W < (1ll << 31) &&
                    (long long)B * per < (1ll << 31),
                "feature_compose: %d images of %d x %d x %d raw and %d x %d x %d composed samples "
                "(an image holds fewer than 2^31 of each)", B, Cin, H, W, Cout, Hp, Wp);
  NSM_CHECK_ARG((((uintptr_t)x | (uintptr_t)out | (uintptr_t)emitter) & 3u) == 0,
                "feature_compose: unaligned pointer");
  a.x = x, a.out = out, a.mean = mean, a.stdv = stdv, a.emitter = emitter, a.part = partial;
  a.Cin = Cin, a.Cout = Cout, a.H = H, a.W = W, a.Hp = Hp, a.Wp = Wp, a.per = per;
  a.scrub = scrub, a.echan = emitter_channel, a.eps = eps, a.floor = ratio_floor;
  a.q = make_fastdiv((uint32_t)((Wp + 3) / 4));
  hipLaunchKernelGGL(feature_compose_kernel, dim3((unsigned)(B * per)), dim3(FR_THREADS), 0,
                     as_stream(stream), a);
  if (partial) frame_census(partial, B, per, 0, report, as_stream(stream));
  NSM_LAUNCH_CHECK("feature_compose");
  return 0;
}
