// The training-patch sampler: one launch gathers a batch of random crops out of
// a device-resident frame pool, straight into the static x / y buffers of the
// training step (nsm_amd/patches.py, DESIGN.md "Training-patch sampler").
//
//   inputs [N][C][H][W] f32, labels [N][E][H][W] f32 (one target plane per
//   emitter size) -> x [B][C][ph][pw] f32 normalised, y [B][1][ph][pw] f32,
//   draws [B][8] int32 (frame, oy, ox, hflip, vflip, emitter, 0, 0).
//
// Draws. Sample i of step t is n = t * B + i (uint64); field f of it is
//   r_f = mix64((seed ^ mix64(rank)) ^ mix64(8 n + f)),  draw(m) = umul64hi(r_f, m)
// (an integer in [0, m), 0 when m == 1): f = 0 the frame (sequential: lo + n mod
// count; random: lo + draw(count)), f = 1 oy = align * draw((H - ph) / align + 1),
// f = 2 ox likewise, f = 3 the flips (top bit h, next bit v; a disabled flip is
// 0), f = 4 the emitter index draw(E). A block belongs to one sample and works
// its draw out once, from block-uniform values, before its loop; nothing here is
// clamped, the ranges hold by construction.
//
// Values. x = ((s * v + o) - mean[c]) / (std[c] + eps): the expression and the
// bits of normalize_frames_kernel (nsm_elem.hip) behind s * v + o, contraction
// off. s = hsign[c] (if h-flipped) * vsign[c] (if v-flipped), 1 otherwise; o =
// emitter_values[e] is added on the emitter channel only, so every other
// channel keeps a -0.0. The label is plane e of the frame, copied bit for bit.
//
// Work. A sample's output is two flat runs, C * ph * pw elements of x and
// ph * pw of y, cut into tiles of PT_TILE = 1024 consecutive elements; block
// blk of a sample takes the tiles blk, blk + per, ... (the trip count is the
// same for every thread of a block). Thread t loads the elements k * 256 + t
// (k = 0..3) of its tile: consecutive lanes on consecutive destination
// elements, that is on consecutive source pixels of a row, left to right or,
// in a mirrored row, right to left; a source row starts at an arbitrary ox, so
// these are dword loads. The vector kernel (pw % 4 == 0, 16-byte aligned
// outputs) passes the four values through LDS and stores the elements
// 4 t .. 4 t + 3 with one 16-byte store; two LDS buffers alternate, so one
// barrier per tile is enough. The scalar kernel stores what it loaded.
// The frame base is formed in 64 bits (a pool holds more than 2^31 elements);
// inside a frame and inside a sample offsets are 32 bits (C * H * W < 2^31 is
// checked). Per-channel constants sit in LDS (C <= PT_MAX_C).
#include "nsm_common.h"

namespace nsm {

constexpr int PT_THREADS = 256, PT_PER_THREAD = 4;
constexpr int PT_TILE = PT_THREADS * PT_PER_THREAD;
constexpr int PT_MAX_C = 256;
constexpr int PT_GRID = 2048;  // blocks aimed at: 8 per CU

struct PatchArgs {
  const float* in;
  const float* lab;
  float* x;
  float* y;
  int32_t* draws;
  const float* mean;
  const float* stdv;
  const float* hsign;
  const float* vsign;
  const float* evals;
  const int64_t* seed_dev;
  const int64_t* step_dev;
  uint64_t seed, step, rank, lo, count;
  uint32_t ny, nx;  // offsets drawn per axis
  int B, C, E, H, W, ph, pw, order, align, hflip, vflip, echan, per;
  uint32_t tiles_x, tiles_y;
  float eps;
  FastDiv dpw, dph;
};

template <bool VEC>
__global__ void __launch_bounds__(PT_THREADS) patch_gather_kernel(PatchArgs a) {
#pragma clang fp contract(off)
  __shared__ float c_mean[PT_MAX_C], c_div[PT_MAX_C], c_sign[PT_MAX_C];
  __shared__ float stage[VEC ? 2 * PT_TILE : 1];
  const uint32_t i = blockIdx.x / (uint32_t)a.per;  // the sample
  const uint32_t blk = blockIdx.x - i * (uint32_t)a.per;
  const int t = threadIdx.x;

  // the sample's draw: block-uniform
  const uint64_t seed = a.seed_dev ? (uint64_t)a.seed_dev[0] : a.seed;
  const uint64_t step = a.step_dev ? (uint64_t)a.step_dev[0] : a.step;
  const uint64_t key = seed ^ mix64(a.rank);
  const uint64_t n = step * (uint64_t)a.B + i;
  const uint64_t frame = a.lo + (a.order == 0 ? n % a.count
                                              : __umul64hi(mix64(key ^ mix64(8 * n + 0)), a.count));
  const uint32_t oy = (uint32_t)a.align * (uint32_t)__umul64hi(mix64(key ^ mix64(8 * n + 1)), a.ny);
  const uint32_t ox = (uint32_t)a.align * (uint32_t)__umul64hi(mix64(key ^ mix64(8 * n + 2)), a.nx);
  const uint64_t rf = mix64(key ^ mix64(8 * n + 3));
  const bool hf = a.hflip && (rf >> 63), vf = a.vflip && ((rf >> 62) & 1);
  const uint32_t e = (uint32_t)__umul64hi(mix64(key ^ mix64(8 * n + 4)), (uint64_t)a.E);
  if (a.draws && blk == 0 && t < 8) {
    const int32_t rec[8] = {(int32_t)frame, (int32_t)oy, (int32_t)ox, (int32_t)hf,
                            (int32_t)vf,    (int32_t)e,  0,           0};
    int32_t v = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) v = t == k ? rec[k] : v;
    a.draws[(size_t)i * 8 + t] = v;
  }
  for (int c = t; c < a.C; c += PT_THREADS) {
    c_mean[c] = a.mean[c];
    c_div[c] = a.stdv[c] + a.eps;
    c_sign[c] = (hf && a.hsign ? a.hsign[c] : 1.f) * (vf && a.vsign ? a.vsign[c] : 1.f);
  }
  __syncthreads();

  const uint32_t HW = (uint32_t)a.H * a.W;
  const uint32_t n_x = (uint32_t)a.C * a.ph * a.pw, n_y = (uint32_t)a.ph * a.pw;
  const float* fin = a.in + frame * ((uint64_t)a.C * HW);
  const float* flab = a.lab + (frame * (uint64_t)a.E + e) * HW;
  float* xo = a.x + (size_t)i * n_x;
  float* yo = a.y + (size_t)i * n_y;
  const float o = a.echan >= 0 ? a.evals[e] : 0.f;
  const uint32_t tiles = a.tiles_x + a.tiles_y;
  int buf = 0;
  for (uint32_t T = blk; T < tiles; T += (uint32_t)a.per, buf ^= 1) {
    const bool is_y = T >= a.tiles_x;  // block-uniform
    const uint32_t base = (is_y ? T - a.tiles_x : T) * PT_TILE;
    const uint32_t total = is_y ? n_y : n_x;
    const float* src = is_y ? flab : fin;
    float* dst = is_y ? yo : xo;
    float v[PT_PER_THREAD];
    uint32_t ch[PT_PER_THREAD];
#pragma unroll
    for (int k = 0; k < PT_PER_THREAD; ++k) {
      const uint32_t f = base + k * PT_THREADS + t;
      v[k] = 0.f, ch[k] = 0;
      if (f < total) {
        const uint32_t row = fdiv(f, a.dpw), col = f - row * a.pw;
        const uint32_t c = fdiv(row, a.dph), r = row - c * a.ph;
        const uint32_t sy = oy + (vf ? a.ph - 1 - r : r), sx = ox + (hf ? a.pw - 1 - col : col);
        v[k] = src[c * HW + sy * a.W + sx];
        ch[k] = c;
      }
    }
    if (!is_y) {
#pragma unroll
      for (int k = 0; k < PT_PER_THREAD; ++k) {
        const uint32_t c = ch[k];
        float s = c_sign[c] * v[k];
        if ((int)c == a.echan) s = s + o;
        v[k] = (s - c_mean[c]) / c_div[c];
      }
    }
    if (VEC) {
      float* sb = stage + buf * PT_TILE;
#pragma unroll
      for (int k = 0; k < PT_PER_THREAD; ++k) sb[k * PT_THREADS + t] = v[k];
      __syncthreads();
      const uint32_t f = base + 4 * t;  // total % 4 == 0: all four or none
      if (f < total) *(f32x4*)(dst + f) = *(const f32x4*)(sb + 4 * t);
    } else {
#pragma unroll
      for (int k = 0; k < PT_PER_THREAD; ++k) {
        const uint32_t f = base + k * PT_THREADS + t;
        if (f < total) dst[f] = v[k];
      }
    }
  }
}

__global__ void patch_advance_kernel(int64_t* step) { step[0] += 1; }

}  // namespace nsm

using namespace nsm;

extern "C" int nsm_patch_gather(const float* inputs, const float* labels, int64_t N, int C, int E,
                                int H, int W, int B, int ph, int pw, const float* mean,
                                const float* stdv, float eps, const float* hsign,
                                const float* vsign, int emitter_channel,
                                const float* emitter_values, int order, int align, int hflip,
                                int vflip, int64_t lo, int64_t count, int rank, uint64_t seed,
                                const int64_t* seed_dev, int64_t step, const int64_t* step_dev,
                                float* x_out, float* y_out, int32_t* draws_out, void* stream) {
  NSM_CHECK_ARG(inputs && labels && mean && stdv && x_out && y_out, "patch_gather: null pointer");
  NSM_CHECK_ARG(N > 0 && N < (1ll << 31) && C > 0 && E > 0 && H > 0 && W > 0 && B > 0,
                "patch_gather: pool %lld x %d (%d label planes) x %d x %d, batch %d", (long long)N,
                C, E, H, W, B);
  NSM_CHECK_ARG(C <= PT_MAX_C, "patch_gather: %d channels (at most %d)", C, PT_MAX_C);
  NSM_CHECK_ARG(ph >= 1 && pw >= 1 && ph <= H && pw <= W,
                "patch_gather: patch %d x %d does not fit the %d x %d frame", ph, pw, H, W);
  NSM_CHECK_ARG((long long)C * H * W < (1ll << 31) && (long long)E * H * W < (1ll << 31),
                "patch_gather: a frame of %d x %d x %d samples or its %d label planes do not fit "
                "32-bit offsets (fewer than 2^31 each)", C, H, W, E);
  NSM_CHECK_ARG(align >= 1, "patch_gather: align %d (at least 1)", align);
  NSM_CHECK_ARG(order == 0 || order == 1, "patch_gather: order %d (0 sequential, 1 random)", order);
  NSM_CHECK_ARG(emitter_channel >= -1 && emitter_channel < C,
                "patch_gather: emitter_channel %d outside [-1, %d)", emitter_channel, C);
  NSM_CHECK_ARG((emitter_channel >= 0) == (emitter_values != nullptr),
                "patch_gather: emitter_channel and emitter_values go together (both or neither)");
  NSM_CHECK_ARG(count >= 1 && lo >= 0 && lo + count <= N,
                "patch_gather: shard [%lld, %lld + %lld) of %lld frames", (long long)lo,
                (long long)lo, (long long)count, (long long)N);
  NSM_CHECK_ARG(rank >= 0 && (step_dev || step >= 0), "patch_gather: rank %d, step %lld", rank,
                (long long)step);
  NSM_CHECK_ARG((((uintptr_t)inputs | (uintptr_t)labels | (uintptr_t)x_out | (uintptr_t)y_out |
                  (uintptr_t)draws_out) & 3u) == 0 &&
                    (((uintptr_t)seed_dev | (uintptr_t)step_dev) & 7u) == 0,
                "patch_gather: unaligned pointer");
  PatchArgs a;
  a.in = inputs, a.lab = labels, a.x = x_out, a.y = y_out, a.draws = draws_out;
  a.mean = mean, a.stdv = stdv, a.hsign = hsign, a.vsign = vsign, a.evals = emitter_values;
  a.seed_dev = seed_dev, a.step_dev = step_dev;
  a.seed = seed, a.step = (uint64_t)step, a.rank = (uint64_t)rank;
  a.lo = (uint64_t)lo, a.count = (uint64_t)count;
  a.ny = (uint32_t)((H - ph) / align + 1), a.nx = (uint32_t)((W - pw) / align + 1);
  a.B = B, a.C = C, a.E = E, a.H = H, a.W = W, a.ph = ph, a.pw = pw, a.order = order;
  a.align = align, a.hflip = hflip != 0, a.vflip = vflip != 0, a.echan = emitter_channel;
  a.tiles_x = (uint32_t)ceil_div((long long)C * ph * pw, PT_TILE);
  a.tiles_y = (uint32_t)ceil_div((long long)ph * pw, PT_TILE);
  const int tiles = (int)(a.tiles_x + a.tiles_y);
  a.per = tiles < ceil_div(PT_GRID, B) ? tiles : ceil_div(PT_GRID, B);
  a.eps = eps;
  a.dpw = make_fastdiv((uint32_t)pw), a.dph = make_fastdiv((uint32_t)ph);
  NSM_CHECK_ARG((long long)B * a.per < (1ll << 31), "patch_gather: batch %d", B);
  const dim3 grid((unsigned)(B * a.per)), block(PT_THREADS);
  const bool vec = pw % 4 == 0 && (((uintptr_t)x_out | (uintptr_t)y_out) & 15u) == 0;
  if (vec)
    hipLaunchKernelGGL(patch_gather_kernel<true>, grid, block, 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(patch_gather_kernel<false>, grid, block, 0, as_stream(stream), a);
  NSM_LAUNCH_CHECK("patch_gather");
  return 0;
}

extern "C" int nsm_patch_advance(int64_t* step_dev, void* stream) {
  NSM_CHECK_ARG(step_dev && ((uintptr_t)step_dev & 7u) == 0, "patch_advance: null or unaligned pointer");
  hipLaunchKernelGGL(patch_advance_kernel, dim3(1), dim3(1), 0, as_stream(stream), step_dev);
  NSM_LAUNCH_CHECK("patch_advance");
  return 0;
}
