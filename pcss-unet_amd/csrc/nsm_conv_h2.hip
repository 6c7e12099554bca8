// The f16 LDS-DMA GEMMs on pre-split f16x2 ("h2") and single-plane f16 operands:
// the gemm_h2 / h2q / h2p kernels (nsm_conv_h2.inc), the 1x1 and direct 3x3
// convolutions on them (nsm_conv_h2d.inc), and below the C entries and plans
// of the Winograd GEMMs on h2 operands. Also owns the single-plane f16 GEMMs
// the bf16 path's Winograd calls (wino_gemm_f16, wino_wgrad_gemm_f16). The
// transforms that write the operands are Winograd kernels (nsm_conv.hip).
#include "nsm_conv.h"
#include "nsm_elem.h"  // bn_act_h2_8: the fused BN-act 1x1 forward (nsm_conv_h2d.inc)

// the bf16 LDS-DMA loaders, which the direct 3x3 convolution on h2 operands
// reuses (nsm_conv_h2d.inc: an h2 tensor read as 16-bit columns)
namespace nsm_bf {
using namespace nsm;
#include "nsm_conv_s16_loaders.inc"
}  // namespace nsm_bf

using namespace nsm;
using namespace nsm_bf;

#include "nsm_conv_h2.inc"
#include "nsm_conv_h2d.inc"

// NSM_H2_WG256=0: the h2 weight gradients keep 128x128 tiles where 256x256 fit
static bool h2_wg256() { static const bool v = env_flag("NSM_H2_WG256", true); return v; }

// the h2 weight-gradient plan: plan_wino_wgrad's, or 256x256 tiles (8 waves,
// the forward's tile) where both channel counts are multiples of 256, with the
// split count that brings the grid to ~1024 blocks (4 rounds of one block per CU)
// splits of a batched weight-gradient GEMM over T tiles for ~target blocks
static void wino_wgrad_resplit(WinoWgradPlan& p, long long T, int cin_p, int cout_p, int nb,
                               long long target) {
  const long long tiles = (long long)ceil_div(cout_p, p.BM) * ceil_div(cin_p, p.BN) * nb;
  long long sp = (target + tiles - 1) / tiles, maxs = (T + 255) / 256;
  if (sp > maxs) sp = maxs;
  if (sp > 64) sp = 64;
  if (sp < 1) sp = 1;
  long long kc = (T + sp - 1) / sp;
  kc = (kc + BK - 1) / BK * BK;
  sp = (T + kc - 1) / kc;
  p.splits = (int)sp;
  p.kchunk = (int)kc;
  p.slab_floats = (size_t)nb * sp * cout_p * cin_p;
  if (sp > 1) p.slab_floats += (size_t)nb * cout_p * cin_p;
}

static WinoWgradPlan plan_wino_wgrad_h2(long long T, int cin_p, int cout_p, int nb) {
  WinoWgradPlan p = plan_wino_wgrad(T, cin_p, cout_p, nb);
  // the 128 / 64 tiles run two blocks per CU: one round of ~512 blocks
  // (plan_wino_wgrad's ~4096 wrote 64 x 57 partial dU slabs at conv8; A/B
  // 4096 / 1024 / 512: 658-659 / 661-663 / 664 frames/s)
  static const long long target = env_int("NSM_H2_WG_BLOCKS", 512);
  wino_wgrad_resplit(p, T, cin_p, cout_p, nb, target);
  if (!h2_wg256() || cin_p % 256 || cout_p % 256) return p;
  p.BM = p.BN = 256;
  const long long tiles = (long long)(cout_p / 256) * (cin_p / 256) * nb;
  static const long long target256 = env_int("NSM_H2_WG256_BLOCKS", 1024);
  long long sp = (target256 + tiles - 1) / tiles, maxs = (T + 255) / 256;
  // a full round of unsplit blocks stays unsplit (conv7: 256 tiles x K = 3872,
  // no partial slabs, no split sum; A/B 694 -> 698 frames/s against 4 splits)
  if (tiles >= cu_count()) sp = 1;
  if (sp > maxs) sp = maxs;
  if (sp > 64) sp = 64;
  if (sp < 1) sp = 1;
  long long kc = (T + sp - 1) / sp;
  kc = (kc + BK - 1) / BK * BK;
  sp = (T + kc - 1) / kc;
  // (conv5's F(4x4) at 32x32: 144 tiles x 2 splits = 288 blocks, measured
  // 52.5 -> 63.5 us: keep the 128x128 plan under three rounds of blocks)
  if (tiles * sp < 768 && !(sp == 1 && tiles >= cu_count()))
    return plan_wino_wgrad(T, cin_p, cout_p, nb);
  p.splits = (int)sp;
  p.kchunk = (int)kc;
  p.slab_floats = (size_t)nb * sp * cout_p * cin_p;
  if (sp > 1) p.slab_floats += (size_t)nb * cout_p * cin_p;
  return p;
}

extern "C" size_t nsm_wino_wgrad_h2_ws(int B, int H, int W, int cin_p, int cout_p, int tile) {
  WinoGeom g;
  if (!wino_geom(tile, B, H, W, g)) return 0;
  return plan_wino_wgrad_h2(g.T, cin_p, cout_p, g.alpha2).slab_floats;
}

extern "C" int nsm_wino_wgrad_h2_plan(int B, int H, int W, int cin_p, int cout_p, int tile,
                                      int* plan) {
  WinoGeom g;
  NSM_CHECK_ARG(plan && wino_geom(tile, B, H, W, g) && cin_p > 0 && cout_p > 0 && cin_p % 32 == 0 &&
                    cout_p % 32 == 0,
                "wino_wgrad_h2_plan: bad args");
  const WinoWgradPlan p = plan_wino_wgrad_h2(g.T, cin_p, cout_p, g.alpha2);
  plan[0] = p.BM;
  plan[1] = p.BN;
  plan[2] = p.splits;
  plan[3] = p.kchunk;
  return 0;
}

extern "C" int nsm_conv3x3_wgrad_wino_h2(const void* dMh, const void* Vh, int B, int H, int W,
                                         int cin_p, int cout_p, int cin, int cout, int tile,
                                         float* dw, float* ws, size_t ws_floats,
                                         const uint32_t* amax_dy, const uint32_t* amax_x,
                                         void* stream) {
  NSM_CHECK_ARG(dMh && Vh && dw && ws && amax_dy && amax_x, "conv3x3_wgrad_wino_h2: null pointer");
  NSM_CHECK_ARG(cin_p % 32 == 0 && cout_p % 32 == 0 && cin <= cin_p && cout <= cout_p,
                "conv3x3_wgrad_wino_h2: bad channels");
  NSM_CHECK_ARG(((uintptr_t)dMh % 16) == 0 && ((uintptr_t)Vh % 16) == 0 && ((uintptr_t)ws % 16) == 0,
                "conv3x3_wgrad_wino_h2: alignment");
  WinoGeom g;
  NSM_CHECK_ARG(wino_geom(tile, B, H, W, g), "conv3x3_wgrad_wino_h2: bad tile or shape");
  const int nb = g.alpha2;
  WinoWgradPlan pl = plan_wino_wgrad_h2(g.T, cin_p, cout_p, nb);
  if (ws_floats < pl.slab_floats) return fail(NSM_E_WS, "conv3x3_wgrad_wino_h2: workspace too small");
  NSM_CHECK_ARG(g.T * 2 * (long long)std::max(cin_p, cout_p) < (1ll << 30),
                "conv3x3_wgrad_wino_h2: operand too large");
  hipStream_t s = as_stream(stream);
  const int M = cout_p, N = cin_p;
  const int rc = wino_wgrad_gemm_h2((const bf16_t*)dMh, (const bf16_t*)Vh, g.T, cin_p, cout_p, nb,
                                    pl.BM, pl.BN, pl.kchunk, pl.splits, ws,
                                    H2Scale{amax_dy, wino_beta(tile, 1)},
                                    H2Scale{amax_x, wino_beta(tile, 0)}, s);
  if (rc) return rc;
  return wgrad_wino_finish(ws, pl, nb, M, N, cin, cout, tile, dw, s);
}

extern "C" int nsm_to_h2(const float* x, int64_t rows, int C, const uint32_t* amax, float beta,
                         void* out, void* stream) {
  NSM_CHECK_ARG(x && out && amax && rows > 0 && C > 0 && C % 8 == 0 && beta > 0.f,
                "to_h2: bad args");
  const long long g = std::min<long long>(ceil_div(rows * (C / 4), 256), 8192);
  hipLaunchKernelGGL(to_h2_kernel, dim3((int)g), dim3(256), 0, as_stream(stream), x,
                     (long long)rows, C, H2Scale{amax, beta}, (bf16_t*)out);
  NSM_LAUNCH_CHECK("to_h2");
  return 0;
}

extern "C" int nsm_wino_gemm_h2(const void* V, const void* U, int B, int H, int W, int cin_p,
                                int cout_p, int tile, float* Mb, const uint32_t* amax_v,
                                float beta_v, const uint32_t* amax_u, float beta_u,
                                void* stream) {
  NSM_CHECK_ARG(V && U && Mb && amax_v && amax_u && cin_p % 32 == 0 && cout_p % 32 == 0,
                "wino_gemm_h2: bad args");
  NSM_CHECK_ARG(((uintptr_t)V % 16) == 0 && ((uintptr_t)U % 16) == 0 && ((uintptr_t)Mb % 16) == 0,
                "wino_gemm_h2: 16B alignment");
  WinoGeom g;
  NSM_CHECK_ARG(wino_geom(tile, B, H, W, g), "wino_gemm_h2: bad tile or shape");
  NSM_CHECK_ARG(g.T * 2 * cin_p < (1ll << 30) && (long long)cout_p * 2 * cin_p < (1ll << 30),
                "wino_gemm_h2: operand too large");
  return wino_gemm_h2((const bf16_t*)V, (const bf16_t*)U, g.T, cin_p, cout_p, g.alpha2, Mb,
                      H2Scale{amax_v, beta_v}, H2Scale{amax_u, beta_u}, as_stream(stream));
}

extern "C" int nsm_wino_gemm_h2_plan(int B, int H, int W, int cin_p, int cout_p, int tile,
                                     int* plan) {
  WinoGeom g;
  NSM_CHECK_ARG(plan && wino_geom(tile, B, H, W, g) && cin_p > 0 && cout_p > 0 && cin_p % 32 == 0 &&
                    cout_p % 32 == 0,
                "wino_gemm_h2_plan: bad args");
  const WinoGemmH2Plan p = plan_wino_gemm_h2(g.T, cin_p, cout_p, g.alpha2);
  plan[0] = p.tile;
  plan[1] = p.form;
  return 0;
}

extern "C" int nsm_wino_gemm_f16_plan(int B, int H, int W, int cin_p, int cout_p, int tile, int o16,
                                      int* plan) {
  WinoGeom g;
  NSM_CHECK_ARG(plan && wino_geom(tile, B, H, W, g) && cin_p > 0 && cout_p > 0 && cin_p % 128 == 0 &&
                    cout_p % 128 == 0 && (o16 == 0 || o16 == 1),
                "wino_gemm_f16_plan: bad args");
  const WinoGemmF16Plan p = plan_wino_gemm_f16(g.T, cin_p, cout_p, g.alpha2);
  plan[0] = p.tile;
  plan[1] = p.form;
  return 0;
}

// the weight-gradient plan of the f16 path: the h2 plan's, on its 256 / 128 tiles
// (the bf16 path's Winograd weight gradient, nsm_conv.hip; declared in nsm_conv.h)
WinoWgradPlan nsm::plan_wino_wgrad_f16(long long T, int cin_p, int cout_p, int nb) {
  WinoWgradPlan p = plan_wino_wgrad_h2(T, cin_p, cout_p, nb);
  // NSM_F16_WG_SPLITS: K splits of the 256x256 tiles (A/B)
  static const long long force = env_int("NSM_F16_WG_SPLITS", 0);
  if (force > 0 && p.BM == 256 && p.BN == 256) {
    long long sp = force, maxs = (T + 255) / 256;
    if (sp > maxs) sp = maxs;
    long long kc = (T + sp - 1) / sp;
    kc = (kc + BK - 1) / BK * BK;
    sp = (T + kc - 1) / kc;
    p.splits = (int)sp;
    p.kchunk = (int)kc;
    p.slab_floats = (size_t)nb * sp * cout_p * cin_p;
    if (sp > 1) p.slab_floats += (size_t)nb * cout_p * cin_p;
  }
  if (force <= 0 && p.BM == 256 && p.BN == 256 && f16_wg_kt64()) {
    // K splits by a round model of the 256x256 blocks (one per CU): rounds x
    // (K / s x a + b) + the split sum's slab traffic c (s + 1) per tile, a, b,
    // c fitted on the B=64 step's conv5-conv7 weight gradients (kernel traces,
    // s = 1..8: conv6 1465 / 1299 / 1296 / 1345 us at s = 1..4, split sum
    // included; conv5 204 at s = 8 vs 136 at s = 3). The h2 planner's ~4
    // rounds left conv6 unsplit at 2.25 rounds and conv5 at 512-row splits
    const long long tiles = (long long)(cout_p / 256) * (cin_p / 256) * nb, cus = cu_count();
    const double a = 26.4e-3, b = 27.5, c = 0.0524;
    long long best = 1;
    double bt = 1e30;
    for (long long s = 1; s <= 8; ++s) {
      long long kc = (T + s - 1) / s;
      kc = (kc + BK - 1) / BK * BK;
      const long long se = (T + kc - 1) / kc;
      if (se != s) continue;
      const double t = (double)((tiles * s + cus - 1) / cus) * ((double)kc * a + b) +
                       (s > 1 ? c * (double)(s + 1) * (double)tiles : 0.0);
      if (t < bt) {
        bt = t;
        best = s;
      }
    }
    long long kc = (T + best - 1) / best;
    kc = (kc + BK - 1) / BK * BK;
    const long long sp = (T + kc - 1) / kc;
    p.splits = (int)sp;
    p.kchunk = (int)kc;
    p.slab_floats = (size_t)nb * sp * cout_p * cin_p;
    if (sp > 1) p.slab_floats += (size_t)nb * cout_p * cin_p;
  }
  if ((p.BM == 256 && p.BN == 256) || (p.BM == 128 && p.BN == 128)) return p;
  // (the h2 planner's smaller tiles: 128 x 128 with its ~512-block split)
  p.BM = p.BN = 128;
  const long long tiles = (long long)ceil_div(cout_p, 128) * ceil_div(cin_p, 128) * nb;
  long long sp = (512 + tiles - 1) / tiles, maxs = (T + 255) / 256;
  if (sp > maxs) sp = maxs;
  if (sp > 64) sp = 64;
  if (sp < 1) sp = 1;
  long long kc = (T + sp - 1) / sp;
  kc = (kc + BK - 1) / BK * BK;
  sp = (T + kc - 1) / kc;
  p.splits = (int)sp;
  p.kchunk = (int)kc;
  p.slab_floats = (size_t)nb * sp * cout_p * cin_p;
  if (sp > 1) p.slab_floats += (size_t)nb * cout_p * cin_p;
  return p;
}

extern "C" int nsm_wino_wgrad_f16_plan(int B, int H, int W, int cin_p, int cout_p, int tile,
                                       int* plan) {
  WinoGeom g;
  NSM_CHECK_ARG(plan && wino_geom(tile, B, H, W, g) && cin_p > 0 && cout_p > 0 && cin_p % 128 == 0 &&
                    cout_p % 128 == 0,
                "wino_wgrad_f16_plan: bad args");
  const WinoWgradPlan p = plan_wino_wgrad_f16(g.T, cin_p, cout_p, g.alpha2);
  plan[0] = p.BM;
  plan[1] = p.BN;
  plan[2] = p.splits;
  plan[3] = p.kchunk;
  return 0;
}
