// The bf16 convolutions (BASELINE config 3): the 16-bit implicit-GEMM body
// nsm_conv_s16.inc instantiated for bf16 (namespace nsm_bf) with its C entries,
// and the three C entries that dispatch on dtype (nsm_conv_fwd_act,
// nsm_conv1x1_bnbwd_chunks, nsm_conv1x1_dgrad_bnbwd: their f16 and fp32 cases
// are calls into nsm_conv_f16.hip / nsm_conv.hip). Includes nsm_conv.h and,
// inside nsm_bf, nsm_conv_s16.inc.
#include "nsm_conv.h"

// The 16-bit conv body is compiled twice: here for bf16 (namespace nsm_bf) and
// in nsm_conv_f16.hip for f16 (nsm_h). Not nested in nsm: argument-dependent
// lookup on nsm's types (F8) would otherwise see nsm's bf16 helpers beside
// nsm_h's f16 ones.
namespace nsm_bf {
using namespace nsm;
__device__ __forceinline__ f32x16 mfma_s16_32(bf16x8 a, bf16x8 b, f32x16 c, int, int, int) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_s16_16(bf16x8 a, bf16x8 b, f32x4 c, int, int, int) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// bits of a value already rounded to bf16 (round_bf)
__device__ __forceinline__ bf16_t s16_bits(float v) { return (bf16_t)(__float_as_uint(v) >> 16); }
__device__ __forceinline__ void st8s(bf16_t* p, F8 v) { nsm::st8(p, v); }
#include "nsm_conv_s16.inc"
}  // namespace nsm_bf

using namespace nsm;
using namespace nsm_bf;

extern "C" int nsm_pack_conv_weight_bf16(const float* w, int cout, int cin, int ksize, int cout_p,
                                         int cin_p, int mode, void* out, void* stream) {
  return s16_pack_conv_weight(w, cout, cin, ksize, cout_p, cin_p, mode, out, stream);
}

extern "C" int nsm_conv_fwd_bf16(const void* x, int ldx, int B, int H, int W, int cin_p,
                                 const void* wpk, const float* bias, int cout_p, int ksize, void* y,
                                 int ldy, const float* pro_scale, const float* pro_shift,
                                 const float* pro_mask, float slope, float* stats, void* stream) {
  return s16_conv_fwd(x, ldx, B, H, W, cin_p, wpk, bias, cout_p, ksize, y, ldy, pro_scale,
                      pro_shift, pro_mask, slope, stats, stream);
}

// BN-partial rows / weight-gradient workspace: the tile plans do not depend on
// the 16-bit format (the f16 convolutions use these two as well)
extern "C" int nsm_conv_stat_rows_bf16(int B, int H, int W, int cout_p) {
  return conv_fwd_bm_b((long long)B * H * W, cout_p);
}

extern "C" size_t nsm_conv_wgrad_bf16_ws(int B, int H, int W, int cin_p, int cout_p, int ksize) {
  // the plan depends on whether the call carries a prologue: cover both
  const size_t a = plan_wgrad_b(B, H, W, cin_p, cout_p, ksize, false).ws_floats;
  const size_t b = plan_wgrad_b(B, H, W, cin_p, cout_p, ksize, true).ws_floats;
  return a > b ? a : b;
}

extern "C" int nsm_conv_wgrad_bf16(const void* dy, int lddy, const void* x, int ldx, int B, int H,
                                   int W, int cin_p, int cout_p, int ksize, const float* pro_scale,
                                   const float* pro_shift, const float* pro_mask, float slope,
                                   float* ws, size_t ws_floats, int cin, int cout, float* dw,
                                   void* stream) {
  return s16_conv_wgrad(dy, lddy, x, ldx, B, H, W, cin_p, cout_p, ksize, pro_scale, pro_shift,
                        pro_mask, slope, ws, ws_floats, cin, cout, dw, stream);
}

// ---- eval-mode conv + BN + LeakyReLU (+ skip) in one pass --------------------
extern "C" int nsm_conv_fwd_act(const void* x, int ldx, int B, int H, int W, int cin_p,
                                const void* wpk, const float* bias, int cout_p, int ksize, void* y,
                                int ldy, const float* act_scale, const float* act_shift,
                                float slope, const void* res, int ldres, int dtype, void* stream) {
  return for_dtype(dtype, "conv_fwd_act", [&, s = as_stream(stream)](auto t) {
    using T = typename decltype(t)::type;
    if constexpr (std::is_same<T, float>::value)
      return conv_fwd_act_f32((const T*)x, ldx, B, H, W, cin_p, (const T*)wpk, bias, cout_p, ksize,
                              (T*)y, ldy, act_scale, act_shift, slope, (const T*)res, ldres, s);
    else  // the two 16-bit formats share a signature
      return (std::is_same<T, bf16_t>::value ? nsm_bf::s16_conv_fwd_act : conv_fwd_act_f16)(
          x, ldx, B, H, W, cin_p, wpk, bias, cout_p, ksize, y, ldy, act_scale, act_shift, slope,
          res, ldres, s);
  });
}

// ---- 1x1 input gradient with the BN backward in its epilogue (EpiBnBwd) ----
// (cop: the 16-bit tile choice depends on it; the fp32 one does not)
extern "C" int nsm_conv1x1_bnbwd_chunks(int B, int H, int W, int cip, int cop, int dtype) {
  const long long M = (long long)B * H * W;
  const int rows = dtype != NSM_F32 ? nsm_bf::bnbwd_rows_b(M, cip, cop) : conv_fwd_bm_f(M, cip);
  return ceil_div(M, rows);
}

extern "C" int nsm_conv1x1_dgrad_bnbwd(const void* dy2, int lddy2, int B, int H, int W, int cop,
                                       const void* w2d, int cip, const void* y1, int ldy1,
                                       const float* scale, const float* shift, const float* mean,
                                       const float* invstd, const float* mask, float slope,
                                       int mode, float* partial, const float* coef, void* out,
                                       int ldo, int dtype, const uint32_t* amax_dy2,
                                       const uint32_t* amax_w, uint32_t* amax_out, void* stream) {
  NSM_CHECK_ARG(dy2 && w2d && y1 && scale && shift && mean, "conv1x1_dgrad_bnbwd: null pointer");
  NSM_CHECK_ARG(mode >= 0 && mode <= 2, "conv1x1_dgrad_bnbwd: mode %d", mode);
  NSM_CHECK_ARG(mode == 2 || (partial && invstd), "conv1x1_dgrad_bnbwd: modes 0/1 need partials");
  NSM_CHECK_ARG(mode == 0 || out, "conv1x1_dgrad_bnbwd: modes 1/2 need an output");
  NSM_CHECK_ARG(mode != 2 || coef, "conv1x1_dgrad_bnbwd: mode 2 needs coef");
  NSM_CHECK_ARG(B > 0 && H > 0 && W > 0 && cop % 32 == 0 && cip % 32 == 0,
                "conv1x1_dgrad_bnbwd: bad shape");
  NSM_CHECK_ARG(lddy2 >= cop && lddy2 % 8 == 0 && ldy1 >= cip && ldy1 % 8 == 0 &&
                    (mode == 0 || (ldo >= cip && ldo % 8 == 0)),
                "conv1x1_dgrad_bnbwd: bad leading dims");
  NSM_CHECK_ARG(((uintptr_t)dy2 % 16) == 0 && ((uintptr_t)w2d % 16) == 0 &&
                    ((uintptr_t)y1 % 16) == 0 && ((uintptr_t)out % 16) == 0,
                "conv1x1_dgrad_bnbwd: 16-B alignment");
  const long long Ml = (long long)B * H * W;
  NSM_CHECK_ARG(Ml < (1ll << 30), "conv1x1_dgrad_bnbwd: too many pixels");
  BnBwdEpiP ep{out, ldo, y1, ldy1, scale, shift, mean, invstd, coef, mask,
               make_fastdiv((uint32_t)(H * W)), slope, partial, mode};
  if (dtype == NSM_F32 && mode == 2) ep.amax = amax_out;
  // 16-bit modes 0/1: amax_out receives max|scale * dz|, the k1 term of the dY1
  // bound nsm_bn_bwd_finalize derives (the lazy-dY1 dual transform's scale)
  if (dtype != NSM_F32 && mode != 2) ep.k1dz = amax_out;
  return for_dtype(dtype, "conv1x1_dgrad_bnbwd", [&, s = as_stream(stream)](auto t) {
    using T = typename decltype(t)::type;
    constexpr bool bf = std::is_same<T, bf16_t>::value;
    if constexpr (std::is_same<T, float>::value)
      return conv1x1_dgrad_bnbwd_f32((const T*)dy2, lddy2, B, H, W, cop, (const T*)w2d, cip, ep,
                                     amax_dy2, amax_w, s);
    else
      return (bf ? nsm_bf::s16_conv1x1_dgrad_bnbwd : conv1x1_dgrad_bnbwd_f16)(
          dy2, lddy2, B, H, W, cop, w2d, cip, ep, s);
  });
}
