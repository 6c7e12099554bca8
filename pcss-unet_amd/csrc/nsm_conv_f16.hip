// The f16 convolutions (the fp16-autocast mode): the 16-bit implicit-GEMM body
// nsm_conv_s16.inc instantiated for IEEE half (namespace nsm_h, where
// nsm_fmt_f16.h shadows the format helpers the body calls) and its C entries.
// conv_fwd_act_f16 and conv1x1_dgrad_bnbwd_f16 are the f16 cases of the
// entries that dispatch on dtype (nsm_conv_bf16.hip; declared in nsm_conv.h).
// Includes nsm_conv.h and, inside nsm_h, nsm_fmt_f16.h and nsm_conv_s16.inc.
#include "nsm_conv.h"

namespace nsm_h {
using namespace nsm;
#include "nsm_fmt_f16.h"
#include "nsm_conv_s16.inc"
}  // namespace nsm_h

using namespace nsm;

extern "C" int nsm_pack_conv_weight_f16(const float* w, int cout, int cin, int ksize, int cout_p,
                                        int cin_p, int mode, void* out, void* stream) {
  return nsm_h::s16_pack_conv_weight(w, cout, cin, ksize, cout_p, cin_p, mode, out, stream);
}

extern "C" int nsm_conv_fwd_f16(const void* x, int ldx, int B, int H, int W, int cin_p,
                                const void* wpk, const float* bias, int cout_p, int ksize, void* y,
                                int ldy, const float* pro_scale, const float* pro_shift,
                                const float* pro_mask, float slope, float* stats, void* stream) {
  return nsm_h::s16_conv_fwd(x, ldx, B, H, W, cin_p, wpk, bias, cout_p, ksize, y, ldy, pro_scale,
                             pro_shift, pro_mask, slope, stats, stream);
}

extern "C" int nsm_conv_wgrad_f16(const void* dy, int lddy, const void* x, int ldx, int B, int H,
                                  int W, int cin_p, int cout_p, int ksize, const float* pro_scale,
                                  const float* pro_shift, const float* pro_mask, float slope,
                                  float* ws, size_t ws_floats, int cin, int cout, float* dw,
                                  void* stream) {
  return nsm_h::s16_conv_wgrad(dy, lddy, x, ldx, B, H, W, cin_p, cout_p, ksize, pro_scale,
                               pro_shift, pro_mask, slope, ws, ws_floats, cin, cout, dw, stream);
}

int nsm::conv_fwd_act_f16(const void* x, int ldx, int B, int H, int W, int cin_p, const void* wpk,
                          const float* bias, int cout_p, int ksize, void* y, int ldy,
                          const float* act_scale, const float* act_shift, float slope,
                          const void* res, int ldres, hipStream_t s) {
  return nsm_h::s16_conv_fwd_act(x, ldx, B, H, W, cin_p, wpk, bias, cout_p, ksize, y, ldy, act_scale,
                                 act_shift, slope, res, ldres, s);
}

int nsm::conv1x1_dgrad_bnbwd_f16(const void* dy2, int lddy2, int B, int H, int W, int cop,
                                 const void* w2d, int cip, const BnBwdEpiP& ep, hipStream_t s) {
  return nsm_h::s16_conv1x1_dgrad_bnbwd(dy2, lddy2, B, H, W, cop, w2d, cip, ep, s);
}
