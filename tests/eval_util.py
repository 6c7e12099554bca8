"""The comparator of the eval-epilogue tests (test_eval_ref.py,
test_gpu_eval_ops.py): a float64 restatement of one eval-mode block step,

    c = conv(x [resized], w) + b
    z = lrelu((c - rmean) * gamma / sqrt(rvar + eps) + beta, slope) (+ res)

and a seeded input maker whose cases make a wrong channel, a wrong sign or a
dropped term visible: per-channel input magnitudes 2^U(-2,2), gamma of mixed
sign, running variances 2^U(-4,4), running means / biases / betas of order 1
(both LeakyReLU branches well populated; test_eval_ref.py asserts the share)."""
import types

import torch
import torch.nn.functional as F

EPS, SLOPE = 1e-5, 0.2

# (B, H, W, cin, cout, k): the op-level shapes shared by the fp32 and the 16-bit tests
SMALL = [(2, 9, 11, 32, 64, 3), (1, 16, 16, 64, 32, 3), (3, 7, 5, 32, 128, 1), (1, 5, 67, 32, 32, 3)]
# One smallest shape per larger tile, M ragged against it (H, W odd or H*W no
# multiple of the tile): (B, H, W, cin, cout, k, rows), rows = the tile's row
# count as the host query reports it.
# fp32 (dispatch_conv_fwd, mb128 = ceil(M / 128)): 128-row tiles from
# mb128 * ceil(N / BN) >= 512 (M >= 65409), 256-row tiles for N <= 64 from
# mb128 >= 4096 (M >= 524161)
F32_LARGE = [(1, 209, 313, 32, 128, 1, 128),   # 128x128
             (1, 209, 313, 32, 64, 1, 128),    # 128x64
             (1, 209, 313, 32, 32, 1, 128),    # 128x32
             (1, 209, 313, 32, 32, 3, 128),    # 128x32, 3x3 (im2col loader)
             (1, 723, 725, 32, 64, 1, 256),    # 256x64
             (1, 723, 725, 32, 32, 1, 256)]    # 256x32
# 16-bit (conv_fwd_bm_b / dispatch_conv_fwd_b, mb256 = ceil(M / 256)); the
# 512x128 tile writes 256-row partials, so the query says 256 for it too
S16_LARGE = [(1, 511, 513, 64, 64, 1, 256),    # 256x64 LDS-DMA: N = 64, mb256 >= 1024
             (1, 511, 513, 32, 64, 1, 256),    # 256x64 register (cin no multiple of 64)
             (1, 239, 257, 64, 256, 1, 256),   # 256x256 LDS-DMA: mb256 * 2 >= 480
             (1, 351, 350, 64, 128, 1, 256),   # 512x128 LDS-DMA: mb256 >= 480
             (1, 201, 203, 64, 384, 1, 256),   # 256x128 LDS-DMA: mb256 * 3 >= 480
             (1, 351, 350, 96, 128, 1, 256),   # 256x128 register (cin 96)
             (1, 209, 313, 32, 32, 3, 128)]    # 128x32 LDS-DMA: 3x3, cin = N = 32, M >= 65409
# fp32 Winograd act shapes (B, H, W, cin, cout) and (B, hi, wi, H, W, cin, cout)
WINO = [(2, 9, 11, 32, 64), (2, 7, 5, 64, 32), (1, 16, 16, 128, 128), (1, 23, 45, 64, 64)]
WINO_SRC = [(2, 5, 7, 10, 14, 32, 64), (1, 17, 30, 34, 60, 64, 32)]
# the bf16 path's F(4x4) on f16 operands, same layouts
WINO_F16 = [(1, 13, 22, 512, 512), (2, 16, 16, 512, 1024)]
WINO_F16_SRC = [(1, 9, 15, 18, 30, 512, 512)]


def rounder(fmt):
    """Round-trip through the storage format ('f32' is the identity)."""
    if fmt == "bf16":
        return lambda t: t.to(torch.bfloat16).float()
    if fmt == "f16":
        return lambda t: t.half().float()
    assert fmt == "f32", fmt
    return lambda t: t


def make_case(B, H, W, ci, co, k, seed=0, fmt="f32", src_hw=None, round_w=True):
    """One seeded case, float32 CPU tensors in the reference (NCHW) layout:
    x [B, ci, h, w] (h, w = src_hw or H, W), w [co, ci, k, k], b, gamma, beta,
    rmean, rvar [co], res [B, co, H, W]. x, res (and w unless round_w=False)
    are representable in `fmt`, so a float64 reference of them is the
    reference of what the device reads."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * B + 131 * H + 17 * W + 5 * ci + 3 * co + k)
    rnd = rounder(fmt)
    h, wd = src_hw if src_hw is not None else (H, W)
    mag = torch.pow(2.0, torch.rand(1, ci, 1, 1, generator=g) * 4 - 2)
    x = rnd(torch.randn(B, ci, h, wd, generator=g) * mag)
    w = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
    if round_w:
        w = rnd(w)
    sign = torch.where(torch.rand(co, generator=g) < 0.25, -1.0, 1.0)
    return types.SimpleNamespace(
        B=B, H=H, W=W, ci=ci, co=co, k=k, src_hw=src_hw, fmt=fmt, eps=EPS, slope=SLOPE,
        x=x, w=w, b=torch.randn(co, generator=g),
        gamma=(torch.rand(co, generator=g) + 0.5) * sign,
        beta=torch.randn(co, generator=g),
        rmean=torch.randn(co, generator=g),
        rvar=torch.pow(2.0, torch.rand(co, generator=g) * 8 - 4),
        res=rnd(torch.randn(B, co, H, W, generator=g)))


def bn_vectors(gamma, beta, rmean, rvar, eps):
    """float64 (scale, shift, mean, invstd) of an eval-mode BatchNorm."""
    gamma, beta, rmean, rvar = (t.double() for t in (gamma, beta, rmean, rvar))
    inv = 1.0 / torch.sqrt(rvar + eps)
    scale = gamma * inv
    return scale, beta - rmean * scale, rmean, inv


def eval_block_ref(x, w, b, gamma, beta, rmean, rvar, eps, slope, res=None, resize_to=None):
    """float64 (c, z), NCHW. resize_to=(H, W): x is first resized (bilinear,
    align_corners) as the decoder's upsample does."""
    x = x.double()
    if resize_to is not None:
        x = F.interpolate(x, size=tuple(resize_to), mode="bilinear", align_corners=True)
    c = F.conv2d(x, w.double(), None if b is None else b.double(), padding=w.shape[-1] // 2)
    v = (1, -1, 1, 1)
    pre = ((c - rmean.double().view(v)) * (gamma.double().view(v) / torch.sqrt(rvar.double().view(v) + eps))
           + beta.double().view(v))
    z = torch.where(pre >= 0, pre, pre * slope)
    if res is not None:
        z = z + res.double()
    return c, z


def reference(case, res=False):
    """(c, z) of a make_case case."""
    return eval_block_ref(case.x, case.w, case.b, case.gamma, case.beta, case.rmean, case.rvar,
                          case.eps, case.slope, res=case.res if res else None,
                          resize_to=(case.H, case.W) if case.src_hw is not None else None)


def branch_shares(case):
    """(share of outputs on the positive LeakyReLU branch, on the negative one)."""
    c, _ = reference(case)
    scale, shift, _, _ = bn_vectors(case.gamma, case.beta, case.rmean, case.rvar, case.eps)
    pre = c * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    pos = (pre > 0).double().mean().item()
    return pos, (pre < 0).double().mean().item()


def nhwc(t):
    """[B, C, H, W] -> [B*H*W, C]"""
    B, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()
