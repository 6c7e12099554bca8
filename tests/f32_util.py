"""The comparator of the fp32 direct-GEMM tests (test_f32_ref.py,
test_gpu_f32_ops.py): element-wise worst-case bounds of an fp32 GEMM output in
the three arithmetic modes of set_f32_split, a spread-magnitude case maker,
and numpy/torch emulations of the two split GEMMs (with mutants) that prove
the bounds on the CPU. The float64 restatements (conv_ref, dgrad_ref,
wgrad_ref), ratio and gen are f16_util's, make_case / nhwc eval_util's.

Notation. a, b: the two fp32 operands of the GEMM; S = conv(|a|, |b|) (+ |bias|)
the absolute-value restatement of the output; K the accumulation length
(taps * cin_p for the forward and the input gradient, B H W for the weight
gradient); e32 = 2^-24. Everything below is derived from the header comments
of csrc/nsm_conv_split.inc and csrc/nsm_conv_split16.inc and from counting
operations in the kernels' source. None of it is measured on the kernels.

Accumulation, every mode:   (1 + g) (K + c) e32 S
  The matrix core adds the products of the K elements of a row into one fp32
  accumulator per output. The model, as in f16_util: one fp32 rounding per K
  element, each relative to a partial sum of at most S. It holds for mode 0
  if v_mfma_f32_32x32x2_f32 fuses product and sum, and for the split modes,
  which issue 3 (f16x2) or 6 (bf16x6) 16-deep MFMAs per 16 K elements, if an
  MFMA rounds at most once per 3 / 6 of its 16 products. A chain that rounded
  after every product of every split term would give 3 K / 6 K: should a
  kernel miss the bound by a factor between 1 and 6 at a long K, this model
  is the first thing to re-derive.
  c = 2 for the forward and the input gradient: the bias add of the epilogue
  (one rounding of acc + bias, S holds |bias|), and one unit for the
  second-order terms of (1 + e32)^(K + 1) (K <= 1152 here). The zero
  initialisation and the power-of-two undo factors of mode 2 are exact.
  c = 64 for the weight gradient, as f16_util.wgrad_bound: the K elements
  are spread over at most 512 split-K slabs, whose fp32 sums are two-level:
  splitsum_kernel adds 16 slabs in two chains of 8 and joins them (9 adds
  deep), wgrad_reduce_kernel adds at most 32 groups in four chains and joins
  them (10 adds deep); 19 <= 64.
  g covers that the split terms the core really adds are not a b but the
  rounded pieces: sum |pieces products| <= (1 + g) S, g = 2^-9 for the f16x2
  split (|h| <= (1 + 2^-11) |x s|, |l| <= 2^-11 (1 + 2^-11) |x s|, three
  terms), 2^-5 for the bf16 split (u = 2^-8, six terms), 0 for mode 0.

Mode 1 in addition:   3 e32 S
  x = h + m + l exactly (three bf16 of 8 significand bits, nsm_conv_split.inc)
  with |m| <= 2^-8 (1 + 2^-8) |x|, |l| <= 2^-16 (1 + 2^-8) |x|. The kernel
  drops am bl, al bm, al bl: (2 2^-24 + 2^-32) (1 + 2^-8)^2 |a b| < 3 e32 |a b|.

Mode 2 in addition, with s = 2^(15 - ceil log2 amax_a), t likewise for b, as
pow2_scale_exp computes them from the VALUE IN THE SLOT (pow2_up below: a slot
holding an upper bound of the maximum gives a larger power of two), X = a s,
Y = b t (|X|, |Y| <= 2^15, exact):
  h = f16(X), l = f16(X - h) leave dX = X - h - l with
      |dX| <= 2^-22 |X| + 2^-25      (2^-25: half the f16 subnormal spacing,
                                      what remains once l is subnormal, i.e.
                                      for |X| < 2^-2 = 2^-17 of 2^15)
      |l|  <= (2^-11 |X| + 2^-25) (1 + 2^-11)
  X Y - (hx hy + hx ly + lx hy) = lx ly + dX Y + (X - dX) dY, so per K element
      |.| <= |X||Y| (3 2^-22 + 2^-31) + (|X| + |Y|) (2^-25 + 2^-35) + 2^-48
  and after the undo factor 1 / (s t), summed over K:
      representation   (3 2^-22 + 2^-31) S        (two operands and the l l product)
      floor            2^-40 (1 + 2^-10) (Pa conv(1, |b|) + Pb conv(|a|, 1))
                       + K 2^-78 Pa Pb             (both pieces at their floors)
  Pa = pow2_up(amax_a) = 2^15 / s, Pb likewise. The last term is what the
  products of two floor-sized pieces add; it matters only where both
  operands of an output are below 2^-38 of their maxima.

The weight gradient's K elements are pixels, its a = dy, b = the activation.

BN backward of the 1x1 input gradient (nsm_conv1x1_dgrad_bnbwd): dY1 = k1 dz +
k2 (y - mean) + k3, dz = dA1 lrelu'(y scale + shift) mask. The bound of dY1
is the GEMM bound of dA1 times |k1 lrelu' mask| plus f16_util.OPS["bn_bwd_apply"]
e32 (|k1 dz| + |k2 (y - mean)| + |k3|). The per-channel sums S1 = sum dz,
S2 = sum dz xhat are fp32 inside a row chunk and float64 across chunks:
  |got - ref| <= sum of the propagated dA1 bounds + BN_SUM_OPS e32 sum |terms|
               + 4 sum over the undetermined-branch elements of |term|
                 (slope 0.2 taken for 1: the term grows by (1 - 0.2) / 0.2)
  BN_SUM_OPS = 48: dz (3: slope constant, two products), xhat and its product
  (3), a lane's rows (<= 16) + the wave shuffles (<= 6) + the waves of a block
  (<= 4) + margin to 32, nsm_sum_rows' groups (<= 8), the store as float (1)."""
import types

import numpy as np
import torch
import torch.nn.functional as F

from eval_util import make_case, nhwc  # noqa: F401  (with the next line: what the tests reach through this module)
from f16_util import conv_ref, dgrad_ref, gen, ratio, wgrad_ref  # noqa: F401

E32 = 2.0 ** -24
C_CONV, C_WGRAD = 2, 64
ACC_SLACK = {0: 0.0, 1: 2.0 ** -5, 2: 2.0 ** -9}
DROPPED_BF16 = 3 * E32
REP_F16X2 = 3 * 2.0 ** -22 + 2.0 ** -31
FLOOR_F16X2 = 2.0 ** -40 * (1 + 2.0 ** -10)
FLOOR2_F16X2 = 2.0 ** -78
TINY_REL = 2.0 ** -17          # below this share of the (power-of-two) maximum l is subnormal
BN_SUM_OPS = 48


def pow2_up(m):
    """2^15 / s of pow2_scale_exp for a slot holding m >= 0: the power of two
    at or above m (0, Inf, NaN: s = 1, i.e. 2^15; the exponent 15 - e clamped
    to [-126, 126])."""
    m = np.float32(m)
    u = int(np.array(m, dtype=np.float32).view(np.uint32)) & 0x7fffffff
    if u == 0 or u >= 0x7f800000:
        return 2.0 ** 15
    e = (u >> 23) - 127
    if u & 0x7fffff:
        e += 1
    se = max(-126, min(126, 15 - e))
    return 2.0 ** (15 - se)


def floor_term(amax_a, amax_b, a_ones, ones_b, K):
    """Mode 2's small-value floor: a_ones = conv(|a|, 1), ones_b = conv(1, |b|)
    (float64), amax_*: the slot values."""
    pa, pb = pow2_up(amax_a), pow2_up(amax_b)
    return FLOOR_F16X2 * (pa * ones_b + pb * a_ones) + K * FLOOR2_F16X2 * pa * pb


def gemm_bound(mode, S, K, c=C_CONV, floor=None):
    """Element-wise bound of an fp32 GEMM output in `mode` (0: fp32 MFMA, 1:
    bf16 three-way split, 2: f16x2 split; floor = floor_term(...), required)."""
    b = (1 + ACC_SLACK[mode]) * (K + c) * E32 * S
    if mode == 1:
        b = b + DROPPED_BF16 * S
    elif mode == 2:
        b = b + REP_F16X2 * S + floor
    else:
        assert mode == 0, mode
    return b


def wgrad_bound(mode, S, kpix, floor=None):
    return gemm_bound(mode, S, kpix, c=C_WGRAD, floor=floor)


def sum_bound(prop, terms, unsure):
    """Bound of a per-channel fp32 / float64 sum over (B, H, W) of NCHW terms:
    prop = the propagated bound of every term, unsure = the elements whose
    LeakyReLU branch the fp32 pre-activation does not determine (1 vs slope)."""
    t = terms.abs()
    return (prop.sum((0, 2, 3)) + BN_SUM_OPS * E32 * t.sum((0, 2, 3))
            + 4.0 * (t * unsure).sum((0, 2, 3)))


def tiny_share(t):
    """Share of the non-zero elements below 2^-17 of pow2_up(max|t|)."""
    a = t.abs()
    nz = a > 0
    return ((a < TINY_REL * pow2_up(a.max().item())) & nz).double().sum().item() / max(1, int(nz.sum()))


# ---- case makers -------------------------------------------------------------------
def spread(g, n, lo=-12, hi=0):
    """n magnitudes 2^U(lo, hi)."""
    return torch.pow(2.0, torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


def make_spread_case(B, H, W, ci, co, k, seed=0):
    """A convolution whose operands spread over many binades, so that a good
    share of both lies below 2^-17 of the tensor maximum (mode 2's floor) and
    whole output rows / channels are made of such elements alone: x = randn
    times a per-channel and a per-image-row magnitude 2^U(-12, 0), w = randn /
    sqrt(K) times a per-output-channel and a per-input-channel one. In every
    other band of three image rows ((h // 3) % 2 == 1) a pixel keeps one
    channel only ((h + w) % ci): the outputs there are sums of a few products,
    where a dropped low-order term of a split is not hidden by K. The bias is
    2^-22 randn times the output channel's magnitude: far above the bound of
    the small outputs (a dropped bias shows), yet its rounding term e32 |b|
    stays below their floor term."""
    g = gen(seed, B, H, W, ci, co, k, 5)
    x = torch.randn(B, ci, H, W, generator=g) * spread(g, ci).view(1, ci, 1, 1) * spread(g, H).view(1, 1, H, 1)
    hh, ww = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    lone = ((hh // 3) % 2 == 1).expand(H, W)
    keep = torch.arange(ci).view(ci, 1, 1) == ((hh + ww) % ci).view(1, H, W)
    x = torch.where(lone.view(1, 1, H, W) & ~keep.view(1, ci, H, W), torch.zeros(()), x)
    omag = spread(g, co)
    w = (torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
         * omag.view(co, 1, 1, 1) * spread(g, ci).view(1, ci, 1, 1))
    b = torch.randn(co, generator=g) * omag * 2.0 ** -22
    return types.SimpleNamespace(B=B, H=H, W=W, ci=ci, co=co, k=k, fmt="f32", x=x, w=w, b=b, lone=lone)


def conv_floor(x, w, amax_x, amax_w):
    """floor_term of the forward convolution of NCHW x with w (zero padding:
    the taps outside the image load exact zeros). conv(|x|, 1) is the same for
    every output channel and conv(1, |w|) sees the sum over the input channels."""
    k = w.shape[-1]
    ci = x.shape[1]
    a_ones = conv_ref(x, torch.ones(1, ci, k, k), None, absval=True)
    ones_b = conv_ref(torch.ones_like(x[:, :1]), w.double().abs().sum(1, keepdim=True), None)
    return floor_term(amax_x, amax_w, a_ones, ones_b, k * k * ci)


def dgrad_floor(dy, w, amax_dy, amax_w):
    k = w.shape[-1]
    co = dy.shape[1]
    a_ones = dgrad_ref(dy, torch.ones(co, 1, k, k), absval=True)
    ones_b = dgrad_ref(torch.ones_like(dy[:, :1]), w.double().abs().sum(0, keepdim=True))
    return floor_term(amax_dy, amax_w, a_ones, ones_b, k * k * co)


def wgrad_floor(a, dy, k, amax_dy, amax_a):
    B, _, H, W = a.shape
    a_ones = wgrad_ref(torch.ones_like(a[:, :1]), dy, k, absval=True)     # conv(|dy|, 1): [co, 1, k, k]
    ones_b = wgrad_ref(a, torch.ones_like(dy[:, :1]), k, absval=True)     # conv(1, |a|): [1, ci, k, k]
    return floor_term(amax_dy, amax_a, a_ones, ones_b, B * H * W)


# ---- CPU emulations of the split GEMMs (test_f32_ref.py) ------------------------------
def im2col(x, k):
    """[B, ci, H, W] fp32 -> [B H W, ci k k] (copies, zero padding)."""
    B, ci, H, W = x.shape
    return F.unfold(x, k, padding=k // 2).permute(0, 2, 1).reshape(B * H * W, ci * k * k).contiguous()


def _mm32(a, b):
    """fp32 [M, K] x [N, K]^T accumulated in fp32 (the products of two 16-bit
    pieces are exact in fp32)."""
    with np.errstate(invalid="ignore", over="ignore"):    # a mutant may overflow f16
        return torch.from_numpy(np.matmul(a.numpy().astype(np.float32), b.numpy().astype(np.float32).T))


def f16x2_gemm(a, b, amax_a, amax_b, drop_hl=False, drop_last=False, swap_scales=False):
    """[M, K] x [N, K]^T as gemm_f32h_kernel forms it: scale by 2^(15 - ceil
    log2 max), h = f16(x s), l = f16(x s - h), three product terms in fp32,
    the scales undone. Mutants: drop_hl (the two h l terms), drop_last (the
    last K element), swap_scales (each operand scaled from the other's slot)."""
    sa, sb = 2.0 ** 15 / pow2_up(amax_a), 2.0 ** 15 / pow2_up(amax_b)
    if swap_scales:
        sa, sb = sb, sa

    def split(x, s):
        xs = (x.double() * s).float()      # a power of two: exact
        h = xs.half()
        return h.float(), (xs - h.float()).half().float()

    if drop_last:
        a, b = a[:, :-1], b[:, :-1]
    (ah, al), (bh, bl) = split(a, sa), split(b, sb)
    acc = _mm32(ah, bh)
    if not drop_hl:
        acc = (_mm32(al, bh) + _mm32(ah, bl)) + acc
    return ((acc.double() / sa) / sb).float()


def bf16x6_gemm(a, b, drop_mm=False, drop_mh=False):
    """The exact three-way bf16 split with the six kept terms (smallest first);
    drop_mm / drop_mh: the am bm / the am bh term left out."""
    def split(x):
        h = x.to(torch.bfloat16).float()
        m = (x - h).to(torch.bfloat16).float()
        return h, m, (x - h - m).to(torch.bfloat16).float()

    (ah, am, al), (bh, bm, bl) = split(a), split(b)
    acc = _mm32(al, bh) + _mm32(ah, bl)
    if not drop_mm:
        acc = acc + _mm32(am, bm)
    if not drop_mh:
        acc = acc + _mm32(am, bh)
    return (acc + _mm32(ah, bm)) + _mm32(ah, bh)
