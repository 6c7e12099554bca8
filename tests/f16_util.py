"""The comparator of the 16-bit train-path kernel tests (test_f16_ref.py,
test_gpu_f16_ops.py): float64 restatements of the operations, element-wise
worst-case bounds, and seeded case makers whose values are rounded through
the storage format before the reference sees them.

Notation: u = unit roundoff of the storage format (2^-11 f16, 2^-8 bf16),
tiny = half the smallest subnormal (2^-25 f16; bf16's subnormals lie below
anything the cases produce: 0), e32 = 2^-24. The matrix core accumulates the
exact products of two 16-bit operands in an fp32 chain, so

  stored GEMM output y = r(acc + bias)
      |got - ref| <= u |ref| + tiny + (1 + u) (K + 2) e32 S
      S = conv(|x|, |w|) + |b|,  K = taps * cin_p
  fp32 weight gradient
      |got - ref| <= (Kpix + 64) e32 S,  S = sum |dy| |a|,  Kpix = B H W
      (+ 64: the two-level slab sums of at most 512 splits)
  elementwise op storing 16 bits
      |got - ref| <= u |ref| + tiny + c e32 A (+ extra)
      A = sum of the absolute values of the op's terms, c = OPS[op] fp32
      operations on the longest path; extra = the propagated bound of an
      intermediate that the op's contract rounds to storage.

None of this is measured on the kernels."""
import types

import numpy as np
import torch
import torch.nn.functional as F

import eval_util as E

U = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
TINY = {"f16": 2.0 ** -25, "bf16": 0.0}
E32 = 2.0 ** -24
F16_MAX = 65504.0
F16_INF_FROM = 65520.0    # |v| >= this rounds to Inf (the tie goes to the even neighbour, Inf)
F16_MIN_NORMAL = 2.0 ** -14
SLOPE = 0.2

# fp32 operations on the longest path of each elementwise op (<= 16)
OPS = {
    "bn_act": 5,            # fma, slope, mask, + res, (contraction slack)
    "avgpool2": 4,          # 3 adds, * 0.25 (exact)
    "avgpool2_bwd_add": 2,  # * 0.25 (exact), + skip
    "resize": 8,            # 1 - l1, 4 tap products of two weights, 3 adds
    "resize_bwd": 12,       # <= 3 x 3 non-zero taps of a x2 upsample, weight products
    "up2_resize": 16,       # two bilinear steps (each as "resize")
    "up2_resize_bwd": 16,   # combined weights (3 ops per axis), their product, the window sum
    "bn_bwd_apply": 9,      # dz (fma, 2 products), k1 dz, y - mean, k2 (.), 2 adds, k2 / k3 rounding
    "head_bwd": 8,          # d = g (1 - o) o (3), 4 products, 3 adds -> within 8
}


def gemm_bound(ref, S, K, fmt):
    u = U[fmt]
    return u * ref.abs() + TINY[fmt] + (1 + u) * (K + 2) * E32 * S


def gemm_acc_term(S, K, fmt):
    return (1 + U[fmt]) * (K + 2) * E32 * S


def wgrad_bound(S, kpix):
    return (kpix + 64) * E32 * S


def elem_bound(ref, A, op, fmt, extra=0.0):
    return U[fmt] * ref.abs() + TINY[fmt] + OPS[op] * E32 * A + extra


def ratio(got, ref, bound):
    """worst |got - ref| / bound (inf if any element is not finite)."""
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isfinite(err), r, torch.full_like(r, float("inf")))
    return r.max().item() if r.numel() else 0.0


# ---- float64 restatements --------------------------------------------------------
def conv_ref(x, w, b, absval=False):
    """float64 NCHW conv (pad k // 2) of float32 operands; absval: of their
    absolute values (the S of the bounds)."""
    x, w = x.double(), w.double()
    b = None if b is None else b.double()
    if absval:
        x, w, b = x.abs(), w.abs(), None if b is None else b.abs()
    return F.conv2d(x, w, b, padding=w.shape[-1] // 2)


def dgrad_ref(dy, w, absval=False):
    dy, w = dy.double(), w.double()
    if absval:
        dy, w = dy.abs(), w.abs()
    return F.conv_transpose2d(dy, w, padding=w.shape[-1] // 2)


def wgrad_ref(a, dy, k, absval=False):
    """float64 dw [co, ci, k, k] = sum over pixels of dy (x) a."""
    a, dy = a.double(), dy.double()
    if absval:
        a, dy = a.abs(), dy.abs()
    B, ci, H, W = a.shape
    co = dy.shape[1]
    if k == 1:
        return torch.einsum("bohw,bihw->oi", dy, a).view(co, ci, 1, 1)
    ap = F.pad(a, (1, 1, 1, 1))
    dw = torch.empty(co, ci, 3, 3, dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            dw[:, :, r, s] = torch.einsum("bohw,bihw->oi", dy, ap[:, :, r:r + H, s:s + W])
    return dw


def lrelu(v, slope=SLOPE):
    return torch.where(v > 0, v, v * slope)


def prologue_ref(y1, sc, sh, mask, fmt, slope=SLOPE):
    """The operand the prologue loader feeds the GEMM: r(lrelu(y1 sc + sh) mask)
    from float64, NCHW (mask [B, C] or None). Returns (a, d): d >= 0 is the
    storage-grid step an element of a may be off by because the loader's four
    fp32 operations (error <= 4 e32 (|y1 sc| + |sh|) |mask|) land across a
    rounding boundary (zero almost everywhere)."""
    rnd = E.rounder(fmt)
    v = (1, -1, 1, 1)
    m = 1.0 if mask is None else mask.double()[:, :, None, None]
    t = y1.double() * sc.double().view(v)
    a64 = lrelu(t + sh.double().view(v), slope) * m
    delta = 4 * E32 * (t.abs() + sh.double().abs().view(v)) * (m if mask is None else m.abs())
    a = rnd(a64.float())
    d = (rnd((a64 + delta).float()) - rnd((a64 - delta).float())).abs().double()
    return a, d


def lin_matrix(n_in, n_out):
    """[n_out, n_in] float64 weights of the bilinear resize with align_corners
    in ATen's fp32 index arithmetic (scale = (in - 1) / (out - 1), src = scale *
    dst, l1 = src - floor(src), l0 = 1 - l1, all fp32): the operation's
    definition, which the kernels reproduce."""
    f = np.float32
    scale = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    l1 = np.clip((src - i0.astype(np.float32)).astype(np.float32), f(0), f(1))
    l0 = (f(1) - l1).astype(np.float32)
    i1 = i0 + (i0 < n_in - 1)
    m = np.zeros((n_out, n_in))
    o = np.arange(n_out)
    np.add.at(m, (o, i0), l0.astype(np.float64))
    np.add.at(m, (o, i1), l1.astype(np.float64))
    return torch.from_numpy(m)


def resample(x, wy, wx, absval=False):
    """float64 [B, C, Ho, Wo] = wy [Ho, Hi] . x [B, C, Hi, Wi] . wx^T."""
    x = x.double()
    if absval:
        x, wy, wx = x.abs(), wy.abs(), wx.abs()
    return torch.einsum("oh,bchw,pw->bcop", wy, x, wx)


def resize_mats(hi, wi, ho, wo):
    return lin_matrix(hi, ho), lin_matrix(wi, wo)


def up2_mats(h, w, th, tw):
    """x2 (align_corners) to (2h, 2w), then resize to (th, tw)."""
    def two(n, t):   # two non-zeros per row: a sparse product keeps wide rows cheap
        return torch.sparse.mm(lin_matrix(2 * n, t).to_sparse(), lin_matrix(n, 2 * n))
    return two(h, th), two(w, tw)


def bn_act_ref(y, scale, shift, fmt, res=None, mask=None, slope=SLOPE):
    """(z, A, bound) float64 of lrelu(y scale + shift) (* mask[b, c]) (+ res), NCHW."""
    v = (1, -1, 1, 1)
    m = 1.0 if mask is None else mask.double()[:, :, None, None]
    t = y.double() * scale.double().view(v)
    z = lrelu(t + shift.double().view(v), slope) * m
    A = (t.abs() + shift.double().abs().view(v)) * (m if mask is None else m.abs())
    if res is not None:
        z = z + res.double()
        A = A + res.double().abs()
    return z, A, elem_bound(z, A, "bn_act", fmt)


def avgpool_ref(x, absval=False):
    x = x.double().abs() if absval else x.double()
    return F.avg_pool2d(x, 2)


def avgpool_bwd(dy, H, W):
    """float64 gradient of avg_pool2d(., 2) at an [.., H, W] input (floor mode)."""
    dy = dy.double()
    up = 0.25 * dy.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return F.pad(up, (0, W - up.shape[3], 0, H - up.shape[2]))


# ---- case makers -------------------------------------------------------------------
def gen(*key):
    s = 7
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def grad_values(shape, g, fmt):
    """The `grad` regime, NCHW: signed magnitudes log-uniform over 2^-24 .. 2^4
    (a GradScaler-scaled gradient tail), rounded to storage; in f16 more than
    a third of them are subnormal. Every fourth channel (c % 4 == 3) and every
    other band of three rows ((h // 3) % 2 == 1) hold the tail alone (2^-24 ..
    2^-15), so that some sums over channels (a pixel of a GEMM output) and
    some sums over pixels (a row of a weight gradient) see subnormal operands
    only, and flushing them shows. bf16 callers use normal_values."""
    B, C, H, W = shape
    e = torch.rand(shape, generator=g, dtype=torch.float64)
    tail = ((torch.arange(C) % 4 == 3).view(1, C, 1, 1)
            | ((torch.arange(H) // 3) % 2 == 1).view(1, 1, H, 1)).expand(shape)
    mag = torch.pow(2.0, torch.where(tail, e * 9 - 24, e * 28 - 24))
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return E.rounder(fmt)((mag * sign).float())


def normal_values(shape, g, fmt, chan_dim=1):
    """The normal regime: randn with per-channel magnitudes 2^U(-2, 2), rounded."""
    ms = [1] * len(shape)
    ms[chan_dim] = shape[chan_dim]
    mag = torch.pow(2.0, torch.rand(ms, generator=g) * 4 - 2)
    return E.rounder(fmt)(torch.randn(shape, generator=g) * mag)


def subnormal_share(t):
    """Share of the non-zero-or-zero elements with |v| < 2^-14."""
    return (t.abs() < F16_MIN_NORMAL).double().mean().item()


def make_grad_case(B, H, W, ci, co, k, fmt, seed=0):
    """A convolution whose activation operand x is in the `grad` regime for
    f16 (normal for bf16); weights as eval_util.make_case."""
    c = E.make_case(B, H, W, ci, co, k, seed=seed, fmt=fmt)
    g = gen(seed, B, H, W, ci, co, k, 1)
    c.x = grad_values((B, ci, H, W), g, fmt) if fmt == "f16" else normal_values((B, ci, H, W), g, fmt)
    return c


TINY_X, TINY_W = 2.0 ** -10, 2.0 ** -9


def make_tiny_case(B, H, W, ci, co, k, seed=0):
    """`tiny_out` (f16): x ~ 2^-10, w ~ 2^-9 / sqrt(K) with per-output-channel
    magnitudes 2^U(-4, 1), no bias to speak of: the outputs lie in f16's
    subnormal range, part of them below its smallest subnormal."""
    g = gen(seed, B, H, W, ci, co, k, 2)
    rnd = E.rounder("f16")
    x = rnd(torch.randn(B, ci, H, W, generator=g) * TINY_X)
    omag = torch.pow(2.0, torch.rand(co, 1, 1, 1, generator=g) * 5 - 4)
    w = rnd(torch.randn(co, ci, k, k, generator=g) * omag * (TINY_W / (ci * k * k) ** 0.5))
    b = torch.randn(co, generator=g) * 2.0 ** -22
    return types.SimpleNamespace(B=B, H=H, W=W, ci=ci, co=co, k=k, fmt="f16", x=x, w=w, b=b)


def make_overflow_case(B, H, W, ci, co, k, seed=0):
    """`overflow` (f16): every fourth output channel (c % 4 == 1) has its
    weight row scaled by the power of two that brings the median |ref| of the
    channel nearest to 65504 (exact in f16: a power of two); the other
    channels are those of eval_util.make_case. case.hot: the scaled channels."""
    c = E.make_case(B, H, W, ci, co, k, seed=seed, fmt="f16")
    ref = conv_ref(c.x, c.w, c.b)
    hot = torch.arange(co) % 4 == 1
    med = ref.abs().permute(1, 0, 2, 3).reshape(co, -1).median(dim=1).values
    p = torch.round(torch.log2(F16_MAX / med)).clamp(0, 17)
    scale = torch.where(hot, torch.pow(2.0, p), torch.ones(co, dtype=torch.float64)).float()
    c.w = c.w * scale.view(-1, 1, 1, 1)
    assert torch.equal(c.w.half().float(), c.w)
    c.hot = hot
    return c


def overflow_classes(ref, S, K):
    """(inf: the reference rounds to +-Inf, ambiguous: |ref| within the
    accumulation term of the 65520 rounding boundary) of an f16 store."""
    a = ref.abs()
    return a >= F16_INF_FROM, (a - F16_INF_FROM).abs() <= gemm_acc_term(S, K, "f16")


# ---- mutants (test_f16_ref.py) -------------------------------------------------------
def toward_zero_f16(t):
    """fp32 -> f16 rounded toward zero (the store-rounding mutant)."""
    h = t.half()
    bits = h.view(torch.int16)
    over = h.float().abs() > t.abs()
    return torch.where(over, bits - 1, bits).view(torch.float16)


def toward_zero_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def flush_subnormal(t):
    return torch.where(t.float().abs() < F16_MIN_NORMAL, torch.zeros_like(t), t)
