"""The comparator of the stage-level tests of the bf16 step's Winograd
F(4x4,3x3) path on single-plane scaled f16 operands (test_wino_f16_ref.py,
test_gpu_wino_f16_ops.py): float64 restatements of every stage, element-wise
worst-case bounds, case makers, and a numpy / torch stand-in of the kernels'
operation sequence (with mutants) that proves the bounds on the CPU. The
Cook-Toom matrices, the transform bounds (OPS), the slot exponent (h2_exp) and
the chain helpers are wino_util's, the accumulation bounds f32_util's.

Notation: e32 = 2^-24, u16 = 2^-11 (f16), ub = 2^-8 (bf16), |.| element-wise.

Single-plane storage (csrc/nsm_conv.hip wino_*_f16_kernel, prep kind 6): an
  operand [36][T][C] holds rn_f16(v 2^e), e = h2_exp(slot, beta), beta =
  nsm_wino_beta(4, which). It is the h plane of an h2 tensor on its own:
      |stored 2^-e - ref| <= tbound (1 + u16) + u16 |ref| + 2^-40 (1 + 2^-10) P
  (wino_util.h2_h_bound; P = 2^15 / 2^e; 2^-40 P = half the f16 subnormal
  spacing, which is all that is left of a value below 2^-29 P = SUB_REL P).
  |stored| <= 2^15 and no Inf, whatever the data.

Sources rounded to bf16 inside a transform (the resize's interpolated value,
  nsm_wino_dual_bn_f16's dY1): the kernel rounds an fp32 value within fb of
  the float64 one d, so the patch element is within
      ub (|d| + fb) + fb
  of d (the fp32 error may move the rounding to the neighbour: that is the ub
  fb term), carried through |C| . |C|^T by wino_util.windows_ref.

GEMM (gemm_h2q_kernel / gemm_h2p_kernel, SP): the reference is the float64
  product of the DECODED stored operands, which are the stage's exact inputs.
  The products of two f16 are exact in fp32, so only the accumulation term
  f32_util.gemm_bound(0, S, K) = (K + 2) e32 S, S = |V| |U|^T, remains. The
  undo factors are powers of two.

f16 M (O16): M16 = rn_f16(acc 2^e_t), acc in the operands' scaled units, one
  e_t = pow2_scale_exp(max|acc| over the tile) per 64 x 64 tile and component.
  With a the accumulators (|a - ref| <= b element-wise) the tile maximum lies
  in [max(|ref| - b), max(|ref| + b)], so e_t lies between the exponents of
  these two numbers (m16_expect); equal almost everywhere. P_t = 2^15 / 2^e_t
  from the smaller admissible exponent (the looser floor):
      |M16 2^-e_t - ref| <= b (1 + u16) + u16 |ref| + 2^-40 (1 + 2^-10) P_t
  and, of the kernel's output alone, 2^14 <= max|M16| <= 2^15 on every
  non-zero tile (2^14 itself where the maximum rounds down to it).

Output transform (wino_output_kernel / wino_output_f16m_buf_kernel): fp32
  A^T M A + b by wino_util.output_ref's bound bo, then one bf16 rounding:
      ub (|ref| + bo) + bo
  _act: z = o a + s (3 roundings on |o a| + |s|, bo carried through |a|), the
  LeakyReLU is 1-Lipschitz and adds one rounding for the slope product.
  The undo factor is 2^clamp(-e_t - e_v, -126, 126) 2^-e_u: past the clamp
  the result is M16 2^(+-126 - e_u), not the true M (m16_decode(clamp=True)).
  BN partials [nslot][3][N] = {sum, M2 about the slot mean, count}: thread
  slot s takes the Winograd tiles s, s + nslot, s + 2 nslot, ..., each tile's
  {count, mean, M2} Chan-merged into the slot's in fp32 (partials_ref).
  nsm_bn_finalize_train merges the slots in double: the slots' bounds carried
  through that merge, one fp32 rounding each for mean and variance, INV_OPS
  for 1 / sqrtf(var + eps) (merged_ref).

Weight gradient: dU = dM^T V of the decoded operands under
  f32_util.wgrad_bound(0, S, T), carried through |G^T| . |G| with the filter
  transform's own roundings on top (wino_util.wgrad_ref's shape).

None of this is measured on the kernels."""
import numpy as np
import torch

import f16_util as H
import f32_util as S
import wino_util as Wn

TILE, NB = 4, 36
E32 = 2.0 ** -24
U16, UB = H.U["f16"], H.U["bf16"]
SUB_REL = 2.0 ** -29          # below this share of P a stored value is f16-subnormal
TOP = 2.0 ** 15
MT = 64                       # the exponent tile of the f16 M


def bf(t):
    """Round-trip through bf16."""
    return t.to(torch.bfloat16).float()


# ---- single-plane storage ------------------------------------------------------------
def sp_decode(t, slot, beta):
    return t.double() * 2.0 ** (-Wn.h2_exp(slot, beta))


def sp_bound(ref, tbound, slot, beta):
    return Wn.h2_h_bound(ref, tbound, slot, beta)


def sp_ratio(t, ref, tbound, slot, beta):
    """Worst err / bound of a stored operand (any shape matching ref); inf if
    it holds an Inf / NaN or a value above 2^15."""
    t = t.reshape(ref.shape)
    if not torch.isfinite(t.float()).all() or t.float().abs().max().item() > TOP:
        return float("inf")
    return H.ratio(sp_decode(t, slot, beta), ref, sp_bound(ref, tbound, slot, beta))


def sp_tiny_share(ref, slot, beta):
    return Wn.tiny_share(ref, Wn.h2_P(slot, beta), SUB_REL)


def pow2(x):
    """2^x of an int or an integer tensor (|x| <= 1022) as float64, from the
    exponent bits: a device pow is not exact."""
    if not torch.is_tensor(x):
        return 2.0 ** int(x)
    return ((x.long() + 1023) << 52).view(torch.float64)


def sp_encode(v, e, trunc=False, flush=False):
    """f16 rn(v 2^e) of fp32 v (e an int or an integer tensor). Mutants:
    trunc (rounded toward zero), flush (f16 subnormals to zero)."""
    xs = (v.double() * pow2(e)).float()
    h = H.toward_zero_f16(xs) if trunc else xs.half()
    return H.flush_subnormal(h) if flush else h


# ---- sources rounded to bf16 inside a transform ---------------------------------------
def rounded_bound(d, fb):
    """Bound of bf16(fp32 value within fb of d) against d."""
    return UB * (d.abs() + fb) + fb


def input_ref(x, src=None):
    """(V ref, bound) in plane layout of NCHW bf16-valued x; src = (wy, wx):
    the align_corners resize sampled per patch element and rounded to bf16."""
    if src is None:
        ref, b, _ = Wn.input_ref(x, TILE)
        return ref, b
    wy, wx = (m.to(x.device) for m in src)
    d = H.resample(x, wy, wx)
    fb = H.OPS["resize"] * E32 * H.resample(x, wy, wx, absval=True)
    return Wn.windows_ref(Wn.patches(d, TILE), Wn.patches(rounded_bound(d, fb), TILE), TILE, "Bt")


def bn_dy_ref(g, y, scale, shift, mean, coef, mask):
    """(dY1, bound) of the bf16 dY1 nsm_wino_dual_bn_f16 forms per element."""
    dy, b = Wn.bn_dy_ref(g, y, scale, shift, mean, coef, mask)
    return dy, rounded_bound(dy, b)


# ---- GEMM ---------------------------------------------------------------------------------
def gemm_ref(V16, U16_, ev, eu):
    """(ref, bound) of M[c] = V[c] U[c]^T from the stored operands V16
    [nb][T][K], U16 [nb][N][K] (f16) decoded with 2^-ev, 2^-eu."""
    Vd, Ud = V16.double() * 2.0 ** -ev, U16_.double() * 2.0 ** -eu
    K = V16.shape[-1]
    ref = Vd @ Ud.transpose(1, 2)
    Sa = Vd.abs() @ Ud.abs().transpose(1, 2)
    return ref, S.gemm_bound(0, Sa, K)


def exp_of(m):
    """pow2_scale_exp of float32(m), element-wise (int64)."""
    m32 = m.float()
    mant, ex = torch.frexp(m32)
    e = torch.where(mant == 0.5, ex - 1, ex).long()
    se = (15 - e).clamp(-126, 126)
    return torch.where((m32 == 0) | ~torch.isfinite(m32), torch.zeros_like(se), se)


def tile_max(a):
    """[nb][T][N] -> [nb][ceil(T / 64)][N / 64] maxima (rows past T count 0)."""
    nb, T, N = a.shape
    R = -(-T // MT)
    p = torch.zeros(nb, R * MT, N, dtype=a.dtype, device=a.device)
    p[:, :T] = a
    return p.view(nb, R, MT, N // MT, MT).amax((2, 4))


def expand(e, T, N):
    """A per-tile quantity [nb][R][Q] at every element [nb][T][N]."""
    return e.repeat_interleave(MT, 1)[:, :T].repeat_interleave(MT, 2)[:, :, :N]


def m16_expect(ref, bound, ev, eu):
    """(e_lo, e_hi) [nb][R][Q]: the admissible range of the tile exponents,
    from the reference alone (module docstring)."""
    sc = 2.0 ** (ev + eu)
    e_lo = exp_of(tile_max((ref.abs() + bound) * sc))
    e_hi = exp_of(tile_max((ref.abs() - bound).clamp(min=0) * sc))
    return e_lo, e_hi


def m16_Pt(e_lo, ev, eu, T, N):
    """P_t of the looser admissible exponent, in M's own units, per element."""
    return expand(pow2(15 - e_lo) * 2.0 ** -(ev + eu), T, N)


def m16_bound(ref, bound, e_lo, ev, eu):
    nb, T, N = ref.shape
    return bound * (1 + U16) + U16 * ref.abs() + Wn.FLOOR * m16_Pt(e_lo, ev, eu, T, N)


def m16_decode(M16, et, ev, eu, clamp=False):
    """float64 M of a stored f16 M [nb][T][N] with tile exponents et
    [nb][R][Q]; clamp: as the output transform undoes it, 2^clamp(-e_t - e_v,
    -126, 126) 2^-e_u."""
    nb, T, N = M16.shape
    x = -(expand(et.long(), T, N) + ev)
    if clamp:
        x = x.clamp(-126, 126)
    return M16.double() * pow2(x) * 2.0 ** -eu


def m16_tiles_ok(M16, et):
    """Of the kernel's output alone: no Inf / NaN, every non-zero tile's
    maximum in [2^14, 2^15], an all-zero tile with exponent 0."""
    a = M16.float().abs()
    if not torch.isfinite(a).all():
        return False
    m = tile_max(a)
    zero = m == 0
    ok = torch.where(zero, et == 0, (m >= 2.0 ** 14) & (m <= TOP))
    return bool(ok.all())


def m16_ratio(M16, et, ref, bound, ev, eu):
    """(worst err / bound of the decoded f16 M, whether every exponent is
    admissible, whether the tiles are well formed)."""
    e_lo, e_hi = m16_expect(ref, bound, ev, eu)
    et = et.long()
    adm = bool(((et >= e_lo) & (et <= e_hi)).all())
    r = H.ratio(m16_decode(M16, et, ev, eu), ref, m16_bound(ref, bound, e_lo, ev, eu))
    return r, adm, m16_tiles_ok(M16, et)


# ---- output transform -------------------------------------------------------------------------
def output_ref(Mp, bias, B, H_, W_, act=None):
    """(y ref, bound) NCHW of the bf16 output of M [36][T][N] (float64, the
    test's own); act = (scale, shift, slope): lrelu(y scale + shift)."""
    ref, bo = Wn.output_ref(Mp, bias, B, H_, W_, TILE)
    if act is not None:
        a, s, slope = act
        a, s = a.double().view(1, -1, 1, 1), s.double().view(1, -1, 1, 1)
        z = ref * a + s
        bz = a.abs() * bo + 3 * E32 * ((ref * a).abs() + s.abs())
        ref, bo = H.lrelu(z, slope), bz + E32 * z.abs()
    return ref, rounded_bound(ref, bo)


def tile_pixels(y):
    """NCHW [B, N, H, W] -> (values [T][N][16], valid [T][1][16]) of the 4 x 4
    output tiles in the kernels' tile order."""
    B, N, H_, W_ = y.shape
    p = Wn.inner(Wn.patches(y, TILE))                              # [B, N, TH, TW, 4, 4]
    v = Wn.inner(Wn.patches(torch.ones(B, 1, H_, W_, dtype=y.dtype, device=y.device), TILE))
    flat = lambda t: t.permute(0, 2, 3, 1, 4, 5).reshape(-1, t.shape[1], 16)  # noqa: E731
    return flat(p), flat(v) > 0


MEAN_OPS = 25     # a tile mean: <= 15 adds, the reciprocal and its product; a merge: delta, the weight
#                   (2), the product and the add, on values of at most max|y|: 17 + 6, + 2 margin


def partials_ref(y, nslot):
    """float64 per-slot statistics of the kernel's own rounded y (NCHW) and
    their fp32 bounds: dict of count [nslot], sum, m2, sum_bound, m2_bound
    [nslot][N]. Slot s: the tiles s + k nslot, merged in that order."""
    vals, valid = tile_pixels(y.double())
    T, N, _ = vals.shape
    nv = valid.double().sum(-1)                                     # [T][1]
    ts = (vals * valid).sum(-1)
    tmean = ts / nv
    tq = (((vals - tmean[..., None]) ** 2) * valid).sum(-1)
    tabs = (vals.abs() * valid).sum(-1)
    tmax = (vals.abs() * valid).amax(-1)
    kmax = -(-T // nslot)

    def slots(t):
        p = torch.zeros(kmax * nslot, t.shape[1], dtype=t.dtype, device=t.device)
        p[:T] = t
        return p.view(kmax, nslot, t.shape[1])
    nv, ts, tmean, tq, tabs, tmax = (slots(t) for t in (nv, ts, tmean, tq, tabs, tmax))
    z = torch.zeros(nslot, N, dtype=torch.float64, device=y.device)
    n, mean, m2, ssum, sabs, ymax, bm2 = (z.clone() for _ in range(7))
    ntile = torch.zeros(nslot, 1, dtype=torch.float64, device=y.device)
    for k in range(kmax):
        on = nv[k] > 0
        n2 = n + nv[k]
        w = torch.where(on, n * nv[k] / n2.clamp(min=1), torch.zeros_like(n))
        delta = torch.where(on, tmean[k] - mean, torch.zeros_like(mean))
        ymax = torch.maximum(ymax, tmax[k])
        dm = MEAN_OPS * (k + 1) * E32 * ymax
        bm2 = bm2 + w * (4 * delta.abs() * dm + 4 * dm * dm) + nv[k] * dm * dm
        mean = mean + delta * nv[k] / n2.clamp(min=1)
        m2 = m2 + torch.where(on, tq[k], torch.zeros_like(m2)) + w * delta * delta
        ssum, sabs, n = ssum + ts[k], sabs + tabs[k], n2
        ntile = ntile + on.double()
    return {"count": n[:, 0], "sum": ssum, "m2": m2,
            "sum_bound": (15 + ntile) * E32 * sabs,
            "m2_bound": (25 + 2 * ntile) * E32 * m2 + bm2}


INV_OPS = 8       # 1 / sqrtf(var + eps) in fp32: the add (1), sqrtf (1 ulp = 2), the division (2.5 ulp = 5)


def merged_ref(y, nslot, eps):
    """(mean, its bound, 1 / sqrt(var + eps), its bound) [N] that
    nsm_bn_finalize_train forms from the slots' fp32 partials of NCHW y. The
    merge runs in double in a fixed order (its own roundings are below 2^-40
    of the terms and left out): mean = float(sum_s S_s / M), so the slots' sum
    bounds / M and one fp32 rounding; m2 = sum_s M2_s + n_s (S_s / n_s - mean)^2,
    so the slots' M2 bounds plus n_s (2 |d_s| e_s + e_s^2), e_s = the error of
    S_s / n_s - mean; var = float(m2 / M); the inverse deviation INV_OPS more."""
    r = partials_ref(y, nslot)
    n = r["count"][:, None]
    M = n.sum()
    on = n > 0
    mean = r["sum"].sum(0) / M
    mb0 = r["sum_bound"].sum(0) / M
    d = torch.where(on, r["sum"] / n.clamp(min=1) - mean, torch.zeros_like(r["sum"]))
    e = r["sum_bound"] / n.clamp(min=1) + mb0
    m2 = (r["m2"] + n * d * d).sum(0)
    m2b = (r["m2_bound"] + torch.where(on, n * (2 * d.abs() * e + e * e), torch.zeros_like(e))).sum(0)
    var = m2 / M
    vb = m2b / M + E32 * var
    rel = vb / (var + eps)
    inv = 1.0 / torch.sqrt(var + eps)
    return mean, mb0 + E32 * mean.abs(), inv, inv * (0.5 * rel / (1 - rel) + INV_OPS * E32)


# ---- weight gradient ----------------------------------------------------------------------------
def wgrad_ref(dM16, V16, ed, ev, cout, cin):
    """(dw ref, bound) [cout][cin][3][3] = G^T (sum_t dM^T V) G of the stored
    operands dM16 [36][T][M], V16 [36][T][N] decoded with 2^-ed, 2^-ev."""
    D, X = dM16.double() * 2.0 ** -ed, V16.double() * 2.0 ** -ev
    T = D.shape[1]
    dU = D.transpose(1, 2) @ X
    gb = S.wgrad_bound(0, D.abs().transpose(1, 2) @ X.abs(), T)
    return gt_carry(dU, gb, cout, cin)


def gt_carry(dU, gb, cout, cin):
    """dU [36][M][N] within gb -> (G^T dU G, bound) of the real channels."""
    Gt = Wn.cmat(TILE, "Gt", dU.device)

    def win(t):
        return t[:, :cout, :cin].reshape(6, 6, cout, cin).permute(2, 3, 0, 1)
    ab = Wn.two_pass(win(dU).abs() + win(gb), Gt.abs())
    return (Wn.two_pass(win(dU), Gt),
            Wn.two_pass(win(gb), Gt.abs()) + Wn.OPS[(TILE, "Gt")][0] * E32 * ab)


# ---- the chained convolution ----------------------------------------------------------------------
def chain_gemm(Vr, eV, Ur, eU, ev, eu, m16):
    """(M ref, M bound) of the GEMM whose stored operands are within eV / eU
    of Vr / Ur; m16: M is then stored as f16 under the loosest admissible
    tile exponent."""
    Va, Ua = Vr.abs() + eV, Ur.abs() + eU
    K = Vr.shape[-1]
    prop = Va @ eU.transpose(1, 2) + eV @ Ur.abs().transpose(1, 2)
    Mr = Vr @ Ur.transpose(1, 2)
    eM = prop + S.gemm_bound(0, Va @ Ua.transpose(1, 2), K)
    if m16:
        e_lo, _ = m16_expect(Mr, eM, ev, eu)
        eM = m16_bound(Mr, eM, e_lo, ev, eu)
    return Mr, eM


def chain_output(Mr, eM, bias, B, H_, W_):
    """(y ref, bound) of the bf16 y from M within eM of Mr."""
    ref, b = Wn.chain_output(Mr, eM, bias, B, H_, W_, TILE)
    return ref, rounded_bound(ref, b)


# ---- case makers --------------------------------------------------------------------------------------
def make_calib(B, H_, W_, C, seed=0):
    """wino_util.make_calib in bf16 values (NCHW fp32)."""
    return bf(Wn.make_calib(B, H_, W_, C, seed))


def make_spread(B, H_, W_, C, seed=0, lo=-44):
    """bf16 values whose per-channel magnitudes cover 2^U(lo, 0) and per-row
    ones 2^U(-12, 0) (bf16 has fp32's exponent range), so that a good share of
    the transformed values lies below 2^-29 of the operand's power-of-two
    maximum, the f16 floor; lone-channel bands as wino_util.make_spread."""
    g = H.gen(seed, B, H_, W_, C, 31)
    x = (torch.randn(B, C, H_, W_, generator=g) * S.spread(g, C, lo, 0).view(1, C, 1, 1)
         * S.spread(g, H_).view(1, 1, H_, 1))
    hh, ww = torch.arange(H_).view(H_, 1), torch.arange(W_).view(1, W_)
    lone = ((hh // 3) % 2 == 1).expand(H_, W_)
    keep = torch.arange(C).view(C, 1, 1) == ((hh + ww) % C).view(1, H_, W_)
    return bf(torch.where(lone.view(1, 1, H_, W_) & ~keep.view(1, C, H_, W_), torch.zeros(()), x))


def make_x(kind, B, H_, W_, C, seed=0):
    return (make_spread if kind == "spread" else make_calib)(B, H_, W_, C, seed)


def make_filters(co, ci, seed=0, spread=False, lo=-40):
    """fp32 filters; spread: per-output- and per-input-channel magnitudes
    2^U(lo, 0) / 2^U(-12, 0)."""
    g = H.gen(seed, co, ci, 32)
    w = torch.randn(co, ci, 3, 3, generator=g) / (9 * ci) ** 0.5
    if spread:
        w = w * S.spread(g, co, lo, 0).view(co, 1, 1, 1) * S.spread(g, ci).view(1, ci, 1, 1)
    return w


def gemm_operands(kind, nb, T, K, N, seed=0):
    """fp32 V [nb][T][K], U [nb][N][K] of the GEMM tests. calib: randn with
    per-component magnitudes 2^U(-3, 3) / 2^U(-6, -3). spread: on top, V's
    rows and U's output channels carry magnitudes 2^U(-24, 0) drawn
    independently INSIDE every 64-row / 64-column exponent tile (the first row
    and channel of a tile keep 1, so a tile's maximum stays at the top), so
    that a good share of M lies below 2^-29 of its tile's maximum."""
    g = H.gen(seed, nb, T, K, N, 33)
    V = torch.randn(nb, T, K, generator=g) * S.spread(g, nb, -3, 3).view(nb, 1, 1)
    U = torch.randn(nb, N, K, generator=g) * S.spread(g, nb, -6, -3).view(nb, 1, 1)
    if kind == "spread":
        rm, cm = S.spread(g, T, -24, 0), S.spread(g, N, -24, 0)
        rm[::MT], cm[::MT] = 1.0, 1.0
        V, U = V * rm.view(1, T, 1), U * cm.view(1, N, 1)
    return V, U


def m16_tiny_share(ref, e_lo, ev, eu):
    nb, T, N = ref.shape
    return Wn.tiny_share(ref, m16_Pt(e_lo, ev, eu, T, N), SUB_REL)


# ---- the stand-in: the kernels' operation sequence on the CPU -------------------------------------------
def emu_sp(v, slot, beta, exp_off=0, swap_chunks=False, **mut):
    """fp32 [rows][C] -> the stored f16 [rows][C]. Mutants: exp_off (the
    producer's exponent off by that much), swap_chunks (8-channel chunk 0 of
    every row swapped with chunk 1), trunc, flush (sp_encode)."""
    out = sp_encode(v, Wn.h2_exp(slot, beta) + exp_off, **mut)
    if swap_chunks:
        out = torch.cat((out[:, 8:16], out[:, 0:8], out[:, 16:]), 1)
    return out


def _planes(K):
    """Channel indices of the two same-plane products of the SP k-steps: the
    8-channel chunks of even / odd index of every 64-channel K-tile."""
    c = torch.arange(K)
    odd = (c // 8) % 2 == 1
    return c[~odd], c[odd]


def emu_gemm_sp(V16, U16_, drop_half=False, cross=False):
    """One component's accumulators (fp32, scaled units) of f16 V16 [T][K],
    U16 [N][K]: h_0(A) h_0(B) + h_1(A) h_1(B). Mutants: drop_half (the h_1
    product of the last K-tile left out), cross (h_0(A) h_1(B) + h_1(A) h_0(B))."""
    K = V16.shape[1]
    p0, p1 = _planes(K)
    A, Bm = V16.float(), U16_.float()
    if cross:
        return S._mm32(A[:, p0], Bm[:, p1]) + S._mm32(A[:, p1], Bm[:, p0])
    q1 = p1[p1 < K - 64] if drop_half else p1
    return S._mm32(A[:, p0], Bm[:, p0]) + S._mm32(A[:, q1], Bm[:, q1])


def emu_o16(acc, static_k=0, **mut):
    """The O16 epilogue on accumulators [nb][T][N]: (M16, e_t). Mutant:
    static_k = K: the static exponent -(15 + ceil log2 K) for every tile."""
    nb, T, N = acc.shape
    et = exp_of(tile_max(acc.abs()))
    if static_k:
        et = torch.full_like(et, -(15 + int(np.ceil(np.log2(static_k)))))
    return sp_encode(acc, expand(et, T, N), **mut), et


def emu_output(Mp, bias, B, H_, W_, act=None, drop_bias=False, trunc=False):
    """fp32 M [36][T][N] -> (bf16-valued y NCHW fp32, the unrounded fp32 y)."""
    TH, TW = Wn.tiles_hw(H_, W_, TILE)
    X = Wn.from_planes(Mp.float(), B, TH, TW).contiguous().numpy()
    o = torch.from_numpy(Wn.emu_wmat2(Wn.cmat32(TILE, "At"), X))
    y = o.permute(0, 1, 2, 4, 3, 5).reshape(B, -1, TH * TILE, TW * TILE)[:, :, :H_, :W_]
    if bias is not None and not drop_bias:
        y = y + bias.view(1, -1, 1, 1)
    if act is not None:
        a, s, slope = act
        z = y * a.view(1, -1, 1, 1) + s.view(1, -1, 1, 1)
        y = torch.where(z > 0, z, z * np.float32(slope))
    y = y.contiguous()
    return (H.toward_zero_bf16(y).float() if trunc else bf(y)), y


def emu_partials(y, nslot):
    """[nslot][3][N] fp32 partials of NCHW y as the output transform forms them."""
    vals, valid = tile_pixels(y.float())
    T, N, _ = vals.shape
    f = np.float32
    out = np.zeros((nslot, 3, N), f)
    vals, valid = vals.numpy(), valid.numpy()
    for s in range(nslot):
        s_n, s_mean, s_m2, s_sum = f(0), np.zeros(N, f), np.zeros(N, f), np.zeros(N, f)
        for t in range(s, T, nslot):
            ok = valid[t, 0]
            nv = f(ok.sum())
            ts = np.zeros(N, f)
            for i in np.nonzero(ok)[0]:
                ts = ts + vals[t, :, i]
            tmean = ts * (f(1) / nv)
            tq = np.zeros(N, f)
            for i in np.nonzero(ok)[0]:
                d = vals[t, :, i] - tmean
                tq = tq + d * d
            n2 = s_n + nv
            delta = tmean - s_mean
            s_mean = s_mean + delta * (nv / n2)
            s_m2 = s_m2 + tq + delta * delta * (s_n * nv / n2)
            s_sum, s_n = s_sum + ts, n2
        out[s, 0], out[s, 1], out[s, 2] = s_sum, s_m2, s_n
    return torch.from_numpy(out)


def partials_ratio(part, y, nslot):
    """(counts equal, worst sum ratio, worst M2 ratio) of partials [nslot][3][N]
    against partials_ref of y."""
    r = partials_ref(y, nslot)
    p = part.double()
    cnt = bool((p[:, 2] == r["count"][:, None]).all())
    return cnt, H.ratio(p[:, 0], r["sum"], r["sum_bound"]), H.ratio(p[:, 1], r["m2"], r["m2_bound"])
