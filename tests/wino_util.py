"""The comparator of the stage-level Winograd tests (test_wino_ref.py,
test_gpu_wino_f32_ops.py): float64 restatements of every stage of the fp32
Winograd F(2x2) / F(4x4) / F(6x6) path on pre-split (h2) operands, element-wise
worst-case bounds, case makers, and a numpy stand-in of the kernels' operation
sequence (with mutants) that proves the bounds on the CPU.

The Cook-Toom matrices are tools/wino_coeffs.py::mats (exact fractions), not
the kernels' tables. Notation: e32 = 2^-24; C the matrix of a two-pass
transform Y = C X C^T; |.| element-wise absolute values.

Transform (wmat / wmat2 / wcol_row of csrc/nsm_conv.hip, contraction off):
  a row of C with n non-zero coefficients costs at most n fp32 roundings per
  pass (the first product, then one add / sub / fma per further coefficient),
  each relative to a partial sum of at most sum |c| |x|. Two passes, one unit
  for the second-order terms, and one unit per pass where a coefficient of C
  is not an fp32 number (the G matrices of F(4x4), F(6x6): 1/3, 1/15, 1/90..):
      |got - ref| <= c e32 (|C| |X| |C|^T),  c = 2 nnz + 1 (+ 2)      (OPS)
  nnz = the largest count of non-zeros in a row of C.
  A source sampled by the align_corners resize inside the transform adds
  f16_util.OPS["resize"] e32 on the resampled |x| (weights >= 0), carried
  through |C| . |C|^T like the data.

h2 storage (include/nsm.h, csrc/nsm_common.h h2_exp / split4h): an operand
  value v is stored as h = f16(v s), l = f16(v s - h), s = 2^e,
  e = 15 - ceil log2(float32(slot) float32(beta)) clamped to [-126, 126]
  (a finite slot whose product overflows saturates at FLT_MAX):
      |(h + l) / s - v| <= 2^-22 |v| + 2^-40 (1 + 2^-10) P,  P = 2^15 / s
  (f32_util's dX bound; 2^-25 / s = 2^-40 P). The decode takes e from the
  slot and nsm_wino_beta, never from the kernel's output. The h plane alone
  is v rounded to nearest: |h / s - v| <= 2^-11 |v| + 2^-40 P (h2_h_bound).
  The GEMMs drop the l l product on the strength of |l| <= 2^-11 |v s|; an h
  rounded toward zero keeps h + l within the first bound but doubles |l|.

GEMM on h2 operands: f32_util.gemm_bound(2, S, K, floor=floor_term(...)) with
  the slot values times beta as the operand maxima. Weight gradient:
  f32_util.wgrad_bound with K = T, then the G^T transform bound on top,
  the GEMM's bound carried through |G^T| . |G|.

None of this is measured on the kernels."""
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

import f16_util as H
import f32_util as S

E32 = 2.0 ** -24
REP = 2.0 ** -22
FLOOR = 2.0 ** -40 * (1 + 2.0 ** -10)
TILES = (2, 4, 6)
NAMES = ("Bt", "A", "At", "G", "Gt")

_spec = importlib.util.spec_from_file_location(
    "wino_coeffs", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "tools", "wino_coeffs.py"))
_wc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_wc)


def _frac_mat(tile, name):
    AT, G, BT = _wc.mats(tile)
    M = {"Bt": BT, "At": AT, "G": G}.get(name)
    if M is None:
        M = {"A": AT, "Gt": G}[name]
        M = [list(r) for r in zip(*M)]
    return M


def _is_f32(fr):
    return type(fr)(float(np.float32(float(fr)))) == fr


def cmat(tile, name, device="cpu"):
    """float64 C of the transform `name` (Bt: input, A: output gradient,
    At: output, G: filter, Gt: weight-gradient output), exact to 2^-53."""
    return torch.tensor([[float(v) for v in r] for r in _frac_mat(tile, name)], dtype=torch.float64,
                        device=device)


def cmat32(tile, name):
    """The fp32 coefficients a kernel holds (numpy float32)."""
    return np.array([[float(v) for v in r] for r in _frac_mat(tile, name)], dtype=np.float32)


def _ops():
    out = {}
    for t in TILES:
        for n in NAMES:
            M = _frac_mat(t, n)
            nnz = max(sum(1 for v in r if v != 0) for r in M)
            inexact = any(not _is_f32(v) for r in M for v in r)
            out[(t, n)] = (2 * nnz + 1 + (2 if inexact else 0), nnz, inexact)
    return out


# (tile, matrix) -> (c, nnz it came from, whether a coefficient is not an fp32 number)
OPS = _ops()


def beta_exact(tile, which):
    """(max row sum of |C|)^2 of the exact matrix: the least bound of
    max|C X C^T| / max|X| (which 0: Bt, 1: A, 2: G)."""
    M = _frac_mat(tile, ("Bt", "A", "G")[which])
    return max(sum(abs(v) for v in r) for r in M) ** 2


# ---- geometry ---------------------------------------------------------------------
def tiles_hw(H_, W_, tile):
    return (H_ + tile - 1) // tile, (W_ + tile - 1) // tile


def patches(x, tile):
    """[B, C, H, W] -> [B, C, TH, TW, alpha, alpha]: the windows at (m ty - 1,
    m tx - 1), zero outside the image."""
    B, C, H_, W_ = x.shape
    TH, TW = tiles_hw(H_, W_, tile)
    xp = F.pad(x, (1, TW * tile + 1 - W_, 1, TH * tile + 1 - H_))
    return xp.unfold(2, tile + 2, tile).unfold(3, tile + 2, tile)


def inner(p):
    """The m x m tile inside an alpha x alpha window."""
    return p[..., 1:-1, 1:-1]


def two_pass(X, C):
    return torch.einsum("ia,...ab,jb->...ij", C, X, C)


def to_planes(Y):
    """[B, C, TH, TW, a, a] -> [a a][T][C] (the kernels' V / dM / M layout)."""
    B, C = Y.shape[:2]
    a2 = Y.shape[-1] * Y.shape[-2]
    return Y.permute(4, 5, 0, 2, 3, 1).reshape(a2, -1, C)


def from_planes(Mp, B, TH, TW):
    """[a a][T][C] -> [B, C, TH, TW, a, a]."""
    a2, T, C = Mp.shape
    a = int(round(a2 ** 0.5))
    return Mp.reshape(a, a, B, TH, TW, C).permute(2, 5, 3, 4, 0, 1)


def transform_ref(X, tile, name, extra_ops=0):
    """(ref, bound) in plane layout of Y = C X C^T for windows X [..., n, n]
    (float64); extra_ops: fp32 operations that formed X's elements, relative
    to |X|, carried through |C| . |C|^T."""
    C = cmat(tile, name, X.device)
    ref = to_planes(two_pass(X, C))
    absr = to_planes(two_pass(X.abs(), C.abs()))
    return ref, (OPS[(tile, name)][0] + extra_ops) * E32 * absr


def input_ref(x, tile, src=None):
    """V = Bt d B of NCHW x (float64 from fp32 values); src = (wy, wx): x is
    resampled first (f16_util.resize_mats). Returns (ref, bound, d)."""
    x = x.double()
    extra = 0
    if src is not None:
        wy, wx = (m.to(x.device) for m in src)
        xa = H.resample(x, wy, wx, absval=True)
        x = H.resample(x, wy, wx)
        extra = H.OPS["resize"]
        C = cmat(tile, "Bt", x.device)
        ref = to_planes(two_pass(patches(x, tile), C))
        absr = to_planes(two_pass(patches(xa, tile), C.abs()))
        return ref, (OPS[(tile, "Bt")][0] + extra) * E32 * absr, x
    ref, b = transform_ref(patches(x, tile), tile, "Bt")
    return ref, b, x


def dm_ref(dy, tile):
    """dM = A dY A^T of the m x m tiles (zero past the image)."""
    return transform_ref(inner(patches(dy.double(), tile)), tile, "A")


def windows_ref(X, Xb, tile, name):
    """(ref, bound) of Y = C X C^T where the fp32 windows the kernel
    transforms are within Xb of X: Xb carried through |C| . |C|^T, and the
    transform's own roundings on |X| + Xb."""
    C = cmat(tile, name, X.device)
    prop = to_planes(two_pass(Xb, C.abs()))
    absr = to_planes(two_pass(X.abs(), C.abs())) + prop
    return to_planes(two_pass(X, C)), prop + OPS[(tile, name)][0] * E32 * absr


def dual_ref(dy, tile, dyb=None):
    """(V ref, V bound, dM ref, dM bound) of the dual transform of NCHW dy
    (float64); dyb: the element-wise bound of the dy the kernel forms."""
    p = patches(dy.double(), tile)
    if dyb is None:
        return transform_ref(p, tile, "Bt") + transform_ref(inner(p), tile, "A")
    pb = patches(dyb, tile)
    return windows_ref(p, pb, tile, "Bt") + windows_ref(inner(p), inner(pb), tile, "A")


def bn_dy_ref(g, y, scale, shift, mean, coef, mask, slope=H.SLOPE):
    """float64 (dy, bound) of the deferred BN backward the fused dual
    transforms form per element, NCHW g, y; scale / shift / mean [C], coef
    [3][C] = {k1, k2, k3}, mask [B][C] or None, all fp32 values taken exactly:
        dz = g lrelu'(y scale + shift) mask,  dy = k1 dz + k2 (y - mean) + k3
        bound = OPS["bn_bwd_apply"] e32 (|k1 dz| + |k2 (y - mean)| + |k3|)
                + (1 - slope) |k1 g mask|  where the fp32 pre-activation lies
                  within its own error (4 e32 (|y scale| + |shift|)) of 0."""
    v = (1, -1, 1, 1)
    g, y = g.double(), y.double()
    k1, k2, k3 = (coef.double()[i].view(v) for i in range(3))
    m = 1.0 if mask is None else mask.double()[:, :, None, None]
    t = y * scale.double().view(v)
    z = t + shift.double().view(v)
    unsure = z.abs() <= 4 * E32 * (t.abs() + shift.double().abs().view(v))
    dz = g * torch.where(z > 0, 1.0, slope) * m
    t1, t2 = k1 * dz, k2 * (y - mean.double().view(v))
    bound = H.OPS["bn_bwd_apply"] * E32 * (t1.abs() + t2.abs() + k3.abs())
    bound = bound + torch.where(unsure, (1 - slope) * (k1 * g * m).abs(), torch.zeros_like(bound))
    return t1 + t2 + k3, bound


def filter_ref(w, tile, flip, n_p, k_p):
    """U [a a][n_p][k_p] = G g G^T (flip: g rotated 180 deg, n = ci, k = co),
    exact zeros in the padding."""
    g = w.double()
    if flip:
        g = g.flip(2, 3).transpose(0, 1)
    n, k = g.shape[:2]
    G = cmat(tile, "G", w.device)
    a2 = (tile + 2) ** 2
    ref = torch.zeros(a2, n_p, k_p, dtype=torch.float64, device=w.device)
    ab = torch.zeros_like(ref)
    ref[:, :n, :k] = two_pass(g, G).permute(2, 3, 0, 1).reshape(a2, n, k)
    ab[:, :n, :k] = two_pass(g.abs(), G.abs()).permute(2, 3, 0, 1).reshape(a2, n, k)
    return ref, OPS[(tile, "G")][0] * E32 * ab


def output_ref(Mp, bias, B, H_, W_, tile):
    """y NCHW = A^T M A + b cropped to H x W, from M [a a][T][N] (float64 of
    fp32 values). The bias add is one more rounding on |o| + |b|."""
    TH, TW = tiles_hw(H_, W_, tile)
    X = from_planes(Mp.double(), B, TH, TW)
    At = cmat(tile, "At", Mp.device)
    o = two_pass(X, At)
    oa = two_pass(X.abs(), At.abs())

    def img(t):
        Bn, N = t.shape[:2]
        return t.permute(0, 1, 2, 4, 3, 5).reshape(Bn, N, TH * tile, TW * tile)[:, :, :H_, :W_]
    ref, ab = img(o), img(oa)
    c = OPS[(tile, "At")][0]
    if bias is not None:
        bb = bias.double().view(1, -1, 1, 1)
        ref, ab, c = ref + bb, ab + bb.abs(), c + 1
    return ref, c * E32 * ab


# ---- h2 storage ---------------------------------------------------------------------
def h2_exp(slot, beta):
    """Host mirror of h2_exp / pow2_scale_exp for a slot holding `slot`."""
    m = np.float32(slot)
    with np.errstate(over="ignore"):
        b = np.float32(m * np.float32(beta))
    if np.isfinite(m) and not np.isfinite(b):
        b = np.finfo(np.float32).max
    u = int(np.array(b, dtype=np.float32).view(np.uint32)) & 0x7fffffff
    if u == 0 or u >= 0x7f800000:
        return 0
    e = (u >> 23) - 127
    if u & 0x7fffff:
        e += 1
    return max(-126, min(126, 15 - e))


def h2_P(slot, beta):
    """P = 2^15 / s: pow2_up(float32(slot) float32(beta)) with h2_exp's saturation."""
    return 2.0 ** (15 - h2_exp(slot, beta))


def h2_decode(t, rows, C, slot, beta):
    """float64 [rows][C] of an h2 tensor (fp16 [rows][2C]: per 8-channel chunk
    h at 16j..16j+7, l at 16j+8..16j+15), exponent from (slot, beta)."""
    v = t.reshape(rows, C // 8, 2, 8).double()
    return (v[:, :, 0, :] + v[:, :, 1, :]).reshape(rows, C) * 2.0 ** (-h2_exp(slot, beta))


def h2_decode_h(t, rows, C, slot, beta):
    """The h plane alone, decoded."""
    v = t.reshape(rows, C // 8, 2, 8).double()
    return v[:, :, 0, :].reshape(rows, C) * 2.0 ** (-h2_exp(slot, beta))


def h2_h_bound(ref, tbound, slot, beta):
    """Bound of the decoded h plane against ref (round to nearest of v s)."""
    return tbound * (1 + H.U["f16"]) + H.U["f16"] * ref.abs() + FLOOR * h2_P(slot, beta)


def h2_ratio(t, ref, tbound, slot, beta):
    """Worst ratio of an h2 tensor [rows][2C] against ref [rows][C] over both
    storage bounds (h + l, and h alone)."""
    rows, C = ref.shape
    return max(H.ratio(h2_decode(t, rows, C, slot, beta), ref, h2_bound(ref, tbound, slot, beta)),
               H.ratio(h2_decode_h(t, rows, C, slot, beta), ref, h2_h_bound(ref, tbound, slot, beta)))


def h2_bound(ref, tbound, slot, beta):
    """Bound of a decoded h2 operand against ref, the stored fp32 value being
    within tbound of ref."""
    return tbound * (1 + REP) + REP * ref.abs() + FLOOR * h2_P(slot, beta)


def slot_value(slot):
    """The maximum held by an operand-maximum slot (fp32 bits as uint32 words)."""
    v = slot.view(torch.int32).cpu().numpy().astype(np.uint32).max()
    return float(np.array(v, dtype=np.uint32).view(np.float32))


def tiny_share(ref, P, rel=S.TINY_REL):
    """Share of ref's non-zero elements below rel (2^-17: where l turns
    subnormal) of P; P a number or a tensor broadcast against ref."""
    a = ref.abs()
    nz = a > 0
    return ((a < rel * P) & nz).double().sum().item() / max(1, int(nz.sum()))


# ---- GEMM stages ----------------------------------------------------------------------
def gemm_ref(V, U, mv, mu):
    """M[c] = V[c] U[c]^T of fp32 V [nb][T][K], U [nb][N][K]; mv / mu: the
    operand maxima the scales come from (slot times beta, fp32 product).
    Returns (ref, bound)."""
    Vd, Ud = V.double(), U.double()
    K = V.shape[-1]
    ref = Vd @ Ud.transpose(1, 2)
    Sa = Vd.abs() @ Ud.abs().transpose(1, 2)
    a_ones = Vd.abs().sum(-1, keepdim=True)                  # [nb][T][1]
    ones_b = Ud.abs().sum(-1).unsqueeze(1)                   # [nb][1][N]
    fl = S.floor_term(mv, mu, a_ones, ones_b, K)
    return ref, S.gemm_bound(2, Sa, K, floor=fl)


def wgrad_ref(dM, V, tile, cout, cin, mdm, mv):
    """dw [cout][cin][3][3] = G^T (sum_t dM[c]^T V[c]) G from fp32 dM [nb][T][M],
    V [nb][T][N]. Returns (ref, bound)."""
    a = tile + 2
    D, X = dM.double(), V.double()
    T = D.shape[1]
    dU = D.transpose(1, 2) @ X                                # [nb][M][N]
    Sa = D.abs().transpose(1, 2) @ X.abs()
    a_ones = D.abs().sum(1).unsqueeze(2)                     # [nb][M][1]
    ones_b = X.abs().sum(1).unsqueeze(1)                     # [nb][1][N]
    gb = S.wgrad_bound(2, Sa, T, floor=S.floor_term(mdm, mv, a_ones, ones_b, T))
    Gt = cmat(tile, "Gt", dM.device)

    def win(t):
        return t[:, :cout, :cin].reshape(a, a, cout, cin).permute(2, 3, 0, 1)
    ref = two_pass(win(dU), Gt)
    ab = two_pass(win(dU).abs() + win(gb), Gt.abs())
    return ref, two_pass(win(gb), Gt.abs()) + OPS[(tile, "Gt")][0] * E32 * ab


# ---- case makers ------------------------------------------------------------------------
def make_calib(B, H_, W_, C, seed=0):
    """Calibrated-looking: randn with per-channel magnitudes 2^U(-2, 2), NCHW fp32."""
    g = H.gen(seed, B, H_, W_, C, 11)
    mag = torch.pow(2.0, torch.rand(1, C, 1, 1, generator=g) * 4 - 2)
    return torch.randn(B, C, H_, W_, generator=g) * mag


def make_spread(B, H_, W_, C, seed=0):
    """f32_util.make_spread_case's activation: per-channel and per-image-row
    magnitudes 2^U(-12, 0), and in every other band of three rows a pixel
    keeps one channel ((h + w) % C)."""
    g = H.gen(seed, B, H_, W_, C, 12)
    x = (torch.randn(B, C, H_, W_, generator=g) * S.spread(g, C).view(1, C, 1, 1)
         * S.spread(g, H_).view(1, 1, H_, 1))
    hh, ww = torch.arange(H_).view(H_, 1), torch.arange(W_).view(1, W_)
    lone = ((hh // 3) % 2 == 1).expand(H_, W_)
    keep = torch.arange(C).view(C, 1, 1) == ((hh + ww) % C).view(1, H_, W_)
    return torch.where(lone.view(1, 1, H_, W_) & ~keep.view(1, C, H_, W_), torch.zeros(()), x)


def make_filters(co, ci, seed=0, spread=True):
    g = H.gen(seed, co, ci, 13)
    w = torch.randn(co, ci, 3, 3, generator=g) / (9 * ci) ** 0.5
    if spread:
        w = w * S.spread(g, co).view(co, 1, 1, 1) * S.spread(g, ci).view(1, ci, 1, 1)
    return w


def make_planes(nb, rows, C, seed=0, spread=False, lo=-3, hi=3):
    """A Winograd-domain operand [nb][rows][C]: randn with per-component
    magnitudes 2^U(lo, hi); spread: per-channel and per-row 2^U(-12, 0) on top."""
    g = H.gen(seed, nb, rows, C, 14)
    t = torch.randn(nb, rows, C, generator=g) * S.spread(g, nb, lo, hi).view(nb, 1, 1)
    if spread:
        t = t * S.spread(g, C).view(1, 1, C) * S.spread(g, rows).view(1, rows, 1)
    return t


def nhwc(x, ld=None):
    """NCHW -> [B H W][C] rows; ld > C: a strided view of a wider NaN-free buffer."""
    B, C, H_, W_ = x.shape
    r = x.permute(0, 2, 3, 1).reshape(B * H_ * W_, C)
    if ld is None or ld == C:
        return r.contiguous()
    buf = torch.full((B * H_ * W_, ld), 7.0, dtype=x.dtype, device=x.device)
    buf[:, :C] = r
    return buf[:, :C]


def beta_pattern(tile, which):
    """(s, n): the sign row of the matrix's largest absolute row sum; an n x n
    input m s s^T gives one output of (row sum)^2 m."""
    M = _frac_mat(tile, ("Bt", "A", "G")[which])
    r = max(M, key=lambda row: sum(abs(v) for v in row))
    return torch.tensor([float((v > 0) - (v < 0)) for v in r]), len(r)


# ---- the stand-in: numpy emulation of the kernels' operation sequence -------------------
f32 = np.float32


def _fma(c, x, a):
    return (np.float64(c) * x.astype(np.float64) + a.astype(np.float64)).astype(np.float32)


def emu_wmat(C32, x):
    """y[..., i] = sum_j C(i, j) x[..., j] in wmat's order: the first product,
    then + / - / fma per non-zero coefficient, fp32 throughout."""
    out = []
    for i in range(C32.shape[0]):
        acc = None
        for j in range(C32.shape[1]):
            c = C32[i, j]
            if c == 0:
                continue
            xj = x[..., j]
            if acc is None:
                acc = xj.copy() if c == 1 else (-xj if c == -1 else (c * xj).astype(f32))
            elif c == 1:
                acc = (acc + xj).astype(f32)
            elif c == -1:
                acc = (acc - xj).astype(f32)
            else:
                acc = _fma(c, xj, acc)
        out.append(acc if acc is not None else np.zeros(x.shape[:-1], f32))
    return np.stack(out, -1)


def emu_wmat2(C32, X):
    """Y = C X C^T as wmat2: the column pass, then the row pass."""
    s = np.swapaxes(emu_wmat(C32, np.swapaxes(X, -1, -2)), -1, -2)
    return emu_wmat(C32, s)


def emu_transform(X, tile, name, C32=None):
    """torch [..., n, n] float32 windows -> plane layout float32."""
    C32 = cmat32(tile, name) if C32 is None else C32
    return to_planes(torch.from_numpy(emu_wmat2(C32, X.contiguous().numpy().astype(f32))))


def emu_h2(v, slot, beta, drop_l=False, trunc=False, exp_off=0, swap_chunks=False):
    """fp32 [rows][C] -> h2 [rows][2C] fp16 as split4h writes it. Mutants:
    drop_l (the l plane zero), trunc (h rounded toward zero), exp_off (the
    producer's scale exponent off by that much), swap_chunks (chunk 0 of
    every row swapped with chunk 1)."""
    rows, C = v.shape
    xs = (v.double() * 2.0 ** (h2_exp(slot, beta) + exp_off)).float()
    h = H.toward_zero_f16(xs) if trunc else xs.half()
    l = (xs - h.float()).half()
    if drop_l:
        l = torch.zeros_like(l)
    out = torch.stack((h.view(rows, C // 8, 8), l.view(rows, C // 8, 8)), 2)
    if swap_chunks:
        out = torch.cat((out[:, 1:2], out[:, 0:1], out[:, 2:]), 1)
    return out.reshape(rows, 2 * C)


def emu_gemm_h2(Vh, Uh, K, ev, eu, drop_hl=False):
    """One component's GEMM on h2 rows [T][2K], [N][2K]: h h + h l + l h in
    fp32, the scales undone. drop_hl: the h(V) l(U) product left out."""
    def planes(t):
        v = t.reshape(t.shape[0], K // 8, 2, 8).float()
        return v[:, :, 0].reshape(-1, K), v[:, :, 1].reshape(-1, K)
    (vh, vl), (uh, ul) = planes(Vh), planes(Uh)
    acc = S._mm32(vl, uh) + S._mm32(vh, uh)
    if not drop_hl:
        acc = acc + S._mm32(vh, ul)
    return ((acc.double() * 2.0 ** -ev) * 2.0 ** -eu).float()


def emu_split_sum(dM, V, splits, drop_last=False):
    """dU[c] = sum over `splits` K slabs of dM[c]^T V[c], each slab and the sum
    in fp32. drop_last: the last slab left out."""
    T = dM.shape[1]
    kc = (T + splits - 1) // splits
    acc = None
    n = splits - 1 if drop_last else splits
    for s in range(n):
        a, b = dM[:, s * kc:(s + 1) * kc], V[:, s * kc:(s + 1) * kc]
        part = torch.from_numpy(np.matmul(a.numpy().astype(f32).transpose(0, 2, 1), b.numpy().astype(f32)))
        acc = part if acc is None else acc + part
    return acc


# ---- the chained convolution: stage bounds carried through the later stages --------------
def _mv(slot, beta):
    with np.errstate(over="ignore"):
        return float(np.float32(slot) * np.float32(beta))


def chain_gemm(Vr, eV, Ur, eU, mv, mu):
    """(M ref, M bound) of M[c] = V[c] U[c]^T where the fp32 operands the h2
    tensors hold are within eV / eU of Vr / Ur: the operand errors through the
    other operand's absolute values, then the GEMM's own bound on the
    magnitudes it really sees."""
    Va, Ua = Vr.abs() + eV, Ur.abs() + eU
    K = Vr.shape[-1]
    prop = Va @ eU.transpose(1, 2) + eV @ Ur.abs().transpose(1, 2)
    fl = S.floor_term(mv, mu, Va.sum(-1, keepdim=True), Ua.sum(-1).unsqueeze(1), K)
    return Vr @ Ur.transpose(1, 2), prop + S.gemm_bound(2, Va @ Ua.transpose(1, 2), K, floor=fl)


def chain_output(Mr, eM, bias, B, H_, W_, tile):
    """(y ref, y bound) NCHW of At M A + b with M within eM of Mr."""
    ref, b0 = output_ref(Mr, bias, B, H_, W_, tile)
    b1 = output_ref(eM, None, B, H_, W_, tile)[1]            # c e32 |At| eM |A|
    return ref, b1 / (OPS[(tile, "At")][0] * E32) + b0 + b1


def chain_wgrad(Dr, eD, Vr, eV, tile, cout, cin, mdm, mv):
    """(dw ref, dw bound) of G^T (sum_t dM^T V) G with dM, V within eD, eV."""
    a = tile + 2
    Da, Va = Dr.abs() + eD, Vr.abs() + eV
    T = Dr.shape[1]
    prop = Da.transpose(1, 2) @ eV + eD.transpose(1, 2) @ Vr.abs()
    fl = S.floor_term(mdm, mv, Da.sum(1).unsqueeze(2), Va.sum(1).unsqueeze(1), T)
    gb = prop + S.wgrad_bound(2, Da.transpose(1, 2) @ Va, T, floor=fl)
    dU = Dr.transpose(1, 2) @ Vr
    Gt = cmat(tile, "Gt", Dr.device)

    def win(t):
        return t[:, :cout, :cin].reshape(a, a, cout, cin).permute(2, 3, 0, 1)
    ab = two_pass(win(dU).abs() + win(gb), Gt.abs())
    return two_pass(win(dU), Gt), two_pass(win(gb), Gt.abs()) + OPS[(tile, "Gt")][0] * E32 * ab
