"""float64 reference of the learned feature extraction (nsm_amd/extract.py,
csrc/nsm_extract.hip): forward, the five gradients, and for every output entry
the number n of terms that make it up and the sum S of their absolute values.

A result computed in fp32 by ANY order of fused or unfused multiply-adds over
those terms differs from the exact one by at most gamma_d S, d the number of
roundings a term passes through (Higham, Accuracy and Stability, §3.1), and
gamma_d <= (d + 2) 2^-24 for d 2^-24 << 1. The terms are the fully expanded
ones, so a quantity that enters a sum already rounded is covered:

  y[c]       = b2[c] + sum_j w2[c][j] h[j]; chain length K = Hd. The first
               layer's error, (Cin + 2) 2^-24 S_pre[j] (its own chain, plus the
               LeakyReLU's multiply, |slope| <= 1), is propagated through |w2|.
  dx[i]      = sum_j sum_c w1[j][i] m[j] w2[c][j] dy[c]             n = Hd Cout
  db1[j]     = sum_p sum_c m[p][j] w2[c][j] dy[p][c]                n = N Cout
  dw1[j][i]  = sum_p sum_c m[p][j] w2[c][j] dy[p][c] x[p][i]        n = N Cout
  db2[c]     = sum_p dy[p][c]                                       n = N
  dw2[c][j]  = sum_p dy[p][c] m[p][j] (b1[j] + sum_i w1[j][i] x[p][i])   n = N (Cin + 1)

with N = B H W pixels and m = 1 where pre > 0, slope elsewhere. d <= n in each
(every chain is no longer than its term count), so the bound is (n + 2) 2^-24 S.
The mask m is a step: the bounds hold where the fp32 and the exact pre agree in
sign, which gaussian_case guarantees by construction (no |pre| within 2^-10 of
S_pre of zero: 2^14 times the chain's bound) and integer_case by exactness.
"""
import numpy as np

U24 = 2.0 ** -24


class Ref:
    pass


def reference(x, dy, w1, b1, w2, b2, slope, sums=True):
    """x [B,Cin,H,W], dy [B,Cout,H,W], w1 [Hd,Cin], b1 [Hd], w2 [Cout,Hd], b2 [Cout]:
    a Ref with pre, h, y, dh, dx, dw1, db1, dw2, db2 (float64) and, with sums,
    bound_<name> for y and the five gradients."""
    x, dy, w1, b1, w2, b2 = (np.asarray(a, dtype=np.float64) for a in (x, dy, w1, b1, w2, b2))
    slope = float(slope)
    B, Cin, H, W = x.shape
    Hd, Cout = w1.shape[0], w2.shape[0]
    N = B * H * W
    X = x.transpose(0, 2, 3, 1).reshape(N, Cin)          # [N, Cin]
    DY = dy.transpose(0, 2, 3, 1).reshape(N, Cout)
    r = Ref()
    pre = X @ w1.T + b1                                   # [N, Hd]
    m = np.where(pre > 0, 1.0, slope)
    h = np.where(pre > 0, pre, pre * slope)
    y = h @ w2.T + b2
    g = DY @ w2                                           # [N, Hd]
    dh = m * g
    r.pre, r.h, r.dh, r.g = pre, h, dh, g
    r.dx_flat = dh @ w1
    r.dw1, r.db1 = dh.T @ X, dh.sum(0)
    r.dw2, r.db2 = DY.T @ h, DY.sum(0)

    def planes(a, C):
        return np.ascontiguousarray(a.reshape(B, H, W, C).transpose(0, 3, 1, 2))
    r.y, r.dx = planes(y, Cout), planes(r.dx_flat, Cin)
    if not sums:
        return r
    aX, aDY, aw1, aw2, am = np.abs(X), np.abs(DY), np.abs(w1), np.abs(w2), np.abs(m)
    S_pre = aX @ aw1.T + np.abs(b1)                       # [N, Hd]
    r.S_pre = S_pre
    S_y = np.abs(h) @ aw2.T + np.abs(b2)
    err_h = (Cin + 2) * U24 * S_pre
    r.bound_y = planes((Hd + 2) * U24 * S_y + err_h @ aw2.T, Cout)
    S_dh = am * (aDY @ aw2)                               # [N, Hd]: sum_c |m w2 dy|
    r.bound_dx = planes((Hd * Cout + 2) * U24 * (S_dh @ aw1), Cin)
    r.bound_db1 = (N * Cout + 2) * U24 * S_dh.sum(0)
    r.bound_dw1 = (N * Cout + 2) * U24 * (S_dh.T @ aX)
    r.bound_db2 = (N + 2) * U24 * aDY.sum(0)
    r.bound_dw2 = (N * (Cin + 1) + 2) * U24 * (aDY.T @ (am * S_pre))
    return r


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def gaussian_case(shape, Cin, Hd, Cout, seed, slope=0.2):
    """(x, dy, w1, b1, w2, b2, slope), fp32 arrays of standard normal inputs and
    Conv2d-scaled weights for shape = (B, H, W). A pixel whose pre comes within
    2^-10 S_pre of zero in some hidden unit is drawn again, so that the mask of
    the fp32 chain (error <= (Cin + 2) 2^-24 S_pre) is the exact one."""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    w1 = _f32(rng.standard_normal((Hd, Cin)) / np.sqrt(Cin))
    b1 = _f32(rng.standard_normal(Hd) * 0.5)
    w2 = _f32(rng.standard_normal((Cout, Hd)) / np.sqrt(Hd))
    b2 = _f32(rng.standard_normal(Cout) * 0.5)
    N = B * H * W
    X = _f32(rng.standard_normal((N, Cin)))
    for _ in range(100):
        X64 = X.astype(np.float64)
        pre = X64 @ w1.astype(np.float64).T + b1
        S = np.abs(X64) @ np.abs(w1.astype(np.float64)).T + np.abs(b1)
        bad = (np.abs(pre) < S * 2.0 ** -10).any(1)
        if not bad.any():
            break
        X[bad] = _f32(rng.standard_normal((int(bad.sum()), Cin)))
    else:
        raise AssertionError("gaussian_case: could not separate pre from zero")
    x = np.ascontiguousarray(X.reshape(B, H, W, Cin).transpose(0, 3, 1, 2))
    dy = _f32(rng.standard_normal((B, Cout, H, W)))
    return x, dy, w1, b1, w2, b2, slope


def integer_case(shape, Cin, Hd, Cout, seed):
    """x in {-2..2}, w1, w2, b1, b2 in {-1,0,1}, dy in {-1,0,1,2}, slope 0.25:
    every intermediate is a small multiple of 1/4, so every fp32 evaluation
    order is exact (test_extract_ref asserts it on the reference) and pre == 0
    is frequent."""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    x = _f32(rng.integers(-2, 3, (B, Cin, H, W)))
    w1 = _f32(rng.integers(-1, 2, (Hd, Cin)))
    b1 = _f32(rng.integers(-1, 2, Hd))
    w2 = _f32(rng.integers(-1, 2, (Cout, Hd)))
    b2 = _f32(rng.integers(-1, 2, Cout))
    dy = _f32(rng.integers(-1, 3, (B, Cout, H, W)))
    return x, dy, w1, b1, w2, b2, 0.25


def same_bits(got, want):
    """got (fp32) equals want bit for bit; want + 0.0 first: the reference's
    matrix products may give -0.0 where every chain that starts from +0.0 gives
    +0.0 (x + (-x) and (+0) + (-0) are +0 in round-to-nearest)."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(np.asarray(want, dtype=np.float64) + 0.0).astype(np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


GRADS = ("dx", "dw1", "db1", "dw2", "db2")
# (B, H, W), Cin, Hd, Cout of the GPU tests' fixed shapes
SHAPES = {
    "w73": ((2, 41, 73), 15, 16, 4),     # three of four rows start off the 16-byte grid
    "w72": ((2, 41, 72), 15, 16, 4),
    "tiny": ((1, 5, 3), 11, 7, 3),       # fewer pixels than a block, odd channel counts
}
