"""The fused perturbation loss (nsm_pert_loss_fwd / nsm_pert_loss_bwd) restated
in numpy fp64, and the input makers the GPU tests share.

The kernels take alpha and w as C floats, so the restatement rounds both to
fp32 first and does everything else in double: the expression the device
evaluates, at a precision where its own rounding does not show."""
import numpy as np

U = 2.0 ** -24    # unit roundoff of fp32


def _f64(a):
    return np.asarray(a, dtype=np.float64).ravel()


def pert_loss_ref(o, t, pouts, alpha, w, vgg=0.0):
    """The record of nsm_pert_loss_fwd in fp64: a dict with l1 = mean|o - t|,
    means[i] = mean|o - p_i|, pert = their mean, and
    total = alpha*l1 + (1 - alpha)*vgg + w*pert."""
    a, w_ = float(np.float32(alpha)), float(np.float32(w))
    o_, t_ = _f64(o), _f64(t)
    means = [float(np.abs(o_ - _f64(p)).mean()) for p in pouts]
    l1 = float(np.abs(o_ - t_).mean())
    pert = float(sum(means) / len(means))
    return {"l1": l1, "pert": pert, "means": means,
            "total": a * l1 + (1.0 - a) * float(vgg) + w_ * pert}


def pert_grad_ref(o, t, pouts, alpha, w, gscale=1.0):
    """d total / d o of the record above, times gscale, in fp64:
    gscale * (alpha/n * sgn(o - t) + w/(P n) * sum_i sgn(o - p_i)), sgn(0) = 0."""
    a, w_ = float(np.float32(alpha)), float(np.float32(w))
    o_, t_ = _f64(o), _f64(t)
    n, P = o_.size, len(pouts)
    s = np.zeros(n)
    for p in pouts:
        s += np.sign(o_ - _f64(p))
    return float(gscale) * ((a / n) * np.sign(o_ - t_) + (w_ / (P * n)) * s)


def grad_bound(n, P, alpha, w, gscale=1.0):
    """4 * 2^-24 * |gscale| * (c0 + P*c1): the two coefficients' roundings to
    fp32, the product c1 * count, the sum of the two terms and the product with
    gscale, on two terms that may cancel."""
    return 4 * U * abs(float(gscale)) * (float(alpha) / n + P * float(w) / (P * n))


def fwd_bound(n):
    """(ceil(log2 n) + 2) * 2^-24, relative: a pairwise fp32 sum of non-negative
    terms (one rounding per level), the rounding of each |o - x| and the final
    rounding to fp32."""
    return (int(np.ceil(np.log2(n))) + 2) * U


def all_tie(n):
    """Positions where every operand equals o (none below 16 elements)."""
    idx = np.arange(n)
    return (idx % 16 == 0) & (n > 16)


def make_operands(n, P, seed=0):
    """o, t, [p_1..p_P] as fp32 vectors with exact ties planted: an eighth of
    p_1 equals o, an eighth of t equals o, and on a sixteenth every operand
    equals o (all signs 0). Lengths up to 16 have no ties."""
    rng = np.random.default_rng([11, n, P, seed])
    o = rng.random(n, dtype=np.float32)
    t = rng.random(n, dtype=np.float32)
    ps = [(o + 0.02 * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
          for _ in range(P)]
    if n > 16:
        idx = np.arange(n)
        ps[0][idx % 8 == 0] = o[idx % 8 == 0]
        mt = (idx % 16 == 0) | (idx % 16 == 4)
        t[mt] = o[mt]
        z = all_tie(n)
        for p in ps[1:]:
            p[z] = o[z]
    return o, t, ps
