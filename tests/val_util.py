"""The yardstick of the validation tests: the six fields of an image's record
{count, sum|d|, sum d^2, max|d|, nonfinite, out_of_range}, l1, mse and psnr in
numpy float64 over the float32 samples, and a restatement of the averaging of
the reference's validate_direct (main.py:624-642).

Every summed term is >= 0, so any summation order lies within n * 2^-53 relative
of the exact sum; for n < 2^17 that is below BOUND, the project's 1e-10
(stats_util.py)."""
import math

import numpy as np

BOUND = 1e-10
COUNT, S1, S2, MAX, BAD, OOR = range(6)


def records(o, t, lo=0.0, hi=1.0):
    """[B, 6] float64: the record of every image of o against t ([B, ...] float32).
    A pair with a non-finite sample counts in `nonfinite` and nowhere else;
    `out_of_range` counts the o of the other pairs outside [lo, hi]."""
    o, t = np.asarray(o), np.asarray(t)
    assert o.dtype == t.dtype == np.float32 and o.shape == t.shape
    B = o.shape[0]
    o, t = o.reshape(B, -1), t.reshape(B, -1)
    fin = np.isfinite(o) & np.isfinite(t)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(fin, np.abs(o.astype(np.float64) - t.astype(np.float64)), 0.0)
    out = np.zeros((B, 6), dtype=np.float64)
    out[:, COUNT] = fin.sum(axis=1)
    out[:, S1] = d.sum(axis=1)
    out[:, S2] = (d * d).sum(axis=1)
    out[:, MAX] = d.max(axis=1)
    out[:, BAD] = (~fin).sum(axis=1)
    with np.errstate(invalid="ignore"):
        out[:, OOR] = (fin & ((o < np.float32(lo)) | (o > np.float32(hi)))).sum(axis=1)
    return out


def fold(recs):
    """One record of several (images of a batch, batches of a set)."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 6)
    out = recs.sum(axis=0)
    out[MAX] = recs[:, MAX].max() if len(recs) else 0.0
    return out


def psnr(mse):
    """validate_consistency.py:120: 20 * log10(1 / sqrt(mse)); inf at mse == 0."""
    if math.isnan(mse):
        return float("nan")
    return float("inf") if mse == 0 else 20.0 * math.log10(1.0 / math.sqrt(mse))


def figures(rec):
    """dict of count, l1, mse, psnr, max_abs, nonfinite, out_of_range of one record
    (l1, mse and psnr NaN at count == 0)."""
    n = rec[COUNT]
    l1 = rec[S1] / n if n > 0 else float("nan")
    mse = rec[S2] / n if n > 0 else float("nan")
    return {"count": int(n), "l1": l1, "mse": mse, "psnr": psnr(mse), "max_abs": float(rec[MAX]),
            "nonfinite": int(rec[BAD]), "out_of_range": int(rec[OOR])}


def rel(got, ref):
    """|got - ref| relative to |ref| (absolute where ref == 0)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.where(ref == 0, 1.0, np.abs(ref))


def validate_direct_means(totals, l1s, perts=None):
    """main.py:624-642: the per-batch `.item()` values summed in loop order from
    0.0 and divided by the batch count; inf without a batch (the perturbation
    figure: 0.0, main.py:655)."""
    val_loss = val_l1 = val_pert = 0.0
    count = 0
    for i, v in enumerate(totals):
        val_loss += v
        val_l1 += l1s[i]
        if perts is not None:
            val_pert += perts[i]
        count += 1
    inf = float("inf")
    return {"loss": val_loss / count if count else inf,
            "l1_loss": val_l1 / count if count else inf,
            "perturbation_loss": val_pert / count if count else 0.0,
            "batches": count}
