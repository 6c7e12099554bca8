"""The yardstick of the channel-statistics tests: an exact two-pass in float64
over the float32 samples (subtract the fp64 mean, square, average), the error
measures of the 1e-10 bound, and the fixture tests/golden/dataset_stats.npz
(make_golden_stats.py)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_stats.npz")
BOUND = 1e-10                       # mean and sigma against the yardstick
TINY = np.finfo(np.float64).tiny    # sigma = 0 must come out as exactly 0
DEPTH, SMALL, CONST, UNIFORM = 3, 4, 5, 6   # channels of the fixture (0-2: unit normals)


def two_pass(x, axes=(0, 2, 3)):
    """Per channel of x [N,C,H,W] (float32) over its finite samples, reduced over
    `axes`: dict of count, mean, std (population), min, max, nonfinite. A channel
    without a finite sample gets mean 0, std 0, min +inf, max -inf."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4
    fin = np.isfinite(x)
    xd = np.where(fin, x, 0).astype(np.float64)
    n = fin.sum(axis=axes)
    nn = np.maximum(n, 1).astype(np.float64)
    mean = xd.sum(axis=axes) / nn
    dev = np.where(fin, xd - np.expand_dims(mean, axes), 0.0)
    var = (dev * dev).sum(axis=axes) / nn
    return {"count": n, "mean": mean, "std": np.sqrt(var),
            "min": np.where(fin, x, np.inf).min(axis=axes).astype(np.float32),
            "max": np.where(fin, x, -np.inf).max(axis=axes).astype(np.float32),
            "nonfinite": (~fin).sum(axis=axes)}


def per_frame(x):
    """two_pass of every frame on its own: arrays [N,C]."""
    return two_pass(x, axes=(2, 3))


def naive_one_pass(x):
    """The cancelling form: sum x and sum x^2 about zero, in float64."""
    xd = np.asarray(x).astype(np.float64)
    n = xd.shape[0] * xd.shape[2] * xd.shape[3]
    s, s2 = xd.sum(axis=(0, 2, 3)), (xd * xd).sum(axis=(0, 2, 3))
    mean = s / n
    return mean, np.sqrt(np.maximum(s2 / n - mean * mean, 0.0))


def mean_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)


def std_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.maximum(ref, TINY)


def load_fixture():
    """inputs [5,7,10,13] float32; ref_means / ref_stds: what the reference's
    calculate_dataset_stats returned for them; ref_mean_dist / ref_std_dist: its
    own distance from two_pass (mean_err / std_err, the largest channel) as
    measured when the fixture was made."""
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def assert_matches(got_mean, got_std, ref, bound=BOUND, what=""):
    me, se = mean_err(got_mean, ref["mean"]), std_err(got_std, ref["std"])
    print(f"{what} mean err {me.max():.3e} std err {se.max():.3e} (bound {bound:.0e})")
    assert (me <= bound).all(), (what, me.tolist())
    assert (se <= bound).all(), (what, se.tolist())
