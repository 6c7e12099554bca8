"""Golden fixture for the channel statistics, made by running the REFERENCE's own
calculate_dataset_stats.py (/root/reference, read-only) here.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stats.py

dataset_stats.npz holds
  inputs [5,7,10,13] float32: channels 0-2 unit normals, 3 a far-from-zero depth
    (1000 + 0.01 N(0,1), rounded to float32), 4 of scale 1e-3, 5 constant
    (sigma = 0), 6 uniform in [0,4];
  ref_means / ref_stds: what `calculate_dataset_stats(dir)` returned for them
    (two host sweeps, float32 pairwise sums per frame and channel into float64);
  ref_mean_dist / ref_std_dist: the reference's distance from the tests'
    yardstick (tests/stats_util.py two_pass: exact float64 two-pass), in the
    measure the tests bound (mean relative to max(|mean|, 1), sigma relative to
    max(sigma, tiny)), the largest channel.

The fixture holds inputs and recorded results only. Never shipped to or run on
the GPU box.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))

import stats_util as U  # noqa: E402


def make_inputs():
    rng = np.random.default_rng(20240607)
    N, H, W = 5, 10, 13
    x = np.empty((N, 7, H, W), dtype=np.float32)
    n = rng.standard_normal((N, 3, H, W))
    x[:, 0:3] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    x[:, U.DEPTH] = (1000.0 + 0.01 * rng.standard_normal((N, H, W))).astype(np.float32)
    x[:, U.SMALL] = (1e-3 * rng.standard_normal((N, H, W))).astype(np.float32)
    x[:, U.CONST] = np.float32(0.75)   # every float32 partial sum of it is exact
    x[:, U.UNIFORM] = rng.uniform(0.0, 4.0, (N, H, W)).astype(np.float32)
    return x


if __name__ == "__main__":
    sys.path.insert(0, REF)
    x = make_inputs()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)  # the reference writes train_stats.npy / .json beside the data
        try:
            np.save(os.path.join(d, "train_inputs.npy"), x)
            from calculate_dataset_stats import calculate_dataset_stats
            st = calculate_dataset_stats(d)
        finally:
            os.chdir(cwd)
    assert st is not None
    means, stds = np.array(st["means"], np.float64), np.array(st["stds"], np.float64)
    ref = U.two_pass(x)
    me, se = U.mean_err(means, ref["mean"]), U.std_err(stds, ref["std"])
    nm, ns = U.naive_one_pass(x)
    print("reference vs two-pass: mean", me.tolist(), "\n  std", se.tolist())
    print("depth: reference mean abs", abs(means[U.DEPTH] - ref["mean"][U.DEPTH]),
          "std rel", se[U.DEPTH], "; naive one-pass std rel", U.std_err(ns, ref["std"])[U.DEPTH])
    assert ref["std"][U.CONST] == 0.0 and stds[U.CONST] == 0.0
    np.savez_compressed(os.path.join(HERE, "dataset_stats.npz"), inputs=x, ref_means=means,
                        ref_stds=stds, ref_mean_dist=np.array(me.max()),
                        ref_std_dist=np.array(se.max()))
