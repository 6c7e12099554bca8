"""GPU: bench.py's plain run and --dump-outputs on a small train step (B=2,
7x64x64, 2 timed steps): the plain record carries the headline keys and none
of what --full adds; the dump holds what the last timed step handed its
caller, float32, and two runs of the same arguments (same seeded inputs)
agree within the fp32 parity bounds of tests/util.py."""
import argparse
import os
import sys

import numpy as np
import pytest

from util import LOSS_REL, OUT_ABS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

B, RES, STEPS = 2, 64, 2


def _measure(device, out_dir, full=False):
    import bench
    args = argparse.Namespace(batch=B, in_ch=7, res=RES, dtype="f32", steps=STEPS, warmup=1,
                              vgg=False, workload="train", full=full,
                              dump_outputs=str(out_dir) if out_dir else None)
    return bench.train_measure(args, 1, 0, device)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_times_the_steps_and_dumps_them(device, tmp_path):
    import bench
    res = _measure(device, tmp_path / "a")
    assert res["steps"] == STEPS and res["unit"] == "frames/s" and res["higher_is_better"]
    assert res["dtype"] == "f32" and res["ms_per_step"] > 0
    assert abs(res["value"] - B * 1e3 / res["ms_per_step"]) <= 2e-3 * res["value"]
    assert res["step_execution"].startswith("eager")
    for k in ("stages", "roofline", "graph", "eager", "secondary", "cpu_baseline"):
        assert k not in res
    a = _load(tmp_path / "a")
    assert sorted(a) == ["buffers", "loss", "out", "params", "x_grad"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64e6
    assert a["out"].shape[0] == B and a["out"].shape[-2:] == (RES, RES)
    assert a["x_grad"].shape == (B, 7, RES, RES) and np.abs(a["x_grad"]).max() > 0
    assert a["params"].shape == (bench.DUMP_MAX_ELEMS,) and a["loss"].shape == ()
    _measure(device, tmp_path / "b")
    b = _load(tmp_path / "b")
    assert abs(a["loss"] - b["loss"]) <= LOSS_REL * abs(a["loss"])
    assert np.abs(a["out"] - b["out"]).max() <= OUT_ABS
    assert np.array_equal(a["buffers"].shape, b["buffers"].shape)
