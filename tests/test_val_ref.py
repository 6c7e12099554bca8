"""CPU: the yardstick of the validation tests (val_util.py) on a hand-computed
example, the host arithmetic of MetricsResult / ValidationResult from given
accumulator values, and the C ABI of the metrics pass as far as it needs no GPU."""
import math
import os
import re

import numpy as np
import torch

import val_util as V
from nsm_amd.validation import (MetricsResult, ValidationResult, metrics_of, per_image_of,
                                result_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nsm.h")


# ---- 1. the yardstick, by hand ---------------------------------------------------------
def test_yardstick_hand_example():
    """d = {0, .5, 1, 0, -.5, 0}: sum|d| = 2, sum d^2 = 1.5, mse = 1/4, psnr =
    20 log10(1 / (1/2)) = 20 log10 2."""
    o = np.array([[0.0, 0.5, 1.0], [0.25, 0.25, 0.25]], dtype=np.float32)
    t = np.array([[0.0, 0.0, 0.0], [0.25, 0.75, 0.25]], dtype=np.float32)
    whole = V.records(o.reshape(1, 2, 3), t.reshape(1, 2, 3))
    assert whole.tolist() == [[6.0, 2.0, 1.5, 1.0, 0.0, 0.0]]
    f = V.figures(whole[0])
    assert f["count"] == 6 and f["l1"] == 2.0 / 6.0 and f["mse"] == 0.25
    assert f["psnr"] == 20.0 * math.log10(2.0) and abs(f["psnr"] - 6.020599913279624) < 1e-14
    rows = V.records(o, t)            # each row an image
    assert rows.tolist() == [[3.0, 1.5, 1.25, 1.0, 0.0, 0.0], [3.0, 0.5, 0.25, 0.5, 0.0, 0.0]]
    assert V.fold(rows).tolist() == whole[0].tolist()


def test_yardstick_zero_error_empty_image_and_range():
    o = np.array([[0.5, 0.25], [np.nan, np.inf], [-0.5, 1.5], [np.nan, 2.0]], dtype=np.float32)
    t = np.array([[0.5, 0.25], [0.0, 0.0], [0.0, 1.0], [0.0, -np.inf]], dtype=np.float32)
    r = V.records(o, t)
    same, empty, outside, mixed = (V.figures(x) for x in r)
    assert same["mse"] == 0.0 and same["psnr"] == float("inf") and same["l1"] == 0.0
    assert r[1].tolist() == [0.0, 0.0, 0.0, 0.0, 2.0, 0.0]
    assert all(math.isnan(empty[k]) for k in ("l1", "mse", "psnr")) and empty["count"] == 0
    # outside [0, 1] still counts in the sums
    assert r[2].tolist() == [2.0, 1.0, 0.5, 0.5, 0.0, 2.0]
    # an out-of-range output whose partner is non-finite is left out of every other field
    assert r[3].tolist() == [0.0, 0.0, 0.0, 0.0, 2.0, 0.0] and mixed["out_of_range"] == 0


def test_validate_direct_restatement():
    m = V.validate_direct_means([0.5, 0.25, 0.125], [0.1, 0.2, 0.4], [1.0, 2.0, 3.0])
    assert m == {"loss": (0.5 + 0.25 + 0.125) / 3, "l1_loss": (0.0 + 0.1 + 0.2 + 0.4) / 3,
                 "perturbation_loss": 2.0, "batches": 3}
    e = V.validate_direct_means([], [])
    assert e["loss"] == e["l1_loss"] == float("inf") and e["perturbation_loss"] == 0.0


# ---- 2. host arithmetic of the results -----------------------------------------------
def test_metrics_result_from_a_record():
    r = metrics_of([6.0, 2.0, 1.5, 1.0, 3.0, 2.0])
    assert isinstance(r, MetricsResult) and r.per_image is None
    assert (r.count, r.l1, r.mse, r.max_abs, r.nonfinite, r.out_of_range) == \
        (6, 2.0 / 6.0, 0.25, 1.0, 3, 2)
    assert r.psnr == V.psnr(0.25)
    assert type(r.count) is int and type(r.nonfinite) is int and type(r.mse) is float
    z = metrics_of([4.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    assert z.mse == 0.0 and z.psnr == float("inf")
    e = metrics_of([0.0, 0.0, 0.0, 0.0, 5.0, 0.0])
    assert e.count == 0 and e.nonfinite == 5
    assert math.isnan(e.l1) and math.isnan(e.mse) and math.isnan(e.psnr)
    p = per_image_of(torch.tensor([[6.0, 2.0, 1.5, 1.0, 3.0, 2.0], [4.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                                   [0.0, 0.0, 0.0, 0.0, 5.0, 0.0]], dtype=torch.float64))
    assert p.count.tolist() == [6, 4, 0] and p.count.dtype == torch.int64
    assert p.mse[:2].tolist() == [0.25, 0.0] and math.isnan(p.mse[2].item())
    assert abs(p.psnr[0].item() - V.psnr(0.25)) < 1e-12 and p.psnr[1].item() == float("inf")
    assert math.isnan(p.psnr[2].item()) and math.isnan(p.l1[2].item())
    assert p.nonfinite.tolist() == [3, 0, 5] and p.out_of_range.tolist() == [2, 0, 0]


def test_validation_result_from_accumulators():
    """acc = {batches, total, parts..., batch L1s, images}: means over batches."""
    names = ("l1_loss", "vgg_loss", "perturbation_loss")
    acc = [3.0, 0.875, 0.75, 0.3, 1.5, 0.7, 5.0]
    state = [6.0, 2.0, 1.5, 1.0, 0.0, 1.0]
    log = [[3.0, 1.5, 1.25, 1.0, 0.0, 0.0], [3.0, 0.5, 0.25, 0.5, 0.0, 1.0], [0.0] * 6]
    r = result_of(acc, state, names, log)
    ref = V.validate_direct_means([0.5, 0.25, 0.125], [0.1, 0.2, 0.4])
    assert isinstance(r, ValidationResult)
    assert r.loss == ref["loss"] == 0.875 / 3 and r.l1_loss == 0.7 / 3
    assert abs(r.l1_loss - ref["l1_loss"]) < 1e-15
    assert r.batches == 3 and float(r) == r.loss
    assert r.parts == {"l1_loss": 0.25, "vgg_loss": 0.3 / 3, "perturbation_loss": 0.5}
    assert r.perturbation_loss == 0.5 and r.vgg_loss == 0.3 / 3
    assert r.metrics.count == 6 and r.metrics.mse == 0.25 and r.metrics.out_of_range == 1
    # 5 images seen, a log of 3: all three rows
    assert r.per_image.count.tolist() == [3, 3, 0]
    # comparisons go by the loss, both ways, against floats and results
    best = float("inf")
    assert r < best and not r > best and r <= r.loss and r >= r.loss and best > r
    worse = result_of([1.0, 0.5, 0.1, 1.0], state)
    assert r < worse and worse > r and min(worse, r) is r
    assert worse.perturbation_loss == 0.0 and worse.parts == {"perturbation_loss": 0.0}
    assert worse.per_image is None
    # two images seen of a log of 3: only those
    few = result_of([1.0, 0.5, 0.1, 2.0], state, (), log)
    assert few.per_image.count.tolist() == [3, 3]
    # what ReduceLROnPlateau does with its argument
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(
        torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0), patience=0)
    sched.step(r)
    assert sched.best == r.loss
    # no batch: main.py:641
    none = result_of([0.0] * 4, [0.0] * 6)
    assert none.loss == none.l1_loss == float("inf") and none.batches == 0
    assert math.isnan(none.metrics.mse)


# ---- 3. the C ABI, without a GPU -----------------------------------------------------------
def test_header_block_and_block_counts():
    import nsm_amd._lib as L
    from nsm_amd import validation
    txt = open(HEADER).read()
    assert int(re.search(r"#define\s+NSM_METRICS_SCALARS\s+(\d+)", txt).group(1)) == \
        validation.MAX_SCALARS == 8
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("nsm_metrics_blocks", "nsm_metrics_partial", "nsm_metrics_merge"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert len(m.group(1).split(",")) == len(L._SIGS[name][1]), name
    blocks = L.lib.nsm_metrics_blocks
    assert blocks(0) == 0 and blocks(-5) == 0 and blocks(2 ** 31) == 0
    assert blocks(1) == 1 and blocks(2 ** 31 - 1) >= 1
    span = next(n for n in range(1, 1 << 20) if blocks(n + 1) == 2)
    assert blocks(span) == 1 and blocks(2 * span + 1) == 3
    assert blocks(1080 * 1920) >= 200          # enough blocks for every CU at 1080p
    # argument checks fail before any launch
    assert L.lib.nsm_metrics_partial(None, None, 1, 16, 0.0, 1.0, None, None) == 1
    assert "null" in L.last_error()
    assert L.lib.nsm_metrics_merge(None, 1, 1, None, 0, None, None, 0, None, None, None) == 1
    assert "null" in L.last_error()


def test_cpu_tensors_are_refused():
    import nsm_amd
    import pytest
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(nsm_amd.NsmError):
        nsm_amd.image_metrics(x, x)
    with pytest.raises(ValueError):
        nsm_amd.image_metrics(x[0], x[0])
