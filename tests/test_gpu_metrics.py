"""GPU: the image-error metrics pass (nsm_metrics_partial / nsm_metrics_merge;
image_metrics, ImageMetrics) against the numpy float64 yardstick of val_util.py
on the same float32 samples.

Every summed term is >= 0, so any summation order is within n * 2^-53 relative of
the exact sum; every case here has n < 2^17, which puts that below 1e-10
(val_util.BOUND): sum|d|, sum d^2, l1 and mse within it, count, max|d|,
nonfinite and out_of_range exactly."""
import ctypes
import math

import numpy as np
import pytest
import torch

import val_util as V

pytestmark = pytest.mark.gpu


def pair(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.random(shape, dtype=np.float32), rng.random(shape, dtype=np.float32)


def run(o, t, lo=0.0, hi=1.0, state=None, scalars=(), acc=None, log=None):
    """The two launches through _lib on device tensors o, t [B, ...]: returns
    (records, frames [B,6], state [6])."""
    from nsm_amd._lib import call, lib, ptr, stream
    B, n = o.shape[0], o[0].numel()
    per = lib.nsm_metrics_blocks(n)
    assert per >= 1
    ws = torch.full((B * per, 6), -7.0, dtype=torch.float64, device=o.device)
    frames = torch.full((B, 6), -7.0, dtype=torch.float64, device=o.device)
    if state is None:
        state = torch.zeros(6, dtype=torch.float64, device=o.device)
    call("nsm_metrics_partial", ptr(o), ptr(t), B, n, lo, hi, ptr(ws), stream())
    K = len(scalars)
    table = (ctypes.c_void_p * K)(*[s.data_ptr() for s in scalars]) if K else None
    call("nsm_metrics_merge", ptr(ws), B, per, table, K, ptr(frames), ptr(log),
         0 if log is None else log.shape[0], ptr(state), ptr(acc), stream())
    return ws, frames, state


def check_records(got, ref, what):
    got = np.asarray(got.cpu().numpy() if torch.is_tensor(got) else got, np.float64).reshape(-1, 6)
    ref = np.asarray(ref, np.float64).reshape(-1, 6)
    err = max(V.rel(got[:, V.S1], ref[:, V.S1]).max(), V.rel(got[:, V.S2], ref[:, V.S2]).max())
    print(f"{what}: sums within {err:.2e} (bound {V.BOUND:.0e})")
    for f in (V.COUNT, V.MAX, V.BAD, V.OOR):
        assert np.array_equal(got[:, f], ref[:, f]), (what, f, got[:, f], ref[:, f])
    assert err <= V.BOUND, (what, err)


def check_result(res, rec, what):
    ref = V.figures(rec)
    for k in ("count", "max_abs", "nonfinite", "out_of_range"):
        assert getattr(res, k) == ref[k], (what, k)
    for k in ("l1", "mse"):
        got = getattr(res, k)
        if math.isnan(ref[k]):
            assert math.isnan(got), (what, k)
        else:
            assert V.rel(got, ref[k]) <= V.BOUND, (what, k, got, ref[k])
    if math.isnan(ref["psnr"]) or math.isinf(ref["psnr"]):
        assert str(res.psnr) == str(ref["psnr"]), (what, res.psnr)
    else:   # d psnr = (10 / ln 10) * d mse / mse
        assert abs(res.psnr - ref["psnr"]) <= 4.35 * V.BOUND, (what, res.psnr, ref["psnr"])


# ---- 1. shapes where the kernel can go wrong -------------------------------------------
# 2x1x150x151: 22650 elements an image = two whole blocks + 6266, odd, so the second
# image starts off the 16-byte grid; 9 images cross the merge's rounds of eight
SHAPES = [(1, 1, 1, 1), (2, 1, 7, 13), (9, 1, 16, 16), (2, 1, 150, 151)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_shapes(device, shape):
    import nsm_amd
    from nsm_amd._lib import lib
    o, t = pair(shape, sum(shape))
    od, td = torch.from_numpy(o).to(device), torch.from_numpy(t).to(device)
    ref = V.records(o, t)
    per = lib.nsm_metrics_blocks(od[0].numel())
    if shape[-1] == 151:
        assert per >= 3 and od[0].numel() < 2 ** 17 and od[0].numel() % 4
    ws, frames, state = run(od, td)
    assert not (ws == -7.0).any()                    # every block wrote its record
    check_records(frames, ref, f"frames {shape}")
    check_records(state, V.fold(ref), f"state {shape}")
    res = nsm_amd.image_metrics(od, td, per_image=True)
    check_result(res, V.fold(ref), f"image_metrics {shape}")
    assert res.per_image.count.tolist() == ref[:, V.COUNT].tolist()
    assert V.rel(res.per_image.mse.cpu().numpy(), ref[:, V.S2] / ref[:, V.COUNT]).max() <= V.BOUND
    assert res.per_image.max_abs.cpu().numpy().tolist() == ref[:, V.MAX].tolist()
    assert nsm_amd.image_metrics(od, td).per_image is None


@pytest.mark.parametrize("shifts", [(1, 1), (1, 2), (3, 0), (0, 3)], ids=str)
def test_views_off_the_16_byte_grid(device, shifts):
    """[3,2,5,11] as views starting 1..3 floats into larger buffers: a misaligned
    head, and a target that sits differently from the output."""
    import nsm_amd
    shape = (3, 2, 5, 11)
    o, t = pair(shape, 5)
    views = []
    for a, s in ((o, shifts[0]), (t, shifts[1])):
        buf = torch.full((a.size + 8,), float("nan"), dtype=torch.float32, device=device)
        v = buf[s:s + a.size].view(shape)
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == 4 * s and v.is_contiguous()
        views.append(v)
    ref = V.records(o, t)
    _, frames, state = run(*views)
    check_records(frames, ref, f"shifts {shifts}")
    check_result(nsm_amd.image_metrics(*views), V.fold(ref), f"shifts {shifts}")


def test_other_dtypes_are_cast(device):
    import nsm_amd
    o, t = pair((2, 1, 7, 13), 3)
    od = torch.from_numpy(o).to(device).to(torch.bfloat16)
    td = torch.from_numpy(t).to(device).double()
    ref = V.fold(V.records(od.float().cpu().numpy(), td.float().cpu().numpy()))
    check_result(nsm_amd.image_metrics(od, td), ref, "bf16 against fp64")
    with pytest.raises(ValueError, match="shape mismatch"):
        nsm_amd.image_metrics(od, td[:1])


# ---- 2. edge cases -------------------------------------------------------------------------
def test_edge_cases(device):
    import nsm_amd
    o, t = pair((4, 1, 7, 13), 9)
    of, tf = o.reshape(4, -1), t.reshape(4, -1)
    of[0, 3], tf[0, 10] = np.nan, np.inf          # NaN in o, Inf in t,
    of[0, 20], tf[0, 20] = -np.inf, np.nan        # and both at one index
    of[1, :] = np.nan                             # an image without a finite pair
    tf[2, :] = of[2, :]                           # identical
    of[3, 0], of[3, 90] = -0.5, 1.5               # outside [0, 1]: counted, and in the sums
    od, td = torch.from_numpy(o).to(device), torch.from_numpy(t).to(device)
    ref = V.records(o, t)
    assert ref[:, V.BAD].tolist() == [3, 91, 0, 0] and ref[:, V.OOR].tolist() == [0, 0, 0, 2]
    assert ref[:, V.COUNT].tolist() == [88, 0, 91, 91]
    _, frames, state = run(od, td)
    check_records(frames, ref, "edge cases")
    assert frames[1].tolist() == [0.0, 0.0, 0.0, 0.0, 91.0, 0.0]
    assert frames[2, 1:4].tolist() == [0.0, 0.0, 0.0]
    res = nsm_amd.image_metrics(od, td, per_image=True)
    check_result(res, V.fold(ref), "edge cases, whole batch")
    p = res.per_image
    assert math.isnan(p.l1[1].item()) and math.isnan(p.mse[1].item()) and math.isnan(p.psnr[1].item())
    assert p.mse[2].item() == 0.0 and p.psnr[2].item() == float("inf")
    # the single images through the host arithmetic
    same = nsm_amd.image_metrics(od[2:3], td[2:3])
    assert same.mse == 0.0 and same.l1 == 0.0 and same.psnr == float("inf") and same.count == 91
    none = nsm_amd.image_metrics(od[1:2], td[1:2])
    assert none.count == 0 and none.nonfinite == 91 and none.max_abs == 0.0
    assert math.isnan(none.l1) and math.isnan(none.mse) and math.isnan(none.psnr)
    # another range: [0.25, 0.5]
    wide = nsm_amd.image_metrics(od, td, value_range=(0.25, 0.5))
    assert wide.out_of_range == int(V.fold(V.records(o, t, 0.25, 0.5))[V.OOR]) > 2


# ---- 3. determinism and accumulation ----------------------------------------------------------
def test_same_call_same_bits(device):
    o, t = pair((2, 1, 150, 151), 21)
    od, td = torch.from_numpy(o).to(device), torch.from_numpy(t).to(device)
    a, b = run(od, td), run(od, td)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64))


def test_split_updates_and_merge(device):
    import nsm_amd
    o, t = pair((8, 1, 16, 16), 4)
    o[5, 0, 0, 0], o[1, 0, 3, 3] = np.nan, 1.5
    od, td = torch.from_numpy(o).to(device), torch.from_numpy(t).to(device)
    ref = V.fold(V.records(o, t))
    whole = nsm_amd.ImageMetrics()
    assert whole.update(od, td) is None
    halves = nsm_amd.ImageMetrics()
    table = torch.cat([halves.update(od[:4], td[:4], per_image=True),
                       halves.update(od[4:], td[4:], per_image=True)])
    check_records(table, V.records(o, t), "per-image tables of 4 + 4")
    a, b = nsm_amd.ImageMetrics(), nsm_amd.ImageMetrics()
    a.update(od[:4], td[:4])
    b.update(od[4:], td[4:])
    merged = nsm_amd.ImageMetrics().merge(a).merge(b)
    assert nsm_amd.ImageMetrics().merge(nsm_amd.ImageMetrics())._state is None
    for acc, what in ((whole, "8 at once"), (halves, "4 + 4"), (merged, "merge of two")):
        check_records(acc._state, ref, what)
        check_result(acc.compute(), ref, what)
    for acc in (halves, merged):
        for f in (V.COUNT, V.MAX, V.BAD, V.OOR):
            assert acc._state[f].item() == whole._state[f].item()
    # reset() starts over, in place
    ptr = whole._state.data_ptr()
    whole.reset()
    whole.update(od[:4], td[:4])
    assert whole._state.data_ptr() == ptr
    assert torch.equal(whole._state.view(torch.int64), a._state.view(torch.int64))
    with pytest.raises(RuntimeError):
        nsm_amd.ImageMetrics().compute()


# ---- 4. the accumulator and the log ---------------------------------------------------------
def test_accumulator_and_log(device):
    o, t = pair((6, 1, 7, 13), 8)
    o[4] = np.nan                                   # the third batch's first image: no finite pair
    o[5] = np.inf                                   # nor its second
    od, td = torch.from_numpy(o).to(device), torch.from_numpy(t).to(device)
    K = 3
    vals = [[0.1, 0.25, 3.0], [0.7, 1e-3, 2.5], [1.0, 2.0, 4.0]]
    acc = torch.zeros(3 + K, dtype=torch.float64, device=device)
    state = torch.zeros(6, dtype=torch.float64, device=device)
    log = torch.full((3, 6), -1.0, dtype=torch.float64, device=device)
    want = [0.0] * (3 + K)
    frames = []
    for i in range(2):
        sc = [torch.tensor(v, dtype=torch.float32, device=device) for v in vals[i]]
        _, fr, _ = run(od[2 * i:2 * i + 2], td[2 * i:2 * i + 2], state=state, scalars=sc, acc=acc,
                       log=log)
        frames.append(fr)
        fr = fr.tolist()
        want[0] += 1.0
        for k in range(K):
            want[1 + k] += float(np.float32(vals[i][k]))
        want[1 + K] += (0.0 + fr[0][V.S1] + fr[1][V.S1]) / (0.0 + fr[0][V.COUNT] + fr[1][V.COUNT])
        want[2 + K] += 2.0
    assert acc.tolist() == want                     # the Python float sums, exactly
    table = torch.cat(frames)
    check_records(table, V.records(o[:4], t[:4]), "frames of two batches")
    # the log holds the first three images and dropped the fourth
    assert torch.equal(log.view(torch.int64), table[:3].view(torch.int64))
    # a third batch: nothing more is logged, the images seen keep counting, and a batch
    # without a finite pair has no L1
    sc = [torch.tensor(v, dtype=torch.float32, device=device) for v in vals[2]]
    run(od[4:6], td[4:6], state=state, scalars=sc, acc=acc, log=log)
    got = acc.tolist()
    assert torch.equal(log.view(torch.int64), table[:3].view(torch.int64))
    assert got[0] == 3.0 and got[2 + K] == 6.0 and math.isnan(got[1 + K])
    assert got[1:1 + K] == [want[1 + k] + float(np.float32(vals[2][k])) for k in range(K)]
    assert state.tolist()[V.BAD] == 2 * 91 and state.tolist()[V.COUNT] == 4 * 91
    # no accumulator, no log: only the state moves
    before = acc.clone()
    run(od[:2], td[:2], state=state)
    assert torch.equal(acc.view(torch.int64), before.view(torch.int64))
    # capacity 0 with an accumulator: counted, not logged
    run(od[:2], td[:2], state=state, acc=acc, scalars=sc, log=log[:0])
    assert acc[2 + K].item() == 8.0
    assert torch.equal(log.view(torch.int64), table[:3].view(torch.int64))


def test_argument_checks(device):
    from nsm_amd._lib import NsmError, call, ptr
    x = torch.zeros(16, dtype=torch.float32, device=device)
    rec = torch.zeros(6, dtype=torch.float64, device=device)
    with pytest.raises(NsmError, match="range"):
        call("nsm_metrics_partial", ptr(x), ptr(x), 1, 16, 1.0, 0.0, ptr(rec), None)
    with pytest.raises(NsmError, match="shape"):
        call("nsm_metrics_partial", ptr(x), ptr(x), 0, 16, 0.0, 1.0, ptr(rec), None)
    with pytest.raises(NsmError, match="scalars"):
        call("nsm_metrics_merge", ptr(rec), 1, 1, None, 9, None, None, 0, ptr(rec), ptr(rec), None)
    with pytest.raises(NsmError, match="accumulator"):
        call("nsm_metrics_merge", ptr(rec), 1, 1, None, 0, None, ptr(rec), 1, ptr(rec), None, None)
