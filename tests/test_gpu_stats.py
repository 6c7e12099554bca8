"""GPU: the device-side channel statistics (nsm_stats_partial / nsm_stats_merge;
ChannelStats, channel_stats, dataset_stats, FrameLoader(stats=)) against the
exact float64 two-pass of stats_util.py on the same float32 samples. Mean and
sigma within 1e-10 (sigma relative to max(sigma, tiny), the mean to
max(|mean|, 1)); count, min, max and the non-finite counts exactly.

Worst measured on an MI355X over every case below: sigma 4.6e-13, mean 2.1e-16
("Dataset channel statistics")."""
import json
import os

import numpy as np
import pytest
import torch

import stats_util as U

pytestmark = pytest.mark.gpu
torch.set_num_threads(16)


@pytest.fixture(scope="module")
def fx():
    d = U.load_fixture()
    d["ref"] = U.two_pass(d["inputs"])
    return d


def check(res, ref, what, bound=U.BOUND):
    """StatsResult (device tensors) against a two_pass dict."""
    U.assert_matches(res.means.cpu().numpy(), res.stds.cpu().numpy(), ref, bound, what)
    assert res.means.dtype == res.stds.dtype == torch.float64
    assert np.array_equal(res.count.cpu().numpy(), ref["count"]), what
    assert np.array_equal(res.nonfinite.cpu().numpy(), ref["nonfinite"]), what
    assert np.array_equal(res.mins.cpu().numpy(), ref["min"]), what
    assert np.array_equal(res.maxs.cpu().numpy(), ref["max"]), what
    assert not torch.isnan(res.means).any() and not torch.isnan(res.stds).any()


def fed(device, x, sizes):
    import nsm_amd
    acc = nsm_amd.ChannelStats(x.shape[1])
    i = 0
    for n in sizes:
        acc.update(torch.from_numpy(x[i:i + n]).to(device))
        i += n
    assert i == len(x)
    return acc


def write_dataset(d, x, split="train"):
    np.save(os.path.join(d, f"{split}_inputs.npy"), x)
    np.save(os.path.join(d, f"{split}_labels.npy"),
            np.zeros((x.shape[0], 1) + x.shape[2:], dtype=np.float64))


# ---- 1. parity ---------------------------------------------------------------------
def test_fixture_parity(device, fx):
    """Planes of 130 floats: every other one starts off a 16-byte boundary."""
    res = fed(device, fx["inputs"], (2, 2, 1)).compute()
    check(res, fx["ref"], "fixture 2+2+1")
    assert res.stds[U.CONST].item() == 0.0
    assert res.count.tolist() == [5 * 10 * 13] * 7


# ---- 2. shapes where the kernel can go wrong ------------------------------------------
def shaped(shape, seed):
    """Every channel far from zero in its own way: offset 1000 / -3 / 0 by channel,
    spread 0.01 / 1 / 1e-3."""
    rng = np.random.default_rng(seed)
    B, C, H, W = shape
    off = np.array([1000.0, -3.0, 0.0])[np.arange(C) % 3].reshape(1, C, 1, 1)
    sc = np.array([0.01, 1.0, 1e-3])[np.arange(C) % 3].reshape(1, C, 1, 1)
    return (off + sc * rng.standard_normal(shape)).astype(np.float32)


SHAPES = [(1, 1, 1, 1), (2, 3, 1, 5), (3, 1, 64, 64), (1, 2, 300, 301),
          (2, 2, 181, 183)]   # 33123 = one whole block + 355, odd: ragged heads and tails


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_shapes(device, shape):
    import nsm_amd
    x = shaped(shape, sum(shape))
    res = nsm_amd.channel_stats(torch.from_numpy(x).to(device))
    check(res, U.two_pass(x), f"shape {shape}")
    if shape == (1, 1, 1, 1):
        assert res.stds.item() == 0.0 and res.means.item() == float(x.reshape(-1)[0])
        assert torch.isnan(res.std()).all()          # n - 1 = 0, as torch.std
    else:
        n = res.count.double()
        assert torch.equal(res.std(), res.stds * torch.sqrt(n / (n - 1)))


@pytest.mark.parametrize("shift", (1, 2, 3))
def test_storage_off_the_16_byte_grid(device, shift):
    """The tensor itself starts 4, 8 or 12 bytes past a 16-byte boundary."""
    import nsm_amd
    shape = (2, 3, 9, 31)
    x = shaped(shape, 5)
    buf = torch.zeros(x.size + 8, dtype=torch.float32, device=device)
    view = buf[shift:shift + x.size].view(shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 * shift and view.is_contiguous()
    check(nsm_amd.channel_stats(view), U.two_pass(x), f"shift {shift}")


# ---- 3. split invariance and determinism --------------------------------------------
def test_split_invariance_and_determinism(device, fx):
    a = fed(device, fx["inputs"], (3, 1, 1))
    b = fed(device, fx["inputs"], (5,))
    ra, rb = a.compute(), b.compute()
    me = U.mean_err(ra.means.cpu().numpy(), rb.means.cpu().numpy()).max()
    se = U.std_err(ra.stds.cpu().numpy(), rb.stds.cpu().numpy()).max()
    print(f"3+1+1 against 5 at once: mean {me:.2e} sigma {se:.2e}")
    assert me <= 1e-12 and se <= 1e-12
    for f in ("count", "mins", "maxs", "nonfinite"):
        assert torch.equal(getattr(ra, f), getattr(rb, f))
    again = fed(device, fx["inputs"], (3, 1, 1))
    assert a._state.shape == (7, 6) and a._state.dtype == torch.float64
    assert torch.equal(a._state.view(torch.int64), again._state.view(torch.int64))
    # reset() starts over, in place
    ptr = a._state.data_ptr()
    a.reset()
    a.update(torch.from_numpy(fx["inputs"]).to(device))
    assert a._state.data_ptr() == ptr
    assert torch.equal(a._state.view(torch.int64), b._state.view(torch.int64))


# ---- 4. per-frame table ------------------------------------------------------------
def test_per_frame_table(device, fx):
    import nsm_amd
    from nsm_amd.stats import result_of
    x = fx["inputs"]
    acc = nsm_amd.ChannelStats(7)
    table = torch.cat([acc.update(torch.from_numpy(x[i:j]).to(device), per_frame=True)
                       for i, j in ((0, 2), (2, 5))])
    assert tuple(table.shape) == (5, 7, 6) and table.dtype == torch.float64
    check(result_of(table), U.per_frame(x), "per frame")
    check(acc.compute(), fx["ref"], "state beside the per-frame table")
    # several blocks per plane
    big = shaped((2, 2, 181, 183), 11)
    t = nsm_amd.ChannelStats(2).update(torch.from_numpy(big).to(device), per_frame=True)
    check(result_of(t), U.per_frame(big), "per frame, 2 blocks a plane")


# ---- 5. non-finite samples -----------------------------------------------------------
def test_nonfinite_samples(device, fx, tmp_path):
    import nsm_amd
    x = fx["inputs"].copy()
    x[1, 2, 3, 4], x[2, 2, 0, 0], x[4, 2, 9, 12] = np.nan, np.inf, -np.inf
    ref = U.two_pass(x)
    res = fed(device, x, (2, 2, 1)).compute()
    assert res.nonfinite.tolist() == [0, 0, 3, 0, 0, 0, 0]
    assert res.count.tolist() == [650, 650, 647, 650, 650, 650, 650]
    check(res, ref, "three non-finite pixels")
    write_dataset(str(tmp_path), x)
    with pytest.raises(ValueError, match=r"channel 2 \(3\)"):
        nsm_amd.dataset_stats(str(tmp_path), batch=2, device=device)
    assert not (tmp_path / "train_stats.json").exists()
    res = nsm_amd.dataset_stats(str(tmp_path), batch=2, device=device, nonfinite="skip")
    check(res, ref, "dataset_stats, nonfinite='skip'")
    assert (tmp_path / "train_stats.json").exists()
    # a plane without a finite sample
    y = np.full((1, 2, 3, 5), np.nan, dtype=np.float32)
    y[0, 1] = 2.5
    check(nsm_amd.channel_stats(torch.from_numpy(y).to(device)), U.two_pass(y), "all-NaN plane")


# ---- 6. graph capture ----------------------------------------------------------------
def test_graph_capture(device):
    """One update captured on one stream (no parallel branches) and replayed over
    three contents of its static input equals the eager sequence bit for bit."""
    import nsm_amd
    shape = (2, 3, 91, 97)
    contents = [torch.from_numpy(shaped(shape, s)).to(device) for s in (1, 2, 3)]
    eager = nsm_amd.ChannelStats(3)
    for c in contents:
        eager.update(c)
    static = torch.empty(shape, dtype=torch.float32, device=device)
    acc = nsm_amd.ChannelStats(3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up: kernels loaded, state and workspace allocated
        static.copy_(contents[0])
        acc.update(static)
    torch.cuda.current_stream().wait_stream(side)
    acc.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        acc.update(static)
    for c in contents:
        static.copy_(c)
        g.replay()
    assert torch.equal(acc._state.view(torch.int64), eager._state.view(torch.int64))
    check(acc.compute(), U.two_pass(np.concatenate([c.cpu().numpy() for c in contents])), "graph")


# ---- 7. end to end --------------------------------------------------------------------
def test_dataset_stats_end_to_end(device, fx, tmp_path):
    import nsm_amd
    from nsm_amd.data import FrameLoader, load_stats
    d = str(tmp_path)
    write_dataset(d, fx["inputs"])
    res, table = nsm_amd.dataset_stats(d, batch=2, device=device, per_frame=True)
    check(res, fx["ref"], "dataset_stats")
    assert tuple(table.shape) == (5, 7, 6)
    assert sorted(os.listdir(d)) == ["train_inputs.npy", "train_labels.npy", "train_stats.json"]
    text = open(os.path.join(d, "train_stats.json")).read()
    js = json.loads(text)
    assert list(js) == ["means", "stds"] and text == json.dumps(js, indent=4)
    assert js["means"] == res.means.tolist() and js["stds"] == res.stds.tolist()
    m, s = load_stats(d, 7)
    # the yardstick rounded to float32; 1e-10 of slack decides no rounding here
    assert torch.equal(m, torch.from_numpy(fx["ref"]["mean"]).to(torch.float32))
    assert torch.equal(s, torch.from_numpy(fx["ref"]["std"]).to(torch.float32))
    # the recorded reference: its own distance from the yardstick plus this pass's
    me = U.mean_err(js["means"], fx["ref_means"]).max()
    se = U.std_err(js["stds"], fx["ref_stds"]).max()
    print(f"against calculate_dataset_stats: mean {me:.2e} sigma {se:.2e}")
    assert me <= fx["ref_mean_dist"] + U.BOUND and se <= fx["ref_std_dist"] + U.BOUND
    a = FrameLoader(d, batch=2, device=device, stats=res)
    b = FrameLoader(d, batch=2, device=device)
    c = FrameLoader(d, batch=2, device=device, stats=(js["means"], js["stds"]))
    try:
        assert len(a) == len(b) == 3
        for _ in range(len(a)):
            (xa, ya), (xb, yb), (xc, _) = a.next(), b.next(), c.next()
            assert torch.equal(xa.detach().view(torch.int32), xb.detach().view(torch.int32))
            assert torch.equal(xc.detach().view(torch.int32), xb.detach().view(torch.int32))
            assert torch.equal(ya, yb)
        with pytest.raises(ValueError):
            FrameLoader(d, batch=2, device=device, stats=([0.0] * 4, [1.0] * 4))
    finally:
        for ld in (a, b, c):
            ld.close()


# ---- 8. shards ------------------------------------------------------------------------
def test_shards_merge(device, fx, tmp_path):
    """world = 2 as two loaders in turn on the one GPU, merged by ChannelStats.merge."""
    import nsm_amd
    from nsm_amd.data import FrameLoader
    d = str(tmp_path)
    write_dataset(d, fx["inputs"])
    whole = nsm_amd.dataset_stats(d, batch=2, device=device, save=False)
    assert os.listdir(d).count("train_stats.json") == 0
    accs, parts = [], []
    for rank in range(2):
        ld = FrameLoader(d, batch=2, device=device, world=2, rank=rank, apply_normalization=False)
        acc = nsm_amd.ChannelStats(ld.C)
        try:
            for _ in range(len(ld)):
                acc.update(ld.next()[0].detach())
        finally:
            ld.close()
        accs.append(acc)
        parts.append(nsm_amd.dataset_stats(d, batch=2, device=device, world=2, rank=rank,
                                           save=False))
    assert (parts[0].count + parts[1].count).tolist() == whole.count.tolist()
    merged = nsm_amd.ChannelStats(7).merge(accs[0]).merge(accs[1]).compute()
    from_results = nsm_amd.ChannelStats(7).merge(parts[0]).merge(parts[1]).compute()
    for got, what in ((merged, "two accumulators"), (from_results, "two StatsResults")):
        me = U.mean_err(got.means.cpu().numpy(), whole.means.cpu().numpy()).max()
        se = U.std_err(got.stds.cpu().numpy(), whole.stds.cpu().numpy()).max()
        print(f"{what} against the unsharded pass: mean {me:.2e} sigma {se:.2e}")
        assert me <= 1e-12 and se <= 1e-12
        for f in ("count", "mins", "maxs", "nonfinite"):
            assert torch.equal(getattr(got, f), getattr(whole, f))
        check(got, fx["ref"], what)
