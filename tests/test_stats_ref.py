"""CPU: the yardstick of the channel-statistics tests (stats_util.two_pass) agrees
with what the reference's calculate_dataset_stats recorded for the fixture, the
fixture's depth channel separates a cancelling form from the 1e-10 bound, and the
public entry points and the C ABI validate their arguments before any GPU work."""
import ctypes
import json

import numpy as np
import pytest
import torch

import nsm_amd
import nsm_amd._lib as L
import stats_util as U
from nsm_amd.data import load_stats


def test_yardstick_agrees_with_the_recorded_reference():
    """Margin: the reference's own distance from the yardstick, measured when the
    fixture was made, times 4 for summation-order differences between numpy builds."""
    fx = U.load_fixture()
    assert fx["inputs"].shape == (5, 7, 10, 13) and fx["inputs"].dtype == np.float32
    ref = U.two_pass(fx["inputs"])
    me, se = U.mean_err(fx["ref_means"], ref["mean"]), U.std_err(fx["ref_stds"], ref["std"])
    print("mean err", me.tolist(), "std err", se.tolist(),
          "recorded", float(fx["ref_mean_dist"]), float(fx["ref_std_dist"]))
    assert 0 < fx["ref_mean_dist"] < 1e-6 and 0 < fx["ref_std_dist"] < 1e-5
    assert (me <= 4 * fx["ref_mean_dist"]).all()
    assert (se <= 4 * fx["ref_std_dist"]).all()
    assert ref["std"][U.CONST] == 0.0 and fx["ref_stds"][U.CONST] == 0.0
    assert (ref["count"] == 5 * 10 * 13).all() and (ref["nonfinite"] == 0).all()


def test_fixture_discriminates_a_cancelling_form():
    """sum x and sum x^2 about zero, in float64, misses the bound on the depth
    channel (1000 + 0.01 N(0,1)) by orders of magnitude."""
    x = U.load_fixture()["inputs"]
    ref = U.two_pass(x)
    _, std = U.naive_one_pass(x)
    err = U.std_err(std, ref["std"])[U.DEPTH]
    print("naive one-pass depth sigma err", err)
    assert err > 1e3 * U.BOUND


def test_yardstick_handles_nonfinite_and_per_frame():
    x = U.load_fixture()["inputs"].copy()
    x[1, 2, 3, 4], x[2, 2, 0, 0], x[4, 2, 9, 12] = np.nan, np.inf, -np.inf
    ref = U.two_pass(x)
    assert ref["nonfinite"].tolist() == [0, 0, 3, 0, 0, 0, 0]
    assert ref["count"][2] == 650 - 3 and np.isfinite(ref["mean"]).all()
    pf = U.per_frame(x)
    assert pf["mean"].shape == (5, 7) and pf["nonfinite"][:, 2].tolist() == [0, 1, 1, 0, 1]
    keep = np.isfinite(x[:, 2])
    assert abs(ref["mean"][2] - x[:, 2][keep].astype(np.float64).mean()) <= 1e-15


BAD_INPUTS = [
    ("rank", torch.zeros(7, 8, 8)),
    ("channels", torch.zeros(2, 4, 8, 8)),
    ("float64", torch.zeros(2, 7, 8, 8, dtype=torch.float64)),
    ("float16", torch.zeros(2, 7, 8, 8, dtype=torch.float16)),
    ("empty", torch.zeros(0, 7, 8, 8)),
    ("not-a-tensor", [[[[0.0]]]]),
]


@pytest.mark.parametrize("x", [b[1] for b in BAD_INPUTS], ids=[b[0] for b in BAD_INPUTS])
def test_update_argument_errors_raise_before_gpu_work(x):
    """The inputs are CPU tensors: a ValueError (not the library's no-GPU error)
    shows that the check came first."""
    acc = nsm_amd.ChannelStats(7)
    with pytest.raises(ValueError):
        acc.update(x)
    if torch.is_tensor(x) and x.dim() == 4 and x.shape[1] != 7:
        return  # channel_stats takes the channel count from x
    with pytest.raises(ValueError):
        nsm_amd.channel_stats(x)


def test_cpu_tensor_is_rejected():
    x = torch.zeros(2, 7, 8, 8)
    with pytest.raises(nsm_amd.NsmError):
        nsm_amd.ChannelStats(7).update(x)
    with pytest.raises(nsm_amd.NsmError):
        nsm_amd.channel_stats(x)
    with pytest.raises(ValueError):
        nsm_amd.ChannelStats(0)
    with pytest.raises(RuntimeError):
        nsm_amd.ChannelStats(3).compute()
    with pytest.raises(ValueError):
        nsm_amd.ChannelStats(3).merge("other")


def test_dataset_stats_argument_errors(tmp_path):
    """Each fails before the loader is opened: the directory holds no frames."""
    with pytest.raises(ValueError, match="nonfinite"):
        nsm_amd.dataset_stats(str(tmp_path), nonfinite="ignore")
    with pytest.raises(ValueError, match="batch"):
        nsm_amd.dataset_stats(str(tmp_path), batch=0)
    with pytest.raises(ValueError, match="world"):
        nsm_amd.dataset_stats(str(tmp_path), world=2, rank=1)
    with pytest.raises(nsm_amd.NsmError):
        nsm_amd.dataset_stats(str(tmp_path), device="cpu")
    assert list(tmp_path.iterdir()) == []


def test_frame_loader_stats_argument_is_checked():
    from nsm_amd.data import _given_stats
    m, s = _given_stats(([0.5, 1.0], (2.0, 3.0)), 2)
    assert m.dtype == s.dtype == torch.float32 and m.tolist() == [0.5, 1.0] and s.tolist() == [2, 3]
    res = nsm_amd.StatsResult(None, torch.tensor([0.1, 0.2], dtype=torch.float64),
                              torch.tensor([1.0, 2.0], dtype=torch.float64), None, None, None)
    m, s = _given_stats(res, 2)
    assert torch.equal(m, torch.tensor([0.1, 0.2])) and torch.equal(s, torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError):
        _given_stats(res, 7)
    with pytest.raises(ValueError):
        _given_stats(3.0, 1)


def test_c_entry_points_reject_null_pointers():
    lib = L.lib
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    for rc in (lib.nsm_stats_partial(None, 1, 1, 16, p, None),
               lib.nsm_stats_partial(p, 1, 1, 16, None, None)):
        assert rc == 1 and "stats_partial" in L.last_error() and "null" in L.last_error()
    for rc in (lib.nsm_stats_merge(None, 1, 1, 1, None, p, None),
               lib.nsm_stats_merge(p, 1, 1, 1, None, None, None)):
        assert rc == 1 and "stats_merge" in L.last_error() and "null" in L.last_error()
    for args in ((0, 1, 16), (1, 0, 16), (1, 1, 0), (1, 1, 1 << 31)):
        assert lib.nsm_stats_partial(p, args[0], args[1], args[2], p, None) == 1
        assert "shape" in L.last_error()
    for args in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert lib.nsm_stats_merge(p, args[0], args[1], args[2], None, p, None) == 1
        assert "frames" in L.last_error()


def test_block_plan():
    lib = L.lib
    span = 32768
    assert [lib.nsm_stats_blocks(n) for n in (0, -1, 1 << 31)] == [0, 0, 0]
    for n in (1, span - 1, span, span + 1, 300 * 301, 512 * 512, 1080 * 1920, (1 << 31) - 1):
        assert lib.nsm_stats_blocks(n) == -(-n // span), n


def test_stats_json_shape_and_round_trip(tmp_path):
    """What dataset_stats writes: the reference's two keys, lists of Python
    floats at full float64 precision, indent 4; load_stats reads it."""
    means = torch.tensor([1000.0000123456789, -0.25, 1e-3], dtype=torch.float64)
    stds = np.array([0.0100123456789, 0.0, 1.5], dtype=np.float64)
    text = nsm_amd.stats_json(means, stds)
    d = json.loads(text)
    assert list(d) == ["means", "stds"]
    assert d["means"] == means.tolist() and d["stds"] == stds.tolist()
    assert all(type(v) is float for v in d["means"] + d["stds"])
    assert text == json.dumps({"means": means.tolist(), "stds": stds.tolist()}, indent=4)
    path = nsm_amd.save_stats(str(tmp_path), means, stds)
    assert [p.name for p in tmp_path.iterdir()] == ["train_stats.json"] and open(path).read() == text
    m, s = load_stats(str(tmp_path), 3)
    assert torch.equal(m, means.to(torch.float32))
    assert torch.equal(s, torch.from_numpy(stds).to(torch.float32))
    assert load_stats(str(tmp_path), 7) is None
    with pytest.raises(ValueError):
        nsm_amd.stats_json([1.0, 2.0], [1.0])


def test_result_std_forms():
    res = nsm_amd.StatsResult(torch.tensor([4, 1]), torch.zeros(2, dtype=torch.float64),
                              torch.tensor([3.0, 0.0], dtype=torch.float64), None, None, None)
    assert res.std(unbiased=False) is res.stds
    u = res.std()
    assert abs(u[0].item() - 3.0 * (4 / 3) ** 0.5) <= 1e-15 and torch.isnan(u[1])


def test_module_has_no_host_synchronisation_outside_dataset_stats():
    """ChannelStats never moves a value to the host; dataset_stats reads the
    non-finite counts once, at its end."""
    import inspect

    import nsm_amd.stats as S
    for obj in (S.ChannelStats, S.result_of, S.channel_stats, S.StatsResult):
        src = inspect.getsource(obj)
        for word in (".item(", ".cpu(", ".tolist(", "synchronize", ".numpy("):
            assert word not in src, (obj.__name__, word)
