"""CPU: the draws of the training-patch sampler. nsm_amd.patches restates them
on the host (PatchSampler.draws, no GPU); patch_util restates them again with
no import from the package. Both must agree exactly, and the stream itself must
be in range, on the align grid and uniform."""
import math

import numpy as np
import pytest
import torch

import patch_util as U

N, C, H, W = 40, 3, 37, 53          # 37 - 16 + 1 = 22 and 53 - 16 + 1 = 38 offsets
SEEDS = (0, 1234, 2 ** 63 + 5)
# 99.9 % quantiles of chi-square by degrees of freedom
CHI2_999 = {1: 10.83, 4: 18.47, 21: 46.8, 37: 69.3}


def sampler(**kw):
    from nsm_amd.patches import PatchSampler
    E = kw.pop("E", 1)
    return PatchSampler(torch.zeros(N, C, H, W), torch.zeros(N, E, H, W), **kw)


@pytest.mark.parametrize("order", ["sequential", "random"])
@pytest.mark.parametrize("rank", [0, 3])
@pytest.mark.parametrize("seed", SEEDS)
def test_host_draws_equal_restatement(seed, rank, order):
    kw = dict(patch=(16, 20), batch=8, seed=seed, order=order, align=2, hflip=True, vflip=True,
              emitter_channel=1, emitter_values=[0.0, 1.0, 2.0, 3.0, 4.0], world=4, rank=rank, E=5)
    s = sampler(**kw)
    lo, count = U.shard(N, 4, rank)
    assert (s.lo, s.count) == (lo, count) == (10 * rank, 10)
    for step in (0, 1, 10 ** 6):
        got = s.draws(step)
        ref = U.draws(seed, rank, step, 8, frame=(H, W), patch=(16, 20), lo=lo, count=count,
                      order=order, align=2, hflip=True, vflip=True, emitters=5)
        assert got.dtype == torch.int32 and tuple(got.shape) == (8, 8)
        assert np.array_equal(got.numpy(), ref), (seed, rank, step, order)
        d = ref
        assert ((d[:, 0] >= lo) & (d[:, 0] < lo + count)).all()
        assert ((d[:, 1] >= 0) & (d[:, 1] <= H - 16) & (d[:, 1] % 2 == 0)).all()
        assert ((d[:, 2] >= 0) & (d[:, 2] <= W - 20) & (d[:, 2] % 2 == 0)).all()
        assert np.isin(d[:, 3:5], (0, 1)).all() and ((d[:, 5] >= 0) & (d[:, 5] < 5)).all()
        assert not d[:, 6:].any()


def test_module_function_is_the_method():
    from nsm_amd import patch_draws
    s = sampler(patch=(16, 16), batch=5, seed=7, order="random", world=2, rank=1)
    a = patch_draws(7, 1, 3, 5, frame=(H, W), patch=(16, 16), lo=s.lo, count=s.count, order="random")
    assert torch.equal(a, s.draws(3))


@pytest.mark.parametrize("seed", SEEDS)
def test_range_one_draws_zero(seed):
    """A whole-frame patch, one frame, one emitter, flips disabled: all zero."""
    d = U.draws(seed, 0, 12345, 64, frame=(H, W), patch=(H, W), lo=0, count=1, order="random")
    assert not d.any()
    from nsm_amd.patches import PatchSampler
    s = PatchSampler(torch.zeros(1, C, H, W), torch.zeros(1, 1, H, W), patch=(H, W), batch=64,
                     seed=seed, order="random")
    assert not s.draws(12345).any()


def test_disabled_flip_is_zero():
    for hf, vf in ((True, False), (False, True)):
        d = U.draws(1234, 0, 0, 256, frame=(H, W), patch=(16, 16), lo=0, count=N, hflip=hf, vflip=vf)
        assert d[:, 3].any() == hf and d[:, 4].any() == vf


def test_sequential_order_walks_the_shard():
    lo, count = U.shard(N, 4, 3)
    frames = np.concatenate([U.draws(1234, 3, t, 8, frame=(H, W), patch=(16, 16), lo=lo,
                                     count=count)[:, 0] for t in range(5)])
    assert frames.tolist() == [lo + n % count for n in range(40)]
    s = sampler(patch=(16, 16), batch=8, seed=1234, world=4, rank=3)
    assert torch.cat([s.draws(t)[:, 0] for t in range(5)]).tolist() == frames.tolist()


def test_draws_are_uniform():
    """Seed 1234, 8192 samples (1024 steps of 8). Offsets over 22 and 38 positions,
    the flip bits, the frame over 38 and the emitter index over 5: chi-square below
    the 99.9 % quantile of its degrees of freedom. The coincidences oy == ox and
    the equal ox draws of ranks 0 and 1 both have probability 1/38 per sample:
    within 4 sigma of 8192/38."""
    kw = dict(frame=(H, W), patch=(16, 16), lo=0, count=38, order="random", hflip=True, vflip=True,
              emitters=5)
    d = U.draws(1234, 0, 0, 8192, **kw)
    assert np.array_equal(d[:16], np.concatenate([U.draws(1234, 0, t, 8, **kw) for t in (0, 1)]))
    stats = {"oy": (d[:, 1], 22), "ox": (d[:, 2], 38), "hflip": (d[:, 3], 2), "vflip": (d[:, 4], 2),
             "emitter": (d[:, 5], 5), "frame": (d[:, 0], 38)}
    for name, (col, m) in stats.items():
        x2 = U.chi2(np.bincount(col, minlength=m))
        print(f"{name}: chi2 {x2:.1f} on {m - 1} degrees of freedom")
        assert x2 < CHI2_999[m - 1], (name, x2)
    x2 = U.chi2(np.bincount(2 * d[:, 3] + d[:, 4], minlength=4))      # the two bits jointly
    assert x2 < 16.27, x2                                             # 3 degrees of freedom
    d1 = U.draws(1234, 1, 0, 8192, **kw)
    exp, sigma = 8192 / 38, math.sqrt(8192 * (1 / 38) * (37 / 38))
    for name, hits in (("oy == ox", int((d[:, 1] == d[:, 2]).sum())),
                       ("rank 0 ox == rank 1 ox", int((d[:, 2] == d1[:, 2]).sum()))):
        print(f"{name}: {hits} of 8192, expected {exp:.1f} +- {sigma:.1f}")
        assert abs(hits - exp) < 4 * sigma, (name, hits)


def test_argument_errors():
    with pytest.raises(ValueError, match="does not fit"):
        sampler(patch=(38, 16))
    with pytest.raises(ValueError, match="channels"):
        sampler(patch=(16, 16), stats=([0.0] * 4, [1.0] * 4))
    with pytest.raises(ValueError, match="emitter_values has 3"):
        sampler(patch=(16, 16), emitter_channel=1, emitter_values=[0.0, 1.0, 2.0], E=5)
    with pytest.raises(ValueError, match="go together"):
        sampler(patch=(16, 16), emitter_channel=1)
    with pytest.raises(ValueError, match="ROCm GPU"):
        sampler(patch=(16, 16)).next()


def test_entry_point_rejects_before_any_launch():
    """nsm_patch_gather validates before it launches (no GPU here, the pointers
    are never followed): a frame beyond 32-bit offsets, a patch larger than the
    frame, align 0, an emitter channel outside [-1, C), an empty shard."""
    import nsm_amd._lib as L
    p = 4096                     # any aligned non-null address

    def rc(C=7, Ew=1, Hh=64, Ww=64, ph=16, pw=16, align=1, ech=-1, ev=None, lo=0, count=4, Nn=4):
        return L.lib.nsm_patch_gather(p, p, Nn, C, Ew, Hh, Ww, 2, ph, pw, p, p, 0.0, None, None, ech,
                                      ev, 0, align, 0, 0, lo, count, 0, 0, None, 0, None, p, p, None,
                                      None)

    for kw, word in ((dict(Hh=32768, Ww=16384), "32-bit"), (dict(Ew=40, Hh=8192, Ww=8192), "32-bit"),
                     (dict(ph=65), "does not fit"), (dict(pw=65), "does not fit"),
                     (dict(align=0), "align"), (dict(ech=7, ev=p), "emitter_channel"),
                     (dict(ech=-2), "emitter_channel"), (dict(ech=3), "go together"),
                     (dict(count=0), "shard"), (dict(lo=2, count=3), "shard"),
                     (dict(C=257), "channels")):
        assert rc(**kw) == 1, kw
        assert word in L.last_error(), (kw, L.last_error())
    assert L.lib.nsm_patch_advance(None, None) == 1 and "null" in L.last_error()


def test_state_dict_roundtrip_on_host():
    s = sampler(patch=(16, 16), batch=4, seed=2 ** 63 + 5, order="random", world=2, rank=1)
    s._step = 9
    st = s.state_dict()
    assert st == {"seed": 2 ** 63 + 5, "step": 9, "order": "random", "rank": 1}
    t = sampler(patch=(16, 16), batch=4, seed=0, order="random", world=2, rank=1)
    t.load_state_dict(st)
    assert t.state_dict() == st and torch.equal(t.draws(t.step), s.draws(9))
    with pytest.raises(ValueError):
        sampler(patch=(16, 16), batch=4, order="sequential", world=2, rank=1).load_state_dict(st)
