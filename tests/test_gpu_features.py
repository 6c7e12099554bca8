"""GPU: G-buffer feature recipes (nsm_amd/features.py, compose_features in
nsm_amd/frames.py, csrc/nsm_features.hip) against feature_util.compose_ref, bit
for bit: the plain composition on unaligned rows, views and the all-16-byte
path, pad + scrub + stats + census, the identity recipe against prepare_frames,
the emitter offset, FramePipeline(recipe=...), dataset_stats(recipe=...) and
PatchSampler.from_dir(recipe=...), and determinism.

Every comparison is on the int32 view of the fp32 values (feature_util.same_bits:
-0.0 is not +0.0). The sign and payload of a NaN that an operation produced are
not IEEE 754's to fix and differ between x86 and gfx950, so such NaNs are
compared by position; raw terms, which move bits, are compared NaN bits and all,
and so is everything behind the scrub."""
import json

import numpy as np
import pytest
import torch

import feature_util as U
import frame_util as F
import stats_util as S
from oracle.weights import make_state
from test_gpu_model import build

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
FRAME = (2, 11, 41, 73)      # rows of 73 floats: three of four start off the 16-byte grid


def on(device, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def report_of(device, B):
    from nsm_amd.frames import new_report
    rep = new_report(B, device)
    rep.fill_(-7)
    return rep


# ---- 1. plain compose ---------------------------------------------------------------
@pytest.mark.parametrize("W", [73, 72], ids=["w73-narrow-rows", "w72-16-byte"])
def test_plain_compose(device, W):
    import nsm_amd
    r = U.recipe6()
    shape = FRAME[:3] + (W,)
    x = U.feature_input(shape)
    ref, census = U.compose_ref(x, r)
    assert census.min() > 0                                     # NaN, +Inf and -Inf are all made
    assert nsm_amd.lib.nsm_feature_blocks(6, 41, W) > 1         # more than one block an image
    got = nsm_amd.compose_features(on(device, x), r)
    assert got.shape == (2, 6, 41, W) and got.dtype == torch.float32
    assert U.same_bits(got, ref, exact=U.raw_channels(r), what=f"plain W={W}")
    # [C,H,W] input, and the census alone changes nothing
    rep = report_of(device, 2)
    again = nsm_amd.compose_features(on(device, x), r, report=rep)
    assert torch.equal(U.bits(again), U.bits(got))
    assert torch.equal(rep[:, :3].cpu(), torch.from_numpy(census)) and (rep[:, 3:] == -7).all()
    one = nsm_amd.compose_features(on(device, x[1]), r)
    assert one.shape == (1, 6, 41, W) and torch.equal(U.bits(one[0]), U.bits(got[1]))


@pytest.mark.parametrize("W", [73, 72])
def test_plain_compose_on_views(device, W):
    """x and out start one float inside a larger buffer: with W = 72 every row is
    then off the 16-byte grid, with W = 73 another three of four are."""
    import nsm_amd
    r = U.recipe6()
    shape = FRAME[:3] + (W,)
    x = U.feature_input(shape)
    ref, _ = U.compose_ref(x, r)
    xbuf = torch.zeros(x.size + 8, dtype=torch.float32, device=device)
    xv = xbuf[1:1 + x.size].view(shape)
    xv.copy_(on(device, x))
    obuf = torch.full((ref.size + 2 * 64 + 1,), SENTINEL, dtype=torch.float32, device=device)
    ov = obuf[65:65 + ref.size].view(ref.shape)
    assert xv.data_ptr() % 16 == 4 and ov.data_ptr() % 16 == 4 and ov.is_contiguous()
    assert nsm_amd.compose_features(xv, r, out=ov) is ov
    assert U.same_bits(ov, ref, exact=U.raw_channels(r), what=f"views W={W}")
    assert bool((obuf[:65] == SENTINEL).all()) and bool((obuf[65 + ref.size:] == SENTINEL).all())


def test_a_raw_channel_nothing_reads(device):
    """Five terms that leave `ce` out (z is read by three, zf by two): whatever
    that plane holds is not seen."""
    import nsm_amd
    r = nsm_amd.FeatureRecipe.parse(U.EXPRS[:5], layout=U.LAYOUT)
    assert r.in_channels == 11 and U.LAYOUT["ce"] not in r.planes_read()
    x = U.feature_input(FRAME)
    ref, census = U.compose_ref(x, r)
    x[:, U.LAYOUT["ce"]] = np.nan
    rep = report_of(device, 2)
    got = nsm_amd.compose_features(on(device, x), r, report=rep)
    assert U.same_bits(got, ref, exact=U.raw_channels(r), what="five terms")
    assert torch.equal(rep[:, :3].cpu(), torch.from_numpy(census))


# ---- 2. pad + scrub + stats + census ---------------------------------------------------
# 41 x 73 -> 48 x 80; 9 x 9 -> 16 x 16 (the longest reach of a reflection: 7 of 9);
# 2 x 2 -> 3 x 3 (row and column 2 are copies of 0); 1 x 1 unpadded
PADDED = [((2, 11, 41, 73), 16), ((2, 11, 9, 9), 16), ((1, 11, 2, 2), 3), ((2, 11, 1, 1), None)]


def full_case(device, shape, pad):
    import nsm_amd
    r = U.recipe6()
    x = U.feature_input(shape, pad_multiple=pad)
    stats = U.stats_for(6)
    Hp, Wp = F.padded(shape[2], pad), F.padded(shape[3], pad)
    ref, census = U.compose_ref(x, r, Hp, Wp, scrub=True, stats=stats)
    rep = report_of(device, shape[0])
    got = nsm_amd.compose_features(on(device, x), r, pad_multiple=pad, scrub=True,
                                   stats=(torch.from_numpy(stats[0]), torch.from_numpy(stats[1])),
                                   report=rep)
    return got, rep, ref, census


@pytest.mark.parametrize("shape,pad", PADDED, ids=["41x73", "9x9", "2x2", "1x1"])
def test_pad_scrub_stats_census(device, shape, pad):
    got, rep, ref, census = full_case(device, shape, pad)
    assert got.shape == ref.shape
    assert not np.isnan(ref).any()                              # the scrub took every NaN
    assert U.same_bits(got, ref, exact="all", what=f"full {shape}")
    assert torch.equal(rep[:, :3].cpu(), torch.from_numpy(census))   # reflected copies not counted
    assert (rep[:, 3:] == -7).all()
    if shape[2] >= 9:
        assert census.min() > 0


def test_reflection_limit_is_prepare_frames(device):
    """A 2 x 2 frame cannot be reflected to 16 x 16 (the pad must stay below the
    dimension, as nn.ReflectionPad2d and prepare_frames ask): the same error."""
    import nsm_amd
    x = torch.zeros(1, 11, 2, 2, device=device)
    with pytest.raises(ValueError, match="height"):
        nsm_amd.compose_features(x, U.recipe6(), pad_multiple=16)
    with pytest.raises(ValueError, match="height"):
        nsm_amd.prepare_frames(x, pad_multiple=16)


# ---- 3. identity equals the existing path -------------------------------------------------
def test_identity_equals_prepare_frames(device):
    import nsm_amd
    from nsm_amd.frames import new_report
    x = F.prep_input((2, 7, 41, 73)).to(device)
    g = torch.Generator().manual_seed(1)
    s = (torch.randn(7, generator=g), torch.rand(7, generator=g) + 0.5)
    r, r2 = new_report(2, device), new_report(2, device)
    a = nsm_amd.compose_features(x, nsm_amd.FeatureRecipe.identity(7), pad_multiple=16, scrub=True,
                                 stats=s, report=r)
    b = nsm_amd.prepare_frames(x, pad_multiple=16, scrub=True, stats=s, report=r2)
    assert a.shape == b.shape == (2, 7, 48, 80)
    assert torch.equal(U.bits(a), U.bits(b))
    assert torch.equal(r[:, :3], r2[:, :3]) and int(r[:, :3].min()) > 0
    raw = nsm_amd.compose_features(x, nsm_amd.FeatureRecipe.identity(7), pad_multiple=16)
    assert torch.equal(U.bits(raw), U.bits(nsm_amd.prepare_frames(x, pad_multiple=16, scrub=False)))


# ---- 4. emitter -------------------------------------------------------------------------
def test_emitter_changes_its_channel_only(device):
    import nsm_amd
    r = U.recipe6()
    x = U.feature_input(FRAME)
    xd = on(device, x)
    plain = nsm_amd.compose_features(xd, r)
    got = nsm_amd.compose_features(xd, r, emitter_channel=5, emitter=[0.0, 2.5])
    ref, _ = U.compose_ref(x, r, emitter_channel=5, emitter=[0.0, 2.5])
    assert U.same_bits(got, ref, exact=[0], what="emitter")
    assert torch.equal(U.bits(got[:, :5]), U.bits(plain[:, :5]))          # NaN bits and all
    assert int((U.bits(plain[:, 0]) == -2 ** 31).sum()) > 0               # a -0.0 went through
    fin = torch.isfinite(plain[1, 5])
    assert torch.equal(got[1, 5][fin], plain[1, 5][fin] + 2.5)
    assert not torch.equal(U.bits(got[1, 5]), U.bits(plain[1, 5]))
    # + 0.0 turns the channel's own -0.0 into +0.0 and changes nothing else
    zero = U.bits(plain[0, 5]) == -2 ** 31
    assert int(zero.sum()) > 0 and bool((U.bits(got[0, 5])[zero] == 0).all())
    assert torch.equal(U.bits(got[0, 5])[~zero], U.bits(plain[0, 5])[~zero])
    # a device tensor and a float say the same
    dev_e = torch.tensor([0.0, 2.5], device=device)
    assert torch.equal(U.bits(nsm_amd.compose_features(xd, r, emitter_channel=5, emitter=dev_e)),
                       U.bits(got))
    both = nsm_amd.compose_features(xd, r, emitter_channel=5, emitter=2.5)
    assert torch.equal(U.bits(both[1]), U.bits(got[1]))
    # behind the scrub and in front of the normalisation
    stats = U.stats_for(6)
    full, _ = U.compose_ref(x, r, 48, 80, scrub=True, stats=stats, emitter_channel=5,
                            emitter=[0.0, 2.5])
    got = nsm_amd.compose_features(xd, r, pad_multiple=16, scrub=True, stats=stats,
                                   emitter_channel=5, emitter=[0.0, 2.5])
    assert U.same_bits(got, full, exact="all", what="emitter, full")


# ---- 5. FramePipeline(recipe=...) ----------------------------------------------------------
def test_pipeline_with_a_recipe(device):
    import nsm_amd
    from nsm_amd.frames import new_report, report_dict
    r = U.recipe6()
    shape, size = (1, 11, 41, 73), (41, 73)
    x = U.mild_input(shape, seed=3)
    xd = on(device, x)
    g = torch.Generator().manual_seed(2)
    stats = (0.1 * torch.randn(6, generator=g), torch.rand(6, generator=g) + 0.5)
    np_stats = (stats[0].numpy(), stats[1].numpy())
    m = build(device, 6, 0.2, make_state(6, 42)).train()
    pipe = nsm_amd.FramePipeline(m, xd, recipe=r, emitter_channel=5, stats=stats, crop=True)
    assert m.training and pipe.raw.shape == shape and pipe.static_in.shape == (1, 6, 48, 80)
    assert pipe.emitter.shape == (1,) and float(pipe.emitter[0]) == 0.0

    def eager(e):
        rep = new_report(1, device)
        xin = nsm_amd.compose_features(xd, r, pad_multiple=16, scrub=True, stats=stats,
                                       emitter_channel=5, emitter=e, report=rep)
        m.eval()
        with torch.no_grad():
            o = m(xin)
        m.train()
        shadow = torch.empty((1, o.shape[1]) + size, dtype=torch.float32, device=device)
        u8 = nsm_amd.finish_frames(o, size, out_f32=shadow, report=rep)
        return xin, u8, shadow, rep

    xin, u8, shadow, rep = eager(0.0)
    got = pipe(xd)
    assert got.dtype == torch.uint8 and got.shape == (1,) + size and torch.equal(got, u8)
    assert torch.equal(U.bits(pipe.shadow), U.bits(shadow))
    assert torch.equal(U.bits(pipe.static_in), U.bits(xin))
    assert int(got.max()) > int(got.min())                                # not a blank frame
    ref0, census = U.compose_ref(x, r, 48, 80, scrub=True, stats=np_stats, emitter_channel=5,
                                 emitter=[0.0])
    assert U.same_bits(pipe.static_in, ref0, exact="all", what="pipeline input")
    d = pipe.report()
    assert d == report_dict(rep)
    assert [d["nan"], d["posinf"], d["neginf"]] == [[int(v)] for v in census[0]]
    assert census.min() > 0
    # a new emitter size: the same graph, replayed
    graph = pipe.graph
    assert pipe.set_emitter([3.0]) is pipe.emitter
    out3 = pipe.replay()
    assert pipe.graph is graph
    ref3, _ = U.compose_ref(x, r, 48, 80, scrub=True, stats=np_stats, emitter_channel=5,
                            emitter=[3.0])
    assert U.same_bits(pipe.static_in, ref3, exact="all", what="pipeline input, emitter 3")
    xin3, u83, shadow3, _ = eager(3.0)
    assert torch.equal(out3, u83) and torch.equal(U.bits(pipe.shadow), U.bits(shadow3))
    assert not torch.equal(U.bits(xin3[:, 5]), U.bits(xin[:, 5]))
    assert torch.equal(U.bits(xin3[:, :5]), U.bits(xin[:, :5]))
    pipe.set_emitter(0.0)
    assert torch.equal(pipe(xd), u8) and pipe.graph is graph


def test_pipeline_construction_errors(device):
    import nsm_amd
    r = U.recipe6()
    m = build(device, 6, 0.2, make_state(6, 42))
    z11, z7 = torch.zeros(1, 11, 41, 73, device=device), torch.zeros(1, 7, 41, 73, device=device)
    for kw, word in [(dict(example=z7, recipe=r), "11 raw channels, the frames have 7"),
                     (dict(example=z11, emitter_channel=5), "needs a recipe"),
                     (dict(example=z11, recipe=r, emitter_channel=6), "emitter_channel"),
                     (dict(example=z11, recipe=r, emitter_channel=True), "emitter_channel"),
                     (dict(example=z11, recipe="z-zf"), "FeatureRecipe"),
                     (dict(example=z11, recipe=r, stats=([0.0] * 11, [1.0] * 11)), "entries")]:
        with pytest.raises(ValueError, match=word):
            nsm_amd.FramePipeline(m, **kw)
    pipe = nsm_amd.FramePipeline(m, torch.zeros(1, 11, 32, 32, device=device), recipe=r, warmup=1)
    assert pipe.emitter is None
    with pytest.raises(ValueError, match="emitter_channel"):
        pipe.set_emitter(1.0)
    with pytest.raises(ValueError, match="captured for"):
        pipe(torch.zeros(1, 6, 32, 32, device=device))


# ---- 6. dataset_stats and PatchSampler.from_dir ------------------------------------------------
def test_stats_and_patch_pool_of_a_recipe(device, tmp_path, monkeypatch):
    import nsm_amd
    from nsm_amd import patches
    r = U.recipe6()
    x = U.mild_input((5, 11, 24, 40), seed=6)
    rng = np.random.default_rng(11)
    y = rng.random((5, 1, 24, 40))                                         # f64, as the reference writes
    np.save(tmp_path / "train_inputs.npy", x)
    np.save(tmp_path / "train_labels.npy", y)
    ref, census = U.compose_ref(x, r)
    assert census.min() > 0

    # the stats are those of the composed channels
    res = nsm_amd.dataset_stats(str(tmp_path), batch=2, device=device, save=False,
                                nonfinite="skip", recipe=r)
    acc = nsm_amd.ChannelStats(6)
    acc.update(on(device, ref))
    want = acc.compute()
    S.assert_matches(res.means.cpu().numpy(), res.stds.cpu().numpy(),
                     {"mean": want.means.cpu().numpy(), "std": want.stds.cpu().numpy()},
                     S.BOUND, "dataset_stats(recipe)")
    assert res.count.tolist() == want.count.tolist()
    bad = [int(v) for v in (~np.isfinite(ref)).sum(axis=(0, 2, 3))]
    assert res.nonfinite.tolist() == want.nonfinite.tolist() == bad and sum(bad) > 0
    assert torch.equal(res.mins, want.mins) and torch.equal(res.maxs, want.maxs)
    with pytest.raises(ValueError, match="non-finite"):
        nsm_amd.dataset_stats(str(tmp_path), batch=2, device=device, save=False, recipe=r)
    with pytest.raises(ValueError, match="raw channels"):
        nsm_amd.dataset_stats(str(tmp_path), batch=2, device=device, save=False,
                              recipe=nsm_amd.FeatureRecipe.identity(7))

    # the pool holds the composed channels, and samples like a pool built from them
    monkeypatch.setattr(patches, "UPLOAD_BYTES", 2 * 4 * 11 * 24 * 40)    # chunks of 2, 2 and 1 frames
    means, stds = [0.1, -0.2, 0.3, 1.5, 0.0, 0.5], [1.0, 0.5, 2.0, 0.25, 1.5, 1.0]
    (tmp_path / "train_stats.json").write_text(json.dumps({"means": means, "stds": stds}))
    kw = dict(patch=(16, 20), batch=4, seed=8, order="random", hflip=True,
              hflip_sign=[1, 1, 1, 1, -1, 1], emitter_channel=5, emitter_values=[1.5],
              record_draws=True)
    a = nsm_amd.PatchSampler.from_dir(str(tmp_path), device=device, recipe=r, **kw)
    assert a.inputs.shape == (5, 6, 24, 40) and a.C == 6
    assert U.same_bits(a.inputs, ref, exact=U.raw_channels(r), what="pool")
    b = nsm_amd.PatchSampler(on(device, ref), on(device, y.astype(np.float32)),
                             stats=(means, stds), **kw)
    assert torch.equal(a.labels, b.labels)
    assert torch.equal(a.means, b.means) and torch.equal(a.stds, b.stds)   # the file's six figures
    (xa, ya), (xb, yb) = a.next(), b.next()
    assert a.last_draws.tolist() == b.last_draws.tolist()
    assert xa.shape == (4, 6, 16, 20) and torch.equal(ya, yb)
    assert U.same_bits(xa.detach(), xb.detach(), what="patches")
    with pytest.raises(ValueError, match="raw channels"):
        nsm_amd.PatchSampler.from_dir(str(tmp_path), device=device,
                                      recipe=nsm_amd.FeatureRecipe.identity(7), **kw)


# ---- 7. determinism -------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(device):
    a, ra, _, _ = full_case(device, *PADDED[0])
    b, rb, _, _ = full_case(device, *PADDED[0])
    assert a.data_ptr() != b.data_ptr()
    assert torch.equal(U.bits(a), U.bits(b)) and torch.equal(ra, rb)


# ---- 8. argument checks ---------------------------------------------------------------------
def test_argument_checks(device):
    import nsm_amd
    r = U.recipe6()
    z = torch.zeros(2, 11, 17, 19, device=device)
    bad = [
        (dict(x=torch.zeros(17, 19, device=device)), "tensor"),
        (dict(x=z.double()), "float32"),
        (dict(x=z.cpu()), "GPU"),
        (dict(x=z[:, :7]), "11 raw channels, the frames have 7"),
        (dict(x=z, recipe=[0, 1]), "FeatureRecipe"),
        (dict(x=z, stats=([0.0] * 11, [1.0] * 11)), "entries"),           # stats are the composed ones
        (dict(x=z, pad_multiple=0), "pad_multiple"),
        (dict(x=z, out=torch.zeros(2, 11, 17, 19, device=device)), "out"),
        (dict(x=z, report=torch.zeros(1, 6, dtype=torch.int32, device=device)), "report"),
        (dict(x=z, emitter_channel=5), "go together"),
        (dict(x=z, emitter=1.0), "go together"),
        (dict(x=z, emitter_channel=6, emitter=1.0), "emitter_channel"),
        (dict(x=z, emitter_channel=5, emitter=[1.0, 2.0, 3.0]), "emitter"),
        (dict(x=z, emitter_channel=5, emitter=torch.zeros(3, device=device)), "emitter"),
        (dict(x=z, emitter_channel=5, emitter="soft"), "emitter"),
    ]
    for kw, word in bad:
        x = kw.pop("x")
        rec = kw.pop("recipe", r)
        with pytest.raises(ValueError, match=word):
            nsm_amd.compose_features(x, rec, **kw)
    assert nsm_amd.compose_features(z, r).shape == (2, 6, 17, 19)
