"""GPU: the inference frame path (nsm_amd/frames.py, csrc/nsm_frame.hip) against
the CPU oracle of frame_util: prepare_frames and finish_frames bitwise, their
census, that neither writes outside its outputs, and FramePipeline against the
hand composition of the same calls."""
import pytest
import torch

import frame_util as U
from oracle.weights import make_state
from test_gpu_model import build

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def same_bits(a, b):
    """torch.equal, and the sign of zero as well (fp32)."""
    return torch.equal(a, b) and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1. prep, bitwise ------------------------------------------------------------
@pytest.mark.parametrize("scrub", [True, False], ids=["scrub", "raw"])
@pytest.mark.parametrize("shape", U.PREP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prep_equals_oracle(device, shape, scrub):
    import nsm_amd
    x = U.prep_input(shape)
    ref = U.prep_ref(x, scrub_on=scrub)
    got = nsm_amd.prepare_frames(x.to(device), scrub=scrub).cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32
    if scrub:
        assert torch.isfinite(got).all()            # the padded copies of a NaN too
        assert same_bits(got, ref)
    else:                                           # NaN != NaN: compare the bits
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def test_prep_3d_input_and_no_padding(device):
    import nsm_amd
    x = U.prep_input((1, 4, 17, 19))
    for m in (None, 1):
        got = nsm_amd.prepare_frames(x[0].to(device), pad_multiple=m)
        assert got.shape == (1, 4, 17, 19) and same_bits(got.cpu(), U.scrub(x))
    got = nsm_amd.prepare_frames(x.to(device), pad_multiple=5)      # 20 x 20: rows of 80 bytes
    assert same_bits(got.cpu(), U.prep_ref(x, pad_multiple=5))
    got = nsm_amd.prepare_frames(x.to(device), pad_multiple=7)      # 21 x 21: no row aligned
    assert same_bits(got.cpu(), U.prep_ref(x, pad_multiple=7))


# ---- 2. prep with stats ------------------------------------------------------------
def stats_for(C, seed=1):
    """Per-channel figures with a std of 0 (a division by eps) in channel 0 and
    a depth-like channel (1000 +- 0.01) last (when C > 1)."""
    g = torch.Generator().manual_seed(seed)
    means, stds = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    stds[0] = 0.0
    if C > 1:
        means[C - 1], stds[C - 1] = 1000.0, 0.01
    return means, stds


@pytest.mark.parametrize("shape", U.PREP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prep_with_stats(device, shape):
    """Bitwise the training loader's nsm_normalize_frames on test 1's result,
    and within 1 ulp of the CPU's fp32 (v - mean) / (std + eps). Measured on
    the MI355X: the worst case is 0 ulp for every shape (both divisions are
    correctly rounded), printed below."""
    import nsm_amd
    from nsm_amd._lib import call, ptr, stream
    B, C, H, W = shape
    x = U.prep_input(shape)
    if C > 1:
        x[:, C - 1] = 1000.0 + 0.01 * x[:, C - 1]            # NaN and +-Inf stay what they are
    means, stds = stats_for(C)
    got = nsm_amd.prepare_frames(x.to(device), stats=(means, stds))
    # the loader's kernel, in place on the un-normalised result
    plain = nsm_amd.prepare_frames(x.to(device))
    dmeans, dstds = means.to(device), stds.to(device)
    call("nsm_normalize_frames", ptr(plain), B, C, plain.shape[2] * plain.shape[3],
         ptr(dmeans), ptr(dstds), U.EPS, stream())
    assert same_bits(got, plain)
    # a StatsResult-like object and a list pair convert the same way
    class Res:
        pass
    r = Res()
    r.means, r.stds = means.double(), stds.double()
    assert same_bits(nsm_amd.prepare_frames(x.to(device), stats=r), got)
    ref = U.prep_ref(x, stats=(means, stds))
    got = got.cpu()
    assert not torch.isnan(ref).any() and not torch.isnan(got).any()   # FLT_MAX / eps is Inf in both
    # distance in units of the last place: the fp32 patterns as ordered integers
    def ordered(t):
        i = t.view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    ulp = (ordered(got) - ordered(ref)).abs().max().item()
    print(f"prep with stats {shape}: worst distance from the CPU expression {ulp} ulp")
    assert ulp <= 1


def test_prep_stats_from_directory(device, tmp_path):
    import nsm_amd
    x = U.prep_input((1, 4, 17, 19))
    means, stds = stats_for(4)
    nsm_amd.save_stats(str(tmp_path), means, stds)
    a = nsm_amd.prepare_frames(x.to(device), stats=str(tmp_path))
    assert same_bits(a, nsm_amd.prepare_frames(x.to(device), stats=(means, stds)))


# ---- 3. prep census --------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 7, 33, 48), (3, 4, 17, 19), (2, 1, 20, 66)],
                         ids=lambda s: "x".join(map(str, s)))
def test_prep_census(device, shape):
    import nsm_amd
    from nsm_amd.frames import new_report, report_dict
    x = U.prep_input(shape, clean_image=shape[0] - 1)
    want = U.prep_census(x)
    assert want[:-1].min() > 0 and want[-1].sum() == 0           # every kind met; one image clean
    for m in (16, None, 32):
        rep = new_report(shape[0], device)
        rep.fill_(-7)
        out = nsm_amd.prepare_frames(x.to(device), pad_multiple=m, report=rep)
        assert torch.equal(rep[:, :3].cpu(), want), m           # padded copies are not counted
        assert (rep[:, 3:] == -7).all()                         # the finish half is not prep's
        assert same_bits(out.cpu(), U.prep_ref(x, pad_multiple=m))
    d = report_dict(rep)
    assert d["nan"] == want[:, 0].tolist() and d["neginf"] == want[:, 2].tolist()


def test_prep_census_many_blocks(device):
    """More blocks per image than the finalize has threads (per > 256)."""
    import nsm_amd
    from nsm_amd.frames import new_report
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 601, 640, generator=g)
    idx = torch.randperm(x[0].numel(), generator=g)
    x[0].view(-1)[idx[:1000]] = float("nan")
    x[0].view(-1)[idx[1000:1700]] = float("inf")
    x[1].view(-1)[idx[:300]] = float("-inf")
    rep = new_report(2, device)
    nsm_amd.prepare_frames(x.to(device), report=rep)
    assert rep[:, :3].tolist() == [[1000, 700, 0], [0, 0, 300]]


# ---- 4. finish, bitwise ------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("full,size", U.FINISH_CROPS,
                         ids=[f"{a}x{b}-{'full' if s is None else 'x'.join(map(str, s))}"
                              for (a, b), s in U.FINISH_CROPS])
def test_finish_equals_oracle(device, C, full, size):
    import nsm_amd
    o = U.finish_input(C, *full, size)
    u8_ref, f32_ref = U.finish_ref(o, size)
    B, (H, W) = o.shape[0], (size or full)
    f32 = torch.empty((B, C, H, W), dtype=torch.float32, device=device)
    u8 = nsm_amd.finish_frames(o.to(device), size, out_f32=f32)
    assert u8.dtype == torch.uint8
    assert u8.shape == ((B, H, W) if C == 1 else (B, H, W, C))   # channels last
    assert torch.equal(u8.cpu(), u8_ref)
    assert torch.equal(f32.cpu(), f32_ref)
    # each alone: the fp32 frame without the bytes, and the bytes without it
    assert torch.equal(nsm_amd.finish_frames(o.to(device), size, quantize=False), f32)
    assert torch.equal(nsm_amd.finish_frames(o.to(device), size), u8)
    if C > 1:                                                    # byte c of a pixel is channel c
        for c in range(C):
            assert torch.equal(u8[..., c].cpu(), (f32_ref[:, c] * 255).to(torch.uint8))


def test_finish_odd_sizes(device):
    """No padding at all: rows of the source and of both outputs unaligned."""
    import nsm_amd
    for C, hw in ((1, (17, 19)), (3, (9, 21)), (4, (5, 7)), (1, (40, 3))):
        o = U.finish_input(C, *hw)
        u8_ref, f32_ref = U.finish_ref(o)
        assert torch.equal(nsm_amd.finish_frames(o.to(device)).cpu(), u8_ref)
        assert torch.equal(nsm_amd.finish_frames(o[0].to(device), quantize=False).cpu(),
                           f32_ref[:1])


# ---- 5. finish census --------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 4])
def test_finish_census_counts_the_crop_only(device, C):
    import nsm_amd
    from nsm_amd.frames import new_report
    full, size = (32, 80), (20, 66)
    o = U.finish_input(C, *full, size)
    want = U.finish_census(o, size)
    o[..., 20:, :] = float("nan")                     # the cropped-away margin
    o[..., :, 66:] = 7.0
    o[..., 25:, 70:] = float("-inf")
    assert torch.equal(U.finish_census(o, size), want) and want.sum(0).min() > 0
    rep = new_report(o.shape[0], device)
    rep.fill_(-7)
    nsm_amd.finish_frames(o.to(device), size, report=rep)
    assert torch.equal(rep[:, 3:].cpu(), want)
    assert (rep[:, :3] == -7).all()
    rep_full = new_report(o.shape[0], device)
    nsm_amd.finish_frames(o.to(device), report=rep_full)
    assert torch.equal(rep_full[:, 3:].cpu(), U.finish_census(o))


# ---- 6. guard ----------------------------------------------------------------------
def carve(numel, dtype, device, lead):
    """A contiguous run of `numel` elements `lead` elements into a sentinel-filled tensor."""
    big = torch.full((numel + 2 * 64 + lead,), SENTINEL if dtype.is_floating_point else 0xA5,
                     dtype=dtype, device=device)
    return big, big[64 + lead:64 + lead + numel]


def untouched(big, lead, numel, fill):
    return bool((big[:64 + lead] == fill).all()) and bool((big[64 + lead + numel:] == fill).all())


@pytest.mark.parametrize("lead", [0, 1, 3])
def test_nothing_outside_the_outputs_is_written(device, lead):
    """lead: the outputs start 0, 1 or 3 elements off the allocation's alignment."""
    import nsm_amd
    for shape in ((1, 4, 17, 19), (2, 1, 20, 66)):
        x = U.prep_input(shape)
        ref = U.prep_ref(x)
        big, run = carve(ref.numel(), torch.float32, device, lead)
        nsm_amd.prepare_frames(x.to(device), out=run.view(ref.shape))
        assert same_bits(run.view(ref.shape).cpu(), ref)
        assert untouched(big, lead, ref.numel(), SENTINEL)
    for C, full, size in ((1, (32, 32), (17, 19)), (3, (32, 32), (17, 19)), (4, (32, 80), (20, 66))):
        o = U.finish_input(C, *full, size)
        u8_ref, f32_ref = U.finish_ref(o, size)
        big8, run8 = carve(u8_ref.numel(), torch.uint8, device, lead)
        bigf, runf = carve(f32_ref.numel(), torch.float32, device, lead)
        nsm_amd.finish_frames(o.to(device), size, out_u8=run8.view(u8_ref.shape),
                              out_f32=runf.view(f32_ref.shape))
        assert torch.equal(run8.view(u8_ref.shape).cpu(), u8_ref)
        assert torch.equal(runf.view(f32_ref.shape).cpu(), f32_ref)
        assert untouched(big8, lead, u8_ref.numel(), 0xA5)
        assert untouched(bigf, lead, f32_ref.numel(), SENTINEL)


# ---- 7. / 8. pipeline ----------------------------------------------------------------
def raw_frames(shape, seed, device, nans=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    for b in range(shape[0]):
        idx = torch.randperm(x[b].numel(), generator=g)[:nans * (b + 1)]
        x[b].view(-1)[idx] = float("nan")
    return x.to(device)


def compose(m, x, stats, size, report=None):
    """The hand composition: prepare_frames -> eval forward -> finish_frames."""
    import nsm_amd
    was = m.training
    m.eval()
    with torch.no_grad():
        o = m(nsm_amd.prepare_frames(x, stats=stats, report=report))
    m.train(was)
    shadow = torch.empty((o.shape[0], o.shape[1]) + tuple(size), dtype=torch.float32,
                         device=o.device)
    u8 = nsm_amd.finish_frames(o, size, out_f32=shadow, report=report)
    return u8, shadow


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,padded", [((1, 7, 90, 150), (96, 160)), ((2, 4, 61, 64), (64, 64))],
                         ids=["1x7x90x150", "2x4x61x64"])
def test_pipeline_equals_composition(device, shape, padded, dtype):
    import nsm_amd
    from nsm_amd.frames import new_report, report_dict
    C = shape[1]
    m = build(device, C, 0.2, make_state(C, 42)).train().set_compute_dtype(dtype)
    g = torch.Generator().manual_seed(2)
    stats = (0.1 * torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5)
    x1, x2 = raw_frames(shape, 11, device), raw_frames(shape, 12, device, nans=3)
    for crop in (False, True):
        size = shape[2:] if crop else padded
        pipe = nsm_amd.FramePipeline(m, x1, stats=stats, crop=crop)
        assert m.training                                   # the capture restores the mode
        assert pipe.raw.shape == shape and pipe.static_in.shape == shape[:2] + padded
        for x in (x1, x2):
            u8, shadow = compose(m, x, stats, size)
            got = pipe(x)
            assert got.dtype == torch.uint8 and got.shape == (shape[0],) + tuple(size)
            assert torch.equal(got, u8)
            assert same_bits(pipe.shadow, shadow)
        assert int(got.max()) > int(got.min())              # not a blank frame
        # the caller writes the raw buffer itself
        pipe.raw.copy_(x1)
        u8, shadow = compose(m, x1, stats, size)
        assert torch.equal(pipe.replay(), u8) and same_bits(pipe.shadow, shadow)
        # the census of a frame with planted NaNs
        rep = new_report(shape[0], device)
        compose(m, x2, stats, size, report=rep)
        pipe(x2)
        got = pipe.report()
        assert got == report_dict(rep)
        assert got["nan"] == [3 * (b + 1) for b in range(shape[0])] and got["posinf"] == [0] * shape[0]


def test_pipeline_follows_weight_changes(device):
    """An in-place change of a parameter shows in the next call (GraphedUnet's
    version-counter refresh), and re-homed parameters are refused."""
    import nsm_amd
    shape, size = (1, 7, 90, 150), (90, 150)
    m = build(device, 7, 0.2, make_state(7, 42))
    x = raw_frames(shape, 21, device)
    pipe = nsm_amd.FramePipeline(m, x, crop=True)
    assert pipe.frozen is not None
    before = pipe(x).clone()
    assert torch.equal(before, compose(m, x, None, size)[0])
    vers = list(pipe._vers)
    with torch.no_grad():
        m.conv6.conv[0].weight.mul_(1.5)
        m.conv3.conv[5].bias.add_(0.25)
    u8, shadow = compose(m, x, None, size)
    after = pipe(x)
    assert pipe._vers != vers                               # went through refresh()
    assert torch.equal(after, u8) and same_bits(pipe.shadow, shadow)
    assert not torch.equal(after, before)
    nsm_amd.FlatAdamW(m.parameters())                       # re-homes every parameter
    with pytest.raises(RuntimeError, match="re-allocated"):
        pipe(x)


# ---- 9. argument checks --------------------------------------------------------------
def test_argument_checks(device):
    import nsm_amd
    from nsm_amd.frames import new_report
    z = torch.zeros(1, 4, 17, 19, device=device)
    bad_prep = [
        (dict(x=torch.zeros(17, 19, device=device)), "tensor"),                     # rank
        (dict(x=torch.zeros(1, 1, 4, 17, 19, device=device)), "tensor"),
        (dict(x=z.double()), "float32"),
        (dict(x=z.cpu()), "GPU"),
        (dict(x=z, stats=([0.0] * 3, [1.0] * 3)), "entries"),                       # stats length
        (dict(x=z, stats=(torch.zeros(4), torch.ones(5))), "entries"),
        (dict(x=z, pad_multiple=0), "pad_multiple"),
        (dict(x=z, pad_multiple=-16), "pad_multiple"),
        (dict(x=torch.zeros(1, 4, 2, 33, device=device)), "height"),                # pad 14 >= 2
        (dict(x=torch.zeros(1, 4, 33, 2, device=device)), "width"),
        (dict(x=z, out=torch.zeros(1, 4, 32, 33, device=device)), "out"),
        (dict(x=z, report=torch.zeros(2, 6, dtype=torch.int32, device=device)), "report"),
    ]
    for kw, word in bad_prep:
        x = kw.pop("x")
        with pytest.raises(ValueError, match=word):
            nsm_amd.prepare_frames(x, **kw)
    o = torch.zeros(1, 1, 32, 32, device=device)
    bad_finish = [
        (dict(out=torch.zeros(32, 32, device=device)), "tensor"),
        (dict(out=o.half()), "float32"),
        (dict(out=o.cpu()), "GPU"),
        (dict(out=torch.zeros(1, 2, 32, 32, device=device)), "channels"),
        (dict(out=torch.zeros(1, 7, 32, 32, device=device)), "channels"),
        (dict(out=o, size=(33, 32)), "crop"),
        (dict(out=o, size=(32, 40)), "crop"),
        (dict(out=o, size=(0, 4)), "crop"),
        (dict(out=o, size=17), "size"),
        (dict(out=o, out_u8=torch.zeros(1, 32, 32, 1, dtype=torch.uint8, device=device)), "out_u8"),
        (dict(out=o, out_f32=torch.zeros(1, 1, 32, 31, device=device)), "out_f32"),
    ]
    for kw, word in bad_finish:
        out = kw.pop("out")
        with pytest.raises(ValueError, match=word):
            nsm_amd.finish_frames(out, **kw)
    m = build(device, 4, 0.2, make_state(4, 42))
    for kw, word in [(dict(example=z[0]), "example"), (dict(example=z.cpu()), "GPU"),
                     (dict(example=z.double()), "float32"),
                     (dict(example=z, pad_multiple=0), "pad_multiple"),
                     (dict(example=torch.zeros(1, 4, 2, 33, device=device)), "height"),
                     (dict(example=z, stats=([0.0] * 7, [1.0] * 7)), "entries")]:
        with pytest.raises(ValueError, match=word):
            nsm_amd.FramePipeline(m, **kw)
    pipe = nsm_amd.FramePipeline(m, torch.zeros(1, 4, 61, 64, device=device), warmup=1)
    for x in (torch.zeros(1, 4, 64, 64, device=device), torch.zeros(2, 4, 61, 64, device=device),
              torch.zeros(1, 4, 61, 64, device=device, dtype=torch.float64),
              torch.zeros(1, 4, 61, 64)):
        with pytest.raises(ValueError, match="captured for"):
            pipe(x)
    assert pipe(torch.zeros(1, 4, 61, 64, device=device)).shape == (1, 64, 64)
