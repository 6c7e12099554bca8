"""CPU: the comparator of the temporal anti-aliasing tests (taa_util.py: the
resolve restated with plain torch indexing on temporal_util's lookup), its exact
properties in float32, the agreement of its float32 and float64 verdicts on
every seeded case, and what needs no device: the exports and the refusals of
nsm_taa_resolve and of the Python entry points.

The reference repository has no TAA pass, so no fixture comes from it."""
import math

import pytest
import torch

import taa_util as A

torch.set_num_threads(16)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- the restatement's exact properties (float32) --------------------------------
@pytest.mark.parametrize("clamp", (True, False))
def test_translation_reproduces_the_frames(clamp):
    """Frame t is frame t-1 rolled and the motion vectors undo the roll: the
    history equals the frame wherever it is accepted, so every output is its
    input bit for bit."""
    frames, mvs = A.translation_case()
    for dtype in (torch.float32, torch.float64):
        out, acc, _ = A.resolve(frames, mvs, clamp=clamp, dtype=dtype)
        assert same(out, [f.to(dtype) for f in frames])
        B, C, H, W = frames[0].shape
        assert all(a.sum().item() == B * (H - 2) * (W - 3) for a in acc[1:])
        assert not acc[0].any()


@pytest.mark.parametrize("clamp", (True, False))
def test_static_sequence_and_full_blend_return_the_input(clamp):
    frames, mvs, z, n = A.inputs((2, 1, 19, 37), "gauss")
    still = [frames[0]] * A.T
    out, acc, _ = A.resolve(still, None, clamp=clamp, dtype=torch.float32)
    assert same(out, still) and all(a.all() for a in acc[1:])
    out, _, _ = A.resolve(still, [torch.zeros_like(m) for m in mvs], clamp=clamp, dtype=torch.float32)
    assert same(out, still)
    out, acc, _ = A.resolve(frames, mvs, depth=z, normals=n, blend=1.0, clamp=clamp,
                            dtype=torch.float32)
    assert same(out, frames) and acc[1].any() and not acc[1].all()


@pytest.mark.parametrize("blend", A.BLENDS)
def test_constant_frame_after_a_checkerboard(blend):
    """The clamp confines the history to the frame's neighbourhood: exactly 0.5;
    without it the history shows through: 0.5 + (1 - blend)(h - 0.5)."""
    frames = A.constant_case()
    out, _, changed = A.resolve(frames, None, blend=blend, dtype=torch.float32)
    assert (out[1] == 0.5).all() and changed[1] == 1.0
    out, _, _ = A.resolve(frames, None, blend=blend, clamp=False, dtype=torch.float32)
    keep = 1 - torch.tensor(blend, dtype=torch.float32)
    assert torch.equal(out[1], 0.5 + keep * (frames[0] - 0.5))
    assert (out[1] != 0.5).all()


@pytest.mark.parametrize("shape,family,reject,clamp,blend", A.CASES, ids=A.IDS)
def test_masks_agree_between_float32_and_float64(shape, family, reject, clamp, blend):
    """Zero mismatches: the seeded inputs keep every verdict at least 1e-4 from
    its threshold (test_temporal_ref.test_decision_margins)."""
    _, (o64, a64, _), (o32, a32, _) = A.reference(shape, family, reject, clamp, blend)
    assert same(a64, a32)
    share = torch.stack(a64[1:]).float().mean().item()
    assert 0.1 < share < 0.97
    worst = max((a.double() - b).abs().max().item() for a, b in zip(o32, o64))
    assert worst < 1e-5


def test_clamp_is_exercised_both_ways():
    """On the seeded (2,1,67,129) Gaussian case the clamp changes some of the
    history samples and leaves others alone, in every frame."""
    _, (_, _, changed), _ = A.reference((2, 1, 67, 129), "gauss", False, True, 0.1)
    assert all(0.01 < c < 0.99 for c in changed[1:]), changed


def test_bounds_replicate_the_edges():
    img = torch.rand(2, 3, 5, 7, dtype=torch.float64)
    lo, hi = A.bounds(img)
    for y, x in ((0, 0), (4, 6), (2, 0), (0, 3), (3, 4)):
        win = img[:, :, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2]
        assert torch.equal(lo[:, :, y, x], win.amin((2, 3)))
        assert torch.equal(hi[:, :, y, x], win.amax((2, 3)))
    for shape in ((1, 1, 1, 7), (1, 2, 5, 1)):
        lo, hi = A.bounds(torch.rand(shape))
        assert lo.shape == hi.shape == shape


# ---- without a device: exports and refusals --------------------------------------
def test_exports():
    import nsm_amd
    import nsm_amd._lib as L
    assert hasattr(L.lib, "nsm_taa_resolve") and "nsm_taa_resolve" in L.symbols()
    for name in ("taa_resolve", "temporal_aa", "TemporalAA"):
        assert callable(getattr(nsm_amd, name))


def test_entry_point_refusals_need_no_gpu():
    """Argument validation fails before any launch, with a readable message
    (the pointers are dummies: nothing dereferences them)."""
    import nsm_amd._lib as L
    cur, hist, out, mv, z0, z1, n0, n1 = (0x1000 * (i + 1) for i in range(8))

    def rc(cur=cur, hist=hist, mv=mv, zc=None, zp=None, nc=None, np_=None, blend=0.1, out=out):
        return L.lib.nsm_taa_resolve(cur, hist, mv, zc, zp, nc, np_, 1, 1, 8, 8, 1.0, 1.0, blend, 1,
                                     0.1, 0.9, out, None, None)

    for kw in (dict(cur=None), dict(hist=None), dict(out=None)):
        assert rc(**kw) == 1 and "taa_resolve: null" in L.last_error()
    assert rc(out=hist) == 1 and "out is hist" in L.last_error()
    assert rc(out=cur) == 1 and "out is cur" in L.last_error()
    for blend in (0.0, -0.1, 1.5, math.nan, math.inf):
        assert rc(blend=blend) == 1 and "blend" in L.last_error()
    for kw in (dict(zc=z0), dict(zp=z1), dict(nc=n0), dict(np_=n1)):
        assert rc(**kw) == 1 and "both frames" in L.last_error()
    for kw in (dict(mv=None, nc=n0, np_=n1), dict(mv=None, zc=z0, zp=z1)):
        assert rc(**kw) == 1 and "without motion vectors" in L.last_error()
    assert L.lib.nsm_taa_resolve(cur, hist, None, None, None, None, None, 1, 8, 1 << 14, 1 << 14, 1.0,
                                 1.0, 0.1, 1, 0.1, 0.9, out, None, None) == 1
    assert "taa_resolve: shape" in L.last_error()


def test_python_refusals_need_no_gpu():
    """Wrong lengths, wrong shapes, depth without motion vectors and a blend
    outside (0, 1] raise ValueError from the host checks alone, on CPU tensors."""
    import nsm_amd
    frames, mvs, z, n = A.inputs((2, 1, 19, 37), "grid")
    for kw in (dict(depth=z), dict(normals=n), dict(motion_vectors=mvs[:-1]),
               dict(motion_vectors=mvs + mvs[:1]), dict(motion_vectors=mvs, depth=z[:-1]),
               dict(motion_vectors=mvs, normals=z), dict(motion_vectors=mvs, depth=n),
               dict(motion_vectors=[m[:, :1] for m in mvs]),
               dict(motion_vectors=[m[:, :, :-1] for m in mvs]),
               dict(motion_vectors=mvs, mv_scale=1.0),
               dict(blend=0.0), dict(blend=1.5), dict(blend=math.nan)):
        with pytest.raises(ValueError):
            nsm_amd.temporal_aa(frames, **kw)
    with pytest.raises(ValueError):
        nsm_amd.temporal_aa(frames[:-1] + [frames[-1][:, :, :-1]], mvs)
    with pytest.raises(ValueError):
        nsm_amd.temporal_aa([])
    f, h = frames[1], frames[0]
    for args, kw in (((f, h[:, :, :-1]), {}), ((f[0], h), {}), ((f, None), {}),
                     ((f, h, mvs[0][:, :1]), {}),
                     ((f, h), dict(depth=z[1], prev_depth=z[0])),          # no motion vectors
                     ((f, h, mvs[0]), dict(depth=z[1])),                   # unpaired
                     ((f, h, mvs[0]), dict(prev_normals=n[0])),
                     ((f, h, mvs[0]), dict(normals=z[1], prev_normals=n[0])),
                     ((f, h, mvs[0]), dict(out=torch.empty(2, 1, 19, 36))),
                     ((f, h, mvs[0]), dict(out=torch.empty(2, 1, 19, 37, dtype=torch.float64))),
                     ((f, h), dict(blend=-0.1))):
        with pytest.raises(ValueError):
            nsm_amd.taa_resolve(*args, **kw)
    for kw in (dict(blend=0.0), dict(blend=2.0), dict(mv_scale=3)):
        with pytest.raises(ValueError):
            nsm_amd.TemporalAA(**kw)
    taa = nsm_amd.TemporalAA()
    for args in ((f[0],), (f, mvs[0][:, :1]), (f, None, n[0]), (f, mvs[0], z[0], z[0])):
        with pytest.raises(ValueError):
            taa(*args)
    # valid arguments reach the device check: there is no CPU implementation
    with pytest.raises(nsm_amd.NsmError):
        nsm_amd.temporal_aa(frames, mvs)
    with pytest.raises(nsm_amd.NsmError):
        nsm_amd.taa_resolve(f, h, mvs[0])
    with pytest.raises(nsm_amd.NsmError):
        taa(f)
