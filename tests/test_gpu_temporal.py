"""GPU: the temporal-instability metric with motion-vector reprojection
(nsm_temporal_pair / nsm_temporal_finalize / nsm_reproject) against the float64
restatement of the paper's Eq. 3 (temporal_util.py) on the same float32 inputs,
and the interface: both normalisations, alpha 5 and 3, depth and normal
rejection, an exact translation, zero motion against the reference's path and
fixture, fully rejected pairs, out-of-bounds guards, `reproject`, the bitwise
properties (repeat, stacked form, streaming form, 16-bit inputs), graph capture
and the refusals.

No fixture comes from running the reference: pert_loss.py:184-187 leaves the
motion-vector branch as `pass`, so `measure_temporal_instability(frames,
motion_vectors)` raises UnboundLocalError there on the first pair."""
import pytest
import torch

import temporal_util as U
from util import load

pytestmark = pytest.mark.gpu
torch.set_num_threads(16)

CASES = [(s, f, r) for f in U.FAMILIES for r in (False, True) for s in U.SHAPES]
IDS = [f"{f}-{'reject' if r else 'position'}-" + "x".join(map(str, s)) for s, f, r in CASES]
REJECT = dict(depth_tol=U.DEPTH_TOL, normal_cos=U.NORMAL_COS)

# A sum may be off by at most max(2 x the error of the float32 restatement on
# that (pair, image), floor x |sum|); the floors are derived, not tuned
# (temporal_util.floor_rel): 1e-6 on the 1/8-pixel grid, plus the coordinate
# rounding term for Gaussian motion vectors (1.4e-5 to 1.9e-4 in all at these
# widths). Worst measured kernel error / |sum| on an MI355X: grid 1.01e-7,
# Gaussian 2.12e-7 (the float32 restatement's own worst: 1.20e-7 and 2.12e-7);
# `reproject` on the grid cases: 8.7e-8 against its atol of 1e-6.


def to_dev(device, seq):
    return None if seq is None else [t.to(device) for t in seq]


def case(device, shape, family, reject):
    (frames, mvs, depth, normals), _, _ = U.reference(shape, family, reject, 5.0)
    kw = dict(depth=to_dev(device, depth), normals=to_dev(device, normals), **REJECT) if reject else {}
    return to_dev(device, frames), to_dev(device, mvs), kw


# ---- kernels ----------------------------------------------------------------
@pytest.mark.parametrize("shape,family,reject", CASES, ids=IDS)
def test_accuracy(device, shape, family, reject):
    """Per (pair, image) sums and counts, and the value in both normalisations,
    for alpha 5 and 3; every pixel counts."""
    import nsm_amd
    frames, mvs, kw = case(device, shape, family, reject)
    n_all = frames[0].numel()
    for alpha in (5.0, 3.0):
        data, (sums, counts, exps, _), (sums32, counts32, _, _) = U.reference(shape, family, reject, alpha)
        got_s, got_c = nsm_amd.temporal_instability_terms(frames, mvs, alpha, **kw)
        assert got_s.shape == got_c.shape == (U.T - 1, shape[0])
        assert got_s.dtype == torch.float32 and got_c.dtype == torch.int64
        assert torch.equal(got_c.cpu(), counts)
        floor = U.floor_rel(shape, family, data[1], sums, exps, alpha)
        err = (got_s.cpu().double() - sums).abs()
        f32 = (sums32.double() - sums).abs()
        bound = torch.maximum(2 * f32, floor * sums.abs())
        print(f"{family} {shape} reject={reject} alpha={alpha}: worst sum error / |sum| "
              f"{(err / sums.abs()).max().item():.2e} (float32 restatement "
              f"{(f32 / sums.abs()).max().item():.2e}, floor {floor.max().item():.2e}); surviving "
              f"{counts.sum().item()} of {counts.numel() * n_all // shape[0]}")
        assert sums.min() > 0
        assert (err <= bound).all()
        for norm in ("valid", "all"):
            ref = U.value(sums, counts, norm, n_all)
            ref32 = U.value(sums32, counts32, norm, n_all)
            v = nsm_amd.measure_temporal_instability(frames, mvs, alpha, normalize=norm, **kw)
            assert v.dim() == 0 and v.dtype == torch.float32 and v.device == frames[0].device
            e = abs(v.item() - ref)
            print(f"  normalize={norm}: value {ref:.7f} error / value {e / ref:.2e} "
                  f"(float32 restatement {abs(ref32 - ref) / ref:.2e})")
            assert e <= max(2 * abs(ref32 - ref), floor.max().item() * ref)
            # the value follows from the terms
            assert abs(U.value(got_s.cpu(), got_c.cpu(), norm, n_all) - v.item()) <= 2.0 ** -22 * ref


def test_translation_is_exactly_zero(device):
    """Frame t is frame t-1 rolled by (3, -2) and the motion vectors are
    (-3, +2): every sum is exactly 0 and (H-2)(W-3) pixels per image survive
    (positions 0 and H-1 are inside: the bounds are inclusive)."""
    import nsm_amd
    frames, mvs = U.translation_case()
    B, C, H, W = frames[0].shape
    frames, mvs = to_dev(device, frames), to_dev(device, mvs)
    sums, counts = nsm_amd.temporal_instability_terms(frames, mvs)
    assert (sums == 0).all() and (counts == (H - 2) * (W - 3)).all()
    for norm in ("valid", "all"):
        assert nsm_amd.measure_temporal_instability(frames, mvs, normalize=norm).item() == 0.0
    # without the motion vectors the same frames are far from stable
    assert nsm_amd.measure_temporal_instability(frames).item() > 0.1


def test_zero_motion_equals_the_unadjusted_path(device):
    import nsm_amd
    fx = load("temporal_b2_5f")
    frames = [torch.from_numpy(f).to(device) for f in fx["frames"]]
    B, C, H, W = frames[0].shape
    mvs = [torch.zeros(B, 2, H, W, device=device) for _ in frames[1:]]
    for a, key in ((5.0, "value_a5"), (3.0, "value_a3")):
        plain = nsm_amd.measure_temporal_instability(frames, alpha=a).item()
        for norm in ("valid", "all"):
            v = nsm_amd.measure_temporal_instability(frames, mvs, a, normalize=norm).item()
            assert abs(v - plain) <= 1e-6 * plain
            assert abs(v - float(fx[key])) <= 1e-6 * float(fx[key])
        _, counts = nsm_amd.temporal_instability_terms(frames, mvs, a)
        assert (counts == C * H * W).all()


WILD = [float("nan"), float("inf"), float("-inf"), 1e30, -1e30]


def test_fully_rejected_pair_contributes_zero(device):
    """Motion vectors holding NaN, +-Inf and +-1e30 are rejected; a pair in which
    every pixel is rejected has sum 0 and count 0 and the result stays finite."""
    import nsm_amd
    shape = (2, 1, 19, 37)
    frames, mvs, _, _ = U.inputs(shape, "gauss")
    mvs = [m.clone() for m in mvs]
    B, _, H, W = shape
    wild = torch.tensor(WILD)[torch.arange(B * H * W) % len(WILD)].view(B, H, W)
    mvs[1][:, 0] = wild                       # x wild, y ordinary
    mvs[1][:, 1, ::2] = wild.flip(2)[:, ::2]  # and y too on every other row
    fd, md = to_dev(device, frames), to_dev(device, mvs)
    sums, counts, _, _ = U.sequence(frames, mvs, 5.0)
    assert (counts[1] == 0).all() and (counts[0] > 0).all()
    got_s, got_c = nsm_amd.temporal_instability_terms(fd, md)
    assert torch.equal(got_c.cpu(), counts)
    assert (got_s[1] == 0).all() and torch.isfinite(got_s).all()
    # the other pairs are what they are without the wild pair, bit for bit
    plain_s, _ = nsm_amd.temporal_instability_terms(fd, to_dev(device, U.inputs(shape, "gauss")[1]))
    assert torch.equal(got_s[0], plain_s[0]) and torch.equal(got_s[2], plain_s[2])
    for norm in ("valid", "all"):
        v = nsm_amd.measure_temporal_instability(fd, md, normalize=norm).item()
        ref = U.value(got_s.cpu(), got_c.cpu(), norm, frames[0].numel())
        assert ref > 0 and abs(v - ref) <= 2.0 ** -22 * ref
    # every pair rejected: exactly 0, not NaN
    all_wild = [md[1]] * (U.T - 1)
    for norm in ("valid", "all"):
        assert nsm_amd.measure_temporal_instability(fd, all_wild, normalize=norm).item() == 0.0
    s, c = nsm_amd.temporal_instability_terms(fd, all_wild)
    assert (s == 0).all() and (c == 0).all()
    # x alone and y alone reject as well
    for ch in (0, 1):
        m = torch.zeros(B, 2, H, W)
        m[:, ch] = wild
        _, valid = nsm_amd.reproject(fd[0], m.to(device))
        assert not valid.any()


# ---- out-of-bounds guard (in the manner of test_gpu_guard.py) ---------------------
GUARD = 1 << 16


def guarded(t, device):
    """`t` in the middle of a larger NaN-filled allocation."""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=torch.float32, device=device)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize("shape", U.SHAPES, ids=["x".join(map(str, s)) for s in U.SHAPES])
def test_wild_motion_vectors_stay_in_bounds(device, shape):
    """Frames, depth and normals live inside NaN-filled buffers: a tap outside a
    tensor would carry a NaN into the result. With wild motion vectors the
    results are finite and bitwise those from tight buffers."""
    import nsm_amd
    frames, mvs, depth, normals = U.inputs(shape, "gauss")
    gen = torch.Generator().manual_seed(1)
    wild = torch.tensor(WILD + [1e9, -1e9, 3e4, -3e4, 2.0 ** 31, -2.0 ** 31, 2.0 ** 24, 1e-30])
    mvs = [torch.where(torch.rand(m.shape, generator=gen) < 0.4,
                       wild[torch.randint(0, len(wild), m.shape, generator=gen)], m) for m in mvs]
    md = to_dev(device, mvs)
    res = []
    for put in (lambda t: t.to(device), lambda t: guarded(t, device)):
        f, z, n = ([put(t) for t in seq] for seq in (frames, depth, normals))
        s, c = nsm_amd.temporal_instability_terms(f, md, depth=z, normals=n, **REJECT)
        s0, c0 = nsm_amd.temporal_instability_terms(f, md)
        v = nsm_amd.measure_temporal_instability(f, md, depth=z, normals=n, **REJECT)
        w, ok = nsm_amd.reproject(f[0], md[0])
        res.append((s, c, s0, c0, v, w, ok))
    for a, b in zip(*res):
        assert torch.isfinite(a.float()).all()
        assert torch.equal(a, b)
    assert res[0][3].sum() > 0   # some pixels survive


# ---- reproject ----------------------------------------------------------------
@pytest.mark.parametrize("family", U.FAMILIES)
@pytest.mark.parametrize("shape", U.SHAPES, ids=["x".join(map(str, s)) for s in U.SHAPES])
def test_reproject(device, shape, family):
    import nsm_amd
    frames, mvs, _, _ = U.inputs(shape, family)
    for t in range(1, U.T):
        ok, taps, _ = U.lookup(mvs[t - 1])
        ref = U.sample(frames[t - 1].double(), taps)
        warped, valid = nsm_amd.reproject(frames[t - 1].to(device), mvs[t - 1].to(device))
        assert warped.shape == shape and warped.dtype == torch.float32
        assert valid.shape == (shape[0], 1) + shape[2:] and valid.dtype == torch.bool
        assert torch.equal(valid.cpu()[:, 0], ok)
        keep = ok.unsqueeze(1).expand_as(ref)
        assert (warped.cpu()[~keep] == 0).all()
        err = (warped.cpu().double() - ref)[keep].abs().max().item()
        print(f"{family} {shape} pair {t}: warped max|d| {err:.2e} on {int(ok.sum())} valid pixels")
        if family == "grid":
            # exact coordinates and weights: eight roundings of values in [0, 1], doubled
            assert err <= 1e-6


# ---- bitwise properties -----------------------------------------------------------
def test_bitwise_properties(device):
    import nsm_amd
    shape = (2, 1, 67, 129)
    frames, mvs, kw = case(device, shape, "gauss", True)

    def run(f, m, **over):
        k = dict(kw, **over)
        return (nsm_amd.measure_temporal_instability(f, m, **k),
                *nsm_amd.temporal_instability_terms(f, m, **k))

    first = run(frames, mvs)
    for other in (run(frames, mvs),
                  run(torch.stack(frames), torch.stack(mvs), depth=torch.stack(kw["depth"]),
                      normals=torch.stack(kw["normals"]))):
        for a, b in zip(first, other):
            assert torch.equal(a, b)
    # a scale that undoes a power-of-two factor is exact
    for a, b in zip(first, run(frames, [2 * m for m in mvs], mv_scale=(0.5, 0.5))):
        assert torch.equal(a, b)
    # the streaming form, in both normalisations
    for norm in ("valid", "all"):
        ti = nsm_amd.TemporalInstability(normalize=norm, **REJECT)
        assert ti.compute() == 0.0
        for rounds in range(2):
            for t, f in enumerate(frames):
                ti.update(f, mvs[t - 1] if t else None, kw["depth"][t], kw["normals"][t])
            want = nsm_amd.measure_temporal_instability(frames, mvs, normalize=norm, **kw).item()
            assert ti.compute() == want and want > 0
            ti.reset()
            assert ti.compute() == 0.0
    # 16-bit frames equal the fp32 call on the converted values
    for dt in (torch.float16, torch.bfloat16):
        f16 = [f.to(dt) for f in frames]
        for a, b in zip(run(f16, mvs), run([f.float() for f in f16], mvs)):
            assert torch.equal(a, b)
        assert not torch.equal(run(f16, mvs)[0], first[0])


def test_streaming_keeps_its_own_copy(device):
    """The caller may reuse one frame buffer: update() does not alias it."""
    import nsm_amd
    frames, mvs, _ = case(device, (2, 1, 19, 37), "grid", False)
    ti = nsm_amd.TemporalInstability()
    buf = torch.empty_like(frames[0])
    for t, f in enumerate(frames):
        buf.copy_(f)
        ti.update(buf, mvs[t - 1] if t else None)
    assert ti.compute() == nsm_amd.measure_temporal_instability(frames, mvs).item()


# ---- graph capture -----------------------------------------------------------------
def test_graph_capture(device):
    """Captured in torch.cuda.graph and replayed on new contents, the list form
    and a streaming update equal the eager calls bitwise: nothing in them
    touches the host."""
    import nsm_amd
    shape = (2, 1, 19, 37)
    frames, mvs, kw = case(device, shape, "gauss", True)
    other, omv, okw = case(device, shape, "grid", True)
    sf, sm = torch.stack(frames), torch.stack(mvs)
    sz, sn = torch.stack(kw["depth"]), torch.stack(kw["normals"])
    ti = nsm_amd.TemporalInstability(device=device, **REJECT)
    ti.update(sf[0], None, sz[0], sn[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up: kernels loaded, allocator primed
        nsm_amd.measure_temporal_instability(sf, sm, depth=sz, normals=sn, **REJECT)
        ti.update(sf[1], sm[0], sz[1], sn[1])
    torch.cuda.current_stream().wait_stream(side)
    ti.reset()
    ti.update(sf[0], None, sz[0], sn[0])
    cf, cm, cz, cn = (torch.empty_like(t[0]) for t in (sf, sm, sz, sn))
    g, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = nsm_amd.measure_temporal_instability(sf, sm, depth=sz, normals=sn, **REJECT)
        s, c = nsm_amd.temporal_instability_terms(sf, sm, depth=sz, normals=sn, **REJECT)
    with torch.cuda.graph(g2):
        ti.update(cf, cm, cz, cn)
    for fr, mv, k in ((other, omv, okw), (frames, mvs, kw)):
        sf.copy_(torch.stack(fr))
        sm.copy_(torch.stack(mv))
        sz.copy_(torch.stack(k["depth"]))
        sn.copy_(torch.stack(k["normals"]))
        g.replay()
        want = nsm_amd.measure_temporal_instability(fr, mv, **k)
        ws, wc = nsm_amd.temporal_instability_terms(fr, mv, **k)
        assert torch.equal(out, want) and torch.equal(s, ws) and torch.equal(c, wc)
        ti.reset()
        ti.update(fr[0], None, k["depth"][0], k["normals"][0])
        for t in range(1, U.T):
            for dst, src in ((cf, fr[t]), (cm, mv[t - 1]), (cz, k["depth"][t]), (cn, k["normals"][t])):
                dst.copy_(src)
            g2.replay()
        assert ti.compute() == want.item()


# ---- refusals -------------------------------------------------------------------------
def test_refusals(device):
    import nsm_amd
    shape = (2, 1, 19, 37)
    frames, mvs, kw = case(device, shape, "grid", True)
    z, n = kw["depth"], kw["normals"]
    bad = [
        dict(depth=z), dict(normals=n),                                       # no motion vectors
        dict(motion_vectors=mvs[:-1]), dict(motion_vectors=mvs + mvs[:1]),    # wrong lengths
        dict(motion_vectors=mvs, depth=z[:-1]), dict(motion_vectors=mvs, normals=n + n[:1]),
        dict(motion_vectors=[m[:, :1] for m in mvs]),                         # wrong shapes
        dict(motion_vectors=[m[:, :, :-1] for m in mvs]),
        dict(motion_vectors=mvs, depth=n), dict(motion_vectors=mvs, normals=z),
        dict(motion_vectors=mvs, depth=[t[:1] for t in z]),
        dict(motion_vectors=mvs, normalize="mean"), dict(motion_vectors=mvs, mv_scale=1.0),
    ]
    for k in bad:
        with pytest.raises(ValueError):
            nsm_amd.measure_temporal_instability(frames, **k)
        with pytest.raises(ValueError):
            nsm_amd.temporal_instability_terms(frames, **k)
    with pytest.raises(ValueError):
        nsm_amd.measure_temporal_instability(frames[:-1] + [frames[-1][:, :, :-1]], mvs)
    with pytest.raises((ValueError, nsm_amd.NsmError)):
        nsm_amd.measure_temporal_instability([f.cpu() for f in frames], mvs)
    with pytest.raises(ValueError):
        nsm_amd.reproject(frames[0], mvs[0][:, :1])
    with pytest.raises(ValueError):
        nsm_amd.reproject(frames[0][0], mvs[0])
    ti = nsm_amd.TemporalInstability()
    ti.update(frames[0])
    for args in ((frames[1], mvs[0][:, :1]), (frames[1], None, z[1]), (frames[1], mvs[0], z[1]),
                 (frames[1][:, :, :-1], None)):
        with pytest.raises(ValueError):
            ti.update(*args)
    with pytest.raises(ValueError):
        nsm_amd.TemporalInstability(normalize="mean")
    # the unadjusted path is untouched by the new arguments' defaults
    assert torch.equal(nsm_amd.measure_temporal_instability(frames),
                       nsm_amd.measure_temporal_instability(frames, None, 5.0))
