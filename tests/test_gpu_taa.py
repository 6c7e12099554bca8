"""GPU: the temporal anti-aliasing resolve (nsm_taa_resolve; taa_resolve,
temporal_aa, TemporalAA) against the float64 restatement of its definition
(taa_util.py, on temporal_util's lookup) on the same float32 inputs: accuracy on
every seeded case, the bitwise properties, the edges (degenerate shapes, wild
motion vectors, guard pages, independent planes), the direction of the effect
on the temporal-instability metric, and graph capture.

Worst measured error of a frame on an MI355X (absolute, values in [0, 1]):
1.2e-7 on the 1/8-pixel grid (the float32 restatement's own: 1.5e-7; floor
4.8e-7 to 1.3e-6), 3.6e-6 with Gaussian motion vectors (float32 restatement
3.6e-6; floor up to 9.1e-5), both on 2x1x67x129 ("Temporal
anti-aliasing pass")."""
import math

import pytest
import torch

import taa_util as A
import temporal_util as U

pytestmark = pytest.mark.gpu
torch.set_num_threads(16)

GEOM = [(s, f, r) for f in A.FAMILIES for r in (False, True) for s in A.SHAPES]
GEOM_IDS = [f"{f}-{'reject' if r else 'position'}-" + "x".join(map(str, s)) for s, f, r in GEOM]
REJECT = dict(depth_tol=A.DEPTH_TOL, normal_cos=A.NORMAL_COS)


def to_dev(device, seq):
    return None if seq is None else [t.to(device) for t in seq]


def case(device, shape, family, reject):
    frames, mvs, depth, normals = A.inputs(shape, family)
    kw = dict(depth=to_dev(device, depth), normals=to_dev(device, normals), **REJECT) if reject else {}
    return to_dev(device, frames), to_dev(device, mvs), kw


def check_frames(got, ref64, ref32, shape, family, mvs, blend, what):
    """Every frame within max(2 x the float32 restatement's error, the derived
    floor) of the float64 restatement; returns the worst error."""
    worst = 0.0
    for t in range(len(ref64)):
        err = (got[t].cpu().double() - ref64[t]).abs().max().item()
        lim, e32 = A.bound(ref64, ref32, shape, family, mvs, blend, t)
        print(f"{what} frame {t}: max|d| {err:.2e} (float32 restatement {e32:.2e}, "
              f"bound {lim:.2e})")
        assert err <= lim
        worst = max(worst, err)
    return worst


# ---- accuracy --------------------------------------------------------------------
@pytest.mark.parametrize("shape,family,reject", GEOM, ids=GEOM_IDS)
def test_accuracy(device, shape, family, reject):
    import nsm_amd
    frames, mvs, kw = case(device, shape, family, reject)
    for clamp in (True, False):
        for blend in A.BLENDS:
            data, (o64, a64, _), (o32, _, _) = A.reference(shape, family, reject, clamp, blend)
            out, acc = nsm_amd.temporal_aa(frames, mvs, blend=blend, clamp=clamp, return_mask=True,
                                           **kw)
            assert out.shape == (A.T,) + shape and out.dtype == torch.float32
            assert acc.shape == (A.T, shape[0], 1) + shape[2:] and acc.dtype == torch.bool
            assert torch.equal(acc.cpu(), torch.stack(a64))
            assert torch.equal(out[0], frames[0])
            worst = check_frames(out, o64, o32, shape, family, data[1], blend,
                                 f"{family} {shape} reject={reject} clamp={clamp} blend={blend}")
            print(f"WORST {family} {shape} reject={reject} clamp={clamp} blend={blend}: {worst:.2e}; "
                  f"accepted {acc[1:].float().mean().item():.2f}")


# ---- bitwise properties ----------------------------------------------------------
@pytest.mark.parametrize("clamp", (True, False))
def test_identities_are_exact(device, clamp):
    """An exact translation, a static sequence and blend = 1 return the inputs
    bit for bit; a constant frame after a checkerboard is exactly 0.5 under the
    clamp and shows the history without it."""
    import nsm_amd
    frames, mvs = A.translation_case()
    B, C, H, W = frames[0].shape
    fd, md = to_dev(device, frames), to_dev(device, mvs)
    out, acc = nsm_amd.temporal_aa(fd, md, clamp=clamp, return_mask=True)
    assert torch.equal(out, torch.stack(fd))
    assert (acc[1:].flatten(1).sum(1) == B * (H - 2) * (W - 3)).all() and not acc[0].any()
    frames, mvs, kw = case(device, (2, 1, 67, 129), "gauss", True)
    still = [frames[0]] * A.T
    for m in (None, [torch.zeros_like(v) for v in mvs]):
        out, acc = nsm_amd.temporal_aa(still, m, clamp=clamp, return_mask=True)
        assert torch.equal(out, torch.stack(still)) and acc[1:].all()
    out, acc = nsm_amd.temporal_aa(frames, mvs, blend=1.0, clamp=clamp, return_mask=True, **kw)
    assert torch.equal(out, torch.stack(frames)) and acc[1].any() and not acc[1].all()
    board, flat = to_dev(device, A.constant_case())
    for blend in A.BLENDS:
        out = nsm_amd.temporal_aa([board, flat], blend=blend, clamp=clamp)
        if clamp:
            assert (out[1] == 0.5).all()
        else:
            keep = 1 - torch.tensor(blend, dtype=torch.float32)
            assert (out[1].cpu() - (0.5 + keep * (board.cpu() - 0.5))).abs().max() <= 2.0 ** -23
            assert (out[1] != 0.5).all()


def test_bitwise_properties(device):
    """Repeat, stacked form, streaming form in both buffer modes, 16-bit
    inputs, and taa_resolve composed by hand."""
    import nsm_amd
    shape = (2, 1, 67, 129)
    frames, mvs, kw = case(device, shape, "gauss", True)
    z, n = kw["depth"], kw["normals"]
    first, mask = nsm_amd.temporal_aa(frames, mvs, return_mask=True, **kw)
    again = nsm_amd.temporal_aa(frames, mvs, **kw)
    stacked = nsm_amd.temporal_aa(torch.stack(frames), torch.stack(mvs), depth=torch.stack(z),
                                  normals=torch.stack(n), **REJECT)
    assert torch.equal(first, again) and torch.equal(first, stacked)
    # a scale that undoes a power-of-two factor is exact
    assert torch.equal(first, nsm_amd.temporal_aa(frames, [2 * m for m in mvs], mv_scale=(0.5, 0.5),
                                                  **kw))
    for capturable in (False, True):
        taa = nsm_amd.TemporalAA(capturable=capturable, **REJECT)
        for rounds in range(2):
            for t, f in enumerate(frames):
                o = taa(f, mvs[t - 1] if t else None, z[t], n[t])
                assert o.dtype == torch.float32 and torch.equal(o, first[t])
            taa.reset()
    # the caller may reuse its buffers: the previous depth and normals are copies
    taa = nsm_amd.TemporalAA(**REJECT)
    bf, bm, bz, bn = (torch.empty_like(s[0]) for s in (frames, mvs, z, n))
    for t in range(A.T):
        for dst, src in ((bf, frames[t]), (bm, mvs[t - 1]), (bz, z[t]), (bn, n[t])):
            dst.copy_(src)
        assert torch.equal(taa(bf, bm, bz, bn), first[t])
    # by hand
    hist = frames[0]
    for t in range(1, A.T):
        out = torch.full(shape, float("nan"), device=device)
        res, acc = nsm_amd.taa_resolve(frames[t], hist, mvs[t - 1], depth=z[t], prev_depth=z[t - 1],
                                       normals=n[t], prev_normals=n[t - 1], out=out,
                                       return_mask=True, **REJECT)
        assert res is out and torch.equal(out, first[t]) and torch.equal(acc, mask[t])
        hist = out
    assert torch.equal(nsm_amd.taa_resolve(frames[1], frames[0], mvs[0]),
                       nsm_amd.temporal_aa(frames[:2], mvs[:1])[1])
    for bad in (frames[1], frames[0]):
        with pytest.raises(ValueError):
            nsm_amd.taa_resolve(frames[1], frames[0], mvs[0], out=bad)
    # 16-bit inputs equal the fp32 call on the converted values
    for dt in (torch.float16, torch.bfloat16):
        f16, z16 = [f.to(dt) for f in frames], [t.to(dt) for t in z]
        a = nsm_amd.temporal_aa(f16, mvs, depth=z16, normals=n, **REJECT)
        b = nsm_amd.temporal_aa([f.float() for f in f16], mvs, depth=[t.float() for t in z16],
                                normals=n, **REJECT)
        assert a.dtype == torch.float32 and torch.equal(a, b) and not torch.equal(a, first)


# ---- edges -----------------------------------------------------------------------
@pytest.mark.parametrize("shape,scale", [((1, 1, 1, 7), (1.0, 1.0)), ((1, 1, 1, 7), (1.0, 0.0)),
                                         ((1, 2, 5, 1), (1.0, 1.0)), ((1, 2, 5, 1), (0.0, 1.0))],
                         ids=["1x7", "1x7-x-only", "5x1", "5x1-y-only"])
def test_degenerate_planes(device, shape, scale):
    """One row and one column (the neighbourhood and the taps fold onto the
    plane), on the 1/8-pixel grid; with the motion along the missing axis
    switched off so that pixels are accepted."""
    import nsm_amd
    frames, mvs, depth, normals = A.inputs(shape, "grid")
    for clamp in (True, False):
        o64, a64, _ = A.resolve(frames, mvs, blend=0.5, clamp=clamp, scale=scale)
        o32, _, _ = A.resolve(frames, mvs, blend=0.5, clamp=clamp, scale=scale, dtype=torch.float32)
        out, acc = nsm_amd.temporal_aa(to_dev(device, frames), to_dev(device, mvs), blend=0.5,
                                       clamp=clamp, mv_scale=scale, return_mask=True)
        assert torch.equal(acc.cpu(), torch.stack(a64))
        if 0.0 in scale:
            assert acc[1:].any()
        check_frames(out, o64, o32, shape, "grid", mvs, 0.5, f"{shape} scale={scale} clamp={clamp}")


WILD = [float("nan"), float("inf"), float("-inf"), 1e30, -1e30]


def test_wild_motion_vectors_return_the_frame(device):
    import nsm_amd
    shape = (2, 1, 19, 37)
    frames, mvs, _, _ = A.inputs(shape, "gauss")
    B, _, H, W = shape
    wild = torch.tensor(WILD)[torch.arange(B * H * W) % len(WILD)].view(B, H, W)
    hit = torch.zeros(B, H, W, dtype=torch.bool)
    hit[:, ::2, 1::3] = True
    mv = mvs[0].clone()
    mv[:, 0][hit] = wild[hit]                           # x wild, y ordinary
    mv[:, 1, ::4][hit[:, ::4]] = wild.flip(2)[:, ::4][hit[:, ::4]]   # and y too on some rows
    for clamp in (True, False):
        out, acc = nsm_amd.taa_resolve(frames[1].to(device), frames[0].to(device), mv.to(device),
                                       clamp=clamp, return_mask=True)
        plain = nsm_amd.taa_resolve(frames[1].to(device), frames[0].to(device), mvs[0].to(device),
                                    clamp=clamp)
        out, acc = out.cpu(), acc.cpu()
        assert torch.isfinite(out).all()
        assert not acc[:, 0][hit].any() and acc.any()
        assert torch.equal(out[:, 0][hit], frames[1][:, 0][hit])
        assert torch.equal(out[:, 0][~hit], plain.cpu()[:, 0][~hit])
    # y alone rejects as well
    mv = torch.zeros(B, 2, H, W)
    mv[:, 1] = wild
    out, acc = nsm_amd.taa_resolve(frames[1].to(device), frames[0].to(device), mv.to(device),
                                   return_mask=True)
    assert not acc.any() and torch.equal(out.cpu(), frames[1])


GUARD = 1 << 16


def guarded(t, device):
    """`t` in the middle of a larger NaN-filled allocation."""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=torch.float32, device=device)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize("shape", A.SHAPES, ids=["x".join(map(str, s)) for s in A.SHAPES])
def test_neighbourhood_and_taps_stay_in_bounds(device, shape):
    """Frame, history, depth and normals live inside NaN-filled buffers: a tap
    or a neighbour outside a tensor would carry a NaN into the result. With wild
    motion vectors the results are finite and bitwise those from tight buffers."""
    import nsm_amd
    frames, mvs, depth, normals = A.inputs(shape, "gauss")
    gen = torch.Generator().manual_seed(1)
    wild = torch.tensor(WILD + [1e9, -1e9, 3e4, -3e4, 2.0 ** 31, -2.0 ** 31, 2.0 ** 24, 1e-30])
    mv = torch.where(torch.rand(mvs[0].shape, generator=gen) < 0.4,
                     wild[torch.randint(0, len(wild), mvs[0].shape, generator=gen)], mvs[0])
    res = []
    for put in (lambda t: t.to(device), lambda t: guarded(t, device)):
        f, z, n = ([put(t) for t in seq[:2]] for seq in (frames, depth, normals))
        for clamp in (True, False):
            res.append(nsm_amd.taa_resolve(f[1], f[0], mv.to(device), depth=z[1], prev_depth=z[0],
                                           normals=n[1], prev_normals=n[0], clamp=clamp,
                                           out=put(torch.zeros(shape)), return_mask=True, **REJECT))
            res.append(nsm_amd.taa_resolve(f[1], f[0], clamp=clamp, return_mask=True))
    half = len(res) // 2
    for (a, am), (b, bm) in zip(res[:half], res[half:]):
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        assert torch.equal(a, b) and torch.equal(am, bm)
    assert res[0][1].any() and not res[0][1].all()


def test_planes_are_independent(device):
    """Another image 1, or another channel 2, leaves every other plane's
    output bitwise unchanged."""
    import nsm_amd
    shape = (2, 3, 19, 37)
    frames, mvs, depth, normals = (to_dev(device, s) for s in A.inputs(shape, "gauss"))
    other = [to_dev(device, s) for s in A.inputs(shape, "gauss", seed=11)]

    def run(fr, mv, z, n):
        return nsm_amd.temporal_aa(fr, mv, depth=z, normals=n, **REJECT)

    base = run(frames, mvs, depth, normals)
    swapped = [[torch.stack([a[0], b[1]]) for a, b in zip(s, o)]
               for s, o in zip((frames, mvs, depth, normals), other)]
    got = run(*swapped)
    assert torch.equal(got[:, 0], base[:, 0]) and not torch.equal(got[:, 1], base[:, 1])
    fr = [f.clone() for f in frames]
    for f, o in zip(fr, other[0]):
        f[:, 2] = o[:, 2]
    got = run(fr, mvs, depth, normals)
    assert torch.equal(got[:, :, :2], base[:, :, :2]) and not torch.equal(got[:, :, 2], base[:, :, 2])


# ---- the direction of the effect (Figure 6's axis) ------------------------------
@pytest.mark.parametrize("clamp", (True, False))
def test_resolved_sequence_is_more_stable(device, clamp):
    """A smooth image plus iid noise per frame, no motion: the metric of the
    resolved sequence is below that of the input and equals the restatement's.
    A frame error e moves D = |O_t - O_{t-1}| by at most 2e and exp(alpha D) by
    at most alpha exp(alpha (Dmax + 2e)) 2e; the metric itself is good to 1e-6
    of its value (test_gpu_temporal)."""
    import nsm_amd
    alpha, blend = 5.0, 0.1
    frames = A.noise_case()
    shape = tuple(frames[0].shape)
    o64, _, _ = A.resolve(frames, None, blend=blend, clamp=clamp)
    o32, _, _ = A.resolve(frames, None, blend=blend, clamp=clamp, dtype=torch.float32)
    zero = [torch.zeros(shape[0], 2, *shape[2:])] * (A.NOISE_T - 1)

    def metric(seq):
        sums, counts, _, _ = U.sequence(seq, zero, alpha)
        return U.value(sums, counts, "valid", seq[0].numel())

    e_in, e_ref = metric(frames), metric(o64)
    fd = to_dev(device, frames)
    out = nsm_amd.temporal_aa(fd, blend=blend, clamp=clamp)
    worst = check_frames(out, o64, o32, shape, "grid", None, blend, f"noise clamp={clamp}")
    got_in = nsm_amd.measure_temporal_instability(fd, alpha=alpha).item()
    got = nsm_amd.measure_temporal_instability(out, alpha=alpha).item()
    lim = max(A.bound(o64, o32, shape, "grid", None, blend, t)[0] for t in range(A.NOISE_T))
    dmax = max((o64[t] - o64[t - 1]).abs().max().item() for t in range(1, A.NOISE_T))
    tol = 1e-6 * e_ref + alpha * math.exp(alpha * (dmax + 2 * lim)) * 2 * lim + 2.0 ** -24
    print(f"noise clamp={clamp}: E input {got_in:.4f} (restatement {e_in:.4f}) -> resolved "
          f"{got:.5f} (restatement {e_ref:.5f}, tolerance {tol:.1e}); worst frame error {worst:.2e}")
    assert abs(got_in - e_in) <= 1e-5 * e_in
    assert got < got_in
    assert abs(got - e_ref) <= tol


# ---- graph capture ---------------------------------------------------------------
def test_graph_capture(device):
    """One TemporalAA(capturable=True) call captured in torch.cuda.graph and
    replayed over two sequences through static inputs equals the eager frames
    bitwise: every buffer stays where it is and nothing touches the host."""
    import nsm_amd
    shape = (2, 1, 19, 37)
    seqs = [case(device, shape, fam, True) for fam in ("grid", "gauss")]
    frames, mvs, kw = seqs[1]
    taa = nsm_amd.TemporalAA(capturable=True, **REJECT)
    taa(frames[0], None, kw["depth"][0], kw["normals"][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up: kernel loaded, allocator primed
        taa(frames[1], mvs[0], kw["depth"][1], kw["normals"][1])
    torch.cuda.current_stream().wait_stream(side)
    cf, cm, cz, cn = (torch.empty_like(t[0]) for t in (frames, mvs, kw["depth"], kw["normals"]))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = taa(cf, cm, cz, cn)
    for fr, mv, k in seqs:
        want = nsm_amd.temporal_aa(fr, mv, **k)
        taa.reset()
        assert torch.equal(taa(fr[0], None, k["depth"][0], k["normals"][0]), want[0])
        for t in range(1, A.T):
            for dst, src in ((cf, fr[t]), (cm, mv[t - 1]), (cz, k["depth"][t]), (cn, k["normals"][t])):
                dst.copy_(src)
            g.replay()
            assert torch.equal(res, want[t])
