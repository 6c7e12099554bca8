"""GPU: the SVGF denoiser (nsm_svgf_accumulate / _variance / _atrous; svgf, SVGF,
atrous_filter, svgf_accumulate, svgf_variance) against the float64 restatement
of its definition (svgf_util.py) on the same float32 inputs: accuracy of every
pass and of the whole recurrence, the bitwise properties, the edges (degenerate
shapes, wild motion vectors, NaN margins, edge stopping), the direction of the
effect, graph capture and the argument errors.

Worst measured errors on an MI355X (absolute, colour in [0, 1]; the float32
restatement's own in brackets): accumulation colour 9.4e-8 (9.8e-8), moments
9.7e-8 (1.1e-7), variance 1.7e-7 (1.8e-7), floor 4.8e-7; variance fallback
colour 1.1e-6 (1.1e-6, floor 2.5e-5), variance 2.6e-6 (2.6e-6, floor 3.0e-4);
one a-trous iteration colour 6.7e-7 (6.7e-7, floor 2.5e-5), variance 7.3e-7
(7.0e-7, floor 6.9e-6 to 3.5e-5); the whole recurrence, any frame: colour
5.9e-7 on "planes" and 1.8e-6 on "random", variance 6.3e-8 and 2.3e-6. Edge
stopping: leakage 2.3e-19 (the restatement's 2.3e-19); with sigma_z and sigma_n
neutralised 7.0e-3. Denoising on 2x1x67x129: MSE 0.02244 -> 0.00012, temporal
instability 1.394 -> 0.017 ("SVGF denoiser")."""
import pytest
import torch

import svgf_util as S

pytestmark = pytest.mark.gpu
torch.set_num_threads(16)

IDS = ["x".join(map(str, s)) for s in S.SHAPES]
REJECT = dict(depth_tol=S.DEPTH_TOL, normal_cos=S.NORMAL_COS)
BIG = (2, 1, 67, 129)


def dev_seq(device, seq):
    return None if seq is None else [t.to(device) for t in seq]


def case(device, shape, family):
    frames, mvs, depth, normals, _ = S.inputs(shape, family)
    return (dev_seq(device, frames), dev_seq(device, mvs), dev_seq(device, depth),
            dev_seq(device, normals))


def close(got, r64, r32, floor, what):
    """got within max(2 x the float32 restatement's error, floor) of r64."""
    err = (got.cpu().double() - r64).abs().max().item()
    lim, e32 = S.bound(r64, r32, floor)
    print(f"{what}: max|d| {err:.2e} (float32 restatement {e32:.2e}, floor {floor:.2e})")
    assert err <= lim, what
    return err


# ---- accuracy ----------------------------------------------------------------
@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_passes(device, shape, family):
    """Each pass alone, on inputs both sides share: the accumulation of frame 1
    on frame 0's outputs, the variance fallback on its results (lengths raised
    on a checkerboard so that some pixels pass through), and the a-trous
    iteration at steps 1 to 16, with and without the luminance term."""
    import nsm_amd
    frames, mvs, depth, normals, _ = S.inputs(shape, family)
    B, C, H, W = shape
    p = S.PARAMS
    sn = p["sigma_n"]
    what = f"{family} {shape}"
    d = lambda t: t.to(device)   # noqa: E731
    # a first frame, then frame 1
    first = S.accumulate(frames[0], depth[0], normals[0], None, None, None, None)
    g0 = nsm_amd.svgf_accumulate(d(frames[0]), return_mask=True)
    for key, got in zip(("color", "moments", "var"), (g0[0], g0[1], g0[3])):
        close(got, first[key], first[key].float(), S.FLOOR_ACC, f"{what} first {key}")
    assert (g0[2] == 1).all() and not g0[4].any()
    assert torch.equal(g0[0], d(frames[0]))
    hist = tuple(first[k].float() for k in ("color", "moments", "length"))
    hist[2].add_(torch.arange(H * W).view(H, W) % 3)      # lengths 1 to 3
    a64, a32 = (S.accumulate(frames[1], depth[1], normals[1], depth[0], normals[0], mvs[0], hist,
                             dtype=dt) for dt in (torch.float64, torch.float32))
    got = nsm_amd.svgf_accumulate(d(frames[1]), d(mvs[0]), depth=d(depth[1]), normals=d(normals[1]),
                                  prev_depth=d(depth[0]), prev_normals=d(normals[0]),
                                  history=tuple(d(t) for t in hist), return_mask=True, **REJECT)
    assert torch.equal(got[4].cpu(), a64["accepted"]) and torch.equal(got[2].cpu().double(),
                                                                    a64["length"])
    assert a64["accepted"].any() and not a64["accepted"].all()
    for key, g in zip(("color", "moments", "var"), (got[0], got[1], got[3])):
        close(g, a64[key], a32[key], S.FLOOR_ACC, f"{what} accumulate {key}")
    # the variance fallback
    acc = {k: a32[k].contiguous() for k in ("color", "moments", "length", "var")}
    yy, xx = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    acc["length"] = acc["length"] + 3.0 * ((xx + yy) % 2)
    v64, v32 = (S.variance_pass(acc["color"], acc["moments"], acc["length"], acc["var"], depth[1],
                                normals[1], p["min_history"], p["sigma_z"], sn, dtype=dt)
                for dt in (torch.float64, torch.float32))
    gc, gv = nsm_amd.svgf_variance(d(acc["color"]), d(acc["moments"]), d(acc["length"]),
                                   d(acc["var"]), d(depth[1]), d(normals[1]),
                                   min_history=p["min_history"], sigma_n=sn)
    close(gc, v64[0], v32[0], S.floor_color(sn), f"{what} variance colour")
    close(gv, v64[1], v32[1], S.floor_var_fallback(sn, p["min_history"]), f"{what} variance var")
    through = (acc["length"] >= p["min_history"]).expand(B, C, H, W)
    assert through.any() and not through.all()
    assert torch.equal(gc.cpu()[through], acc["color"][through])
    # the a-trous iteration
    color, var = v32[0].contiguous(), v32[1].contiguous()
    vmax = var.max().item()
    for step in (1, 2, 4, 8, 16):
        r64, r32 = (S.atrous(color, var, depth[1], normals[1], step, p["sigma_z"], sn, p["sigma_l"],
                             dtype=dt) for dt in (torch.float64, torch.float32))
        gc, gv = nsm_amd.atrous_filter(d(color), d(depth[1]), d(normals[1]), d(var), step=step,
                                       sigma_n=sn)
        close(gc, r64[0], r32[0], S.floor_color(sn), f"{what} a-trous {step} colour")
        close(gv, r64[1], r32[1], S.floor_var_atrous(sn, vmax), f"{what} a-trous {step} var")
    r64, r32 = (S.atrous(color, None, depth[1], normals[1], 2, 1.0, 8.0, dtype=dt)
                for dt in (torch.float64, torch.float32))
    gc = nsm_amd.atrous_filter(d(color), d(depth[1]), d(normals[1]), step=2, sigma_n=8.0)
    assert torch.is_tensor(gc)
    close(gc, r64[0], r32[0], S.floor_color(8.0), f"{what} depth-aware post filter")
    assert torch.equal(gc, nsm_amd.atrous_filter(d(color), d(depth[1]), d(normals[1]), d(var),
                                                 step=2, sigma_n=8.0, sigma_l=0.0))


SEQ = [(s, f, m, "default") for f in S.FAMILIES for s in S.SHAPES for m in (True, False)] \
    + [S.CAP_CASE + (True, "cap")]
SEQ_IDS = [f"{f}-{'mv' if m else 'still'}-{p}-" + "x".join(map(str, s)) for s, f, m, p in SEQ]


@pytest.mark.parametrize("shape,family,motion,params", SEQ, ids=SEQ_IDS)
def test_recurrence(device, shape, family, motion, params):
    """The whole recurrence over T = 6 frames, with and without motion vectors:
    colour and variance of every frame; masks and lengths through the chained
    accumulation (neither depends on a colour)."""
    import nsm_amd
    data, r64, r32 = S.reference(shape, family, motion, params)
    kw = dict(S.CAP if params == "cap" else S.PARAMS)
    frames, mvs, depth, normals = case(device, shape, family)
    mvs = mvs if motion else None
    out, var = nsm_amd.svgf(frames, mvs, depth=depth, normals=normals, return_variance=True,
                            **kw, **REJECT)
    assert out.shape == (S.T,) + shape and out.dtype == torch.float32
    assert var.shape == (S.T, shape[0], 1) + shape[2:]
    worst = [0.0, 0.0]
    for t in range(S.T):
        vmax = r64["var"][t].max().item()
        fc, fv = S.floor_sequence(t, vmax, **kw)
        what = f"{family} {shape} mv={motion} {params} frame {t}"
        worst[0] = max(worst[0], close(out[t], r64["out"][t], r32["out"][t], fc, what + " colour"))
        worst[1] = max(worst[1], close(var[t], r64["var"][t], r32["var"][t], fv, what + " var"))
    print(f"WORST {family} {shape} mv={motion} {params}: colour {worst[0]:.2e} var {worst[1]:.2e}")
    hist = None
    for t in range(S.T):
        res = nsm_amd.svgf_accumulate(
            frames[t], mvs[t - 1] if mvs and t else None, depth=depth[t], normals=normals[t],
            prev_depth=depth[t - 1] if t else None, prev_normals=normals[t - 1] if t else None,
            history=hist, max_history=kw["max_history"], return_mask=True, **REJECT)
        assert torch.equal(res[4].cpu(), r64["accepted"][t]), t
        assert torch.equal(res[2].cpu().double(), r64["length"][t]), t
        hist = res[:3]


# ---- bitwise properties --------------------------------------------------------
def test_bitwise_properties(device):
    """Repeat, stacked form, streaming form in both buffer modes, a batch of two
    against each image alone, the identity, 16-bit inputs."""
    import nsm_amd
    frames, mvs, z, n = case(device, BIG, "planes")
    kw = dict(depth=z, normals=n, **REJECT)
    first, var = nsm_amd.svgf(frames, mvs, return_variance=True, **kw)
    again = nsm_amd.svgf(frames, mvs, **kw)
    stacked = nsm_amd.svgf(torch.stack(frames), torch.stack(mvs), depth=torch.stack(z),
                           normals=torch.stack(n), **REJECT)
    assert torch.equal(first, again) and torch.equal(first, stacked)
    assert not torch.equal(first, torch.stack(frames))
    for capturable in (False, True):
        f = nsm_amd.SVGF(capturable=capturable, return_variance=True, **REJECT)
        for rounds in range(2):
            for t, fr in enumerate(frames):
                o, v = f(fr, mvs[t - 1] if t else None, z[t], n[t])
                assert o.dtype == torch.float32 and torch.equal(o, first[t]), (capturable, t)
                assert torch.equal(v, var[t])
            f.reset()
    for fb, its in ((0, 5), (2, 5), (1, 1), (3, 2)):
        want = nsm_amd.svgf(frames, mvs, iterations=its, feedback=fb, **kw)
        f = nsm_amd.SVGF(its, feedback=fb, **REJECT)
        for t, fr in enumerate(frames):
            assert torch.equal(f(fr, mvs[t - 1] if t else None, z[t], n[t]), want[t]), (fb, its, t)
    assert torch.equal(nsm_amd.svgf(frames, mvs, iterations=2, feedback=3, **kw),
                       nsm_amd.svgf(frames, mvs, iterations=2, feedback=2, **kw))
    for b in range(BIG[0]):
        alone = nsm_amd.svgf([t[b:b + 1] for t in frames], [t[b:b + 1] for t in mvs],
                             depth=[t[b:b + 1] for t in z], normals=[t[b:b + 1] for t in n], **REJECT)
        assert torch.equal(alone, first[:, b:b + 1])
    for m in (mvs, None):
        same = nsm_amd.svgf(frames, m, iterations=0, alpha=1.0, moments_alpha=1.0, **kw)
        assert torch.equal(same, torch.stack(frames))
    for dt in (torch.float16, torch.bfloat16):
        f16, z16 = [f.to(dt) for f in frames], [t.to(dt) for t in z]
        a = nsm_amd.svgf(f16, mvs, depth=z16, normals=n, **REJECT)
        b = nsm_amd.svgf([f.float() for f in f16], mvs, depth=[t.float() for t in z16], normals=n,
                         **REJECT)
        assert a.dtype == torch.float32 and torch.equal(a, b) and not torch.equal(a, first)
    # three channels: the ops compose to the recurrence
    frames, mvs, z, n = case(device, (1, 3, 8, 5), "planes")
    want = nsm_amd.svgf(frames[:1], None, depth=z[:1], normals=n[:1], iterations=2)[0]
    c, m, ln, v = nsm_amd.svgf_accumulate(frames[0])
    c, v = nsm_amd.svgf_variance(c, m, ln, v, z[0], n[0])
    for step in (1, 2):
        c, v = nsm_amd.atrous_filter(c, z[0], n[0], v, step=step)
    assert torch.equal(c, want)


def test_graph_capture(device):
    """One SVGF(capturable=True) call captured in torch.cuda.graph and replayed
    over the sequence through static inputs equals the eager frames bitwise."""
    import nsm_amd
    shape = (2, 1, 19, 37)
    frames, mvs, z, n = case(device, shape, "planes")
    want = nsm_amd.svgf(frames, mvs, depth=z, normals=n, **REJECT)
    f = nsm_amd.SVGF(capturable=True, **REJECT)
    f(frames[0], None, z[0], n[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up: kernels loaded, allocator primed
        f(frames[1], mvs[0], z[1], n[1])
    torch.cuda.current_stream().wait_stream(side)
    cf, cm, cz, cn = (torch.empty_like(t[0]) for t in (frames, mvs, z, n))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = f(cf, cm, cz, cn)
    f.reset()
    assert torch.equal(f(frames[0], None, z[0], n[0]), want[0])
    for t in range(1, S.T):
        for dst, src in ((cf, frames[t]), (cm, mvs[t - 1]), (cz, z[t]), (cn, n[t])):
            dst.copy_(src)
        g.replay()
        assert torch.equal(res, want[t]), t


# ---- edges ---------------------------------------------------------------------
@pytest.mark.parametrize("shape,scale", [((1, 1, 1, 7), (1.0, 0.0)), ((1, 3, 5, 1), (0.0, 1.0)),
                                         ((1, 1, 1, 1), (0.0, 0.0)), ((2, 1, 1, 1), (1.0, 1.0))],
                         ids=["1x7", "5x1", "1x1", "1x1-rejected"])
def test_degenerate_planes(device, shape, scale):
    """One row, one column and one pixel: the gradient vanishes along the
    missing axis, most taps are outside; the motion along a missing axis is
    switched off so that pixels are accepted."""
    import nsm_amd
    frames, mvs, depth, normals, _ = S.random_inputs(shape)
    kw = dict(S.PARAMS, sigma_n=2.0)
    r64, r32 = (S.sequence(frames, mvs, depth, normals, scale=scale, dtype=dt, **kw)
                for dt in (torch.float64, torch.float32))
    out, var = nsm_amd.svgf(dev_seq(device, frames), dev_seq(device, mvs),
                            depth=dev_seq(device, depth), normals=dev_seq(device, normals),
                            mv_scale=scale, return_variance=True, **kw, **REJECT)
    if scale != (1.0, 1.0):
        assert any(a.any() for a in r64["accepted"])
    for t in range(S.T):
        fc, fv = S.floor_sequence(t, r64["var"][t].max().item(), **kw)
        close(out[t], r64["out"][t], r32["out"][t], fc, f"{shape} frame {t} colour")
        close(var[t], r64["var"][t], r32["var"][t], fv, f"{shape} frame {t} var")


WILD = [float("nan"), float("inf"), float("-inf"), 1e30, -1e30]


def test_wild_motion_vectors_are_rejected(device):
    import nsm_amd
    shape = (2, 1, 19, 37)
    frames, mvs, z, n = case(device, shape, "planes")
    B, _, H, W = shape
    wild = torch.tensor(WILD)[torch.arange(B * H * W) % len(WILD)].view(B, H, W)
    hit = torch.zeros(B, H, W, dtype=torch.bool)
    hit[:, ::2, 1::3] = True
    mv = mvs[0].cpu().clone()
    mv[:, 0][hit] = wild[hit]
    mv[:, 1, ::4][hit[:, ::4]] = wild.flip(2)[:, ::4][hit[:, ::4]]
    hist = nsm_amd.svgf_accumulate(frames[0])[:3]
    kw = dict(depth=z[1], normals=n[1], prev_depth=z[0], prev_normals=n[0], history=hist,
              return_mask=True, **REJECT)
    c, m, ln, v, acc = (t.cpu() for t in nsm_amd.svgf_accumulate(frames[1], mv.to(device), **kw))
    plain = [t.cpu() for t in nsm_amd.svgf_accumulate(frames[1], mvs[0], **kw)]
    hit = hit.unsqueeze(1)
    assert all(torch.isfinite(t).all() for t in (c, m, ln, v))
    assert not acc[hit].any() and acc.any() and (ln[hit] == 1).all() and (ln[acc] == 2).all()
    assert torch.equal(c[hit], frames[1].cpu()[hit]) and (v[hit] == 0).all()
    for got, ref in zip((c, ln, v, acc), (plain[0], plain[2], plain[3], plain[4])):
        assert torch.equal(got[~hit], ref[~hit])
    out = nsm_amd.svgf(frames[:2], [mv.to(device)], depth=z[:2], normals=n[:2], **REJECT)
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_no_out_of_image_reads(device, shape):
    """Every input is a contiguous slice of ONE NaN-filled buffer with NaN
    margins on both sides: a tap outside an image would carry a NaN into the
    result. The results are NaN-free and bitwise those from stand-alone tensors."""
    import nsm_amd
    frames, mvs, depth, normals, _ = S.inputs(shape, "planes")
    seqs = (frames, mvs, depth, normals)
    margin = 4 * shape[3] * 17 + 64     # beyond any tap of step 16 in any direction
    total = sum(t.numel() + margin for s in seqs for t in s) + 2 * shape[1] * (
        frames[0].numel() + margin) + margin
    buf = torch.full((total,), float("nan"), dtype=torch.float32, device=device)
    at = [margin]

    def guarded(t):
        view = buf[at[0]:at[0] + t.numel()].view(t.shape)
        at[0] += t.numel() + margin
        view.copy_(t)
        return view

    gf, gm, gz, gn = ([guarded(t) for t in s] for s in seqs)
    pf, pm, pz, pn = (dev_seq(device, s) for s in seqs)
    got = nsm_amd.svgf(gf, gm, depth=gz, normals=gn, return_variance=True, **REJECT)
    ref = nsm_amd.svgf(pf, pm, depth=pz, normals=pn, return_variance=True, **REJECT)
    for a, b in zip(got, ref):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    var = guarded(ref[1][0])
    for step in (1, 2, 4, 8, 16):
        o = guarded(torch.zeros(shape))
        a, av = nsm_amd.atrous_filter(gf[0], gz[0], gn[0], var, step=step, out=o)
        b, bv = nsm_amd.atrous_filter(pf[0], pz[0], pn[0], ref[1][0], step=step)
        assert a is o and torch.isfinite(a).all() and torch.isfinite(av).all()
        assert torch.equal(a, b) and torch.equal(av, bv)
        at[0] -= o.numel() + margin
        o.fill_(float("nan"))
    assert torch.isnan(buf[:margin]).all() and torch.isnan(buf[-margin:]).all()


def test_edge_stopping(device):
    """A colour of exactly 0 and 1 on the two sides of the "planes" edge with a
    variance of 0.01: five iterations at sigma_n = 128 leave each side within the
    restatement's own leakage (plus the accuracy bound); with sigma_z and
    sigma_n neutralised the same input blurs across the edge."""
    import nsm_amd
    shape = (2, 1, 19, 37)
    _, _, depth, normals, _ = S.inputs(shape, "planes")
    side = S.edge_side(shape).expand(shape)
    color = side.float().contiguous()
    var = torch.full(shape, 0.01)
    assert side.any() and not side.all()
    z, n = depth[0].to(device), normals[0].to(device)
    for sz, sn, stops in ((1.0, 128.0, True), (1e30, 0.0, False)):
        c64, v64, c32, v32 = color.double(), var.double(), color, var
        gc, gv = color.to(device), var.to(device)
        for i in range(5):
            c64, v64, _ = S.atrous(c64, v64, depth[0], normals[0], 1 << i, sz, sn, 4.0)
            c32, v32, _ = S.atrous(c32, v32, depth[0], normals[0], 1 << i, sz, sn, 4.0,
                                   dtype=torch.float32)
            gc, gv = nsm_amd.atrous_filter(gc, z, n, gv, step=1 << i, sigma_z=sz, sigma_n=sn)
        lim, _ = S.bound(c64, c32, 5 * S.floor_color(sn))
        leak64 = max(c64[~side].max().item(), 1 - c64[side].min().item())
        leak = max(gc.cpu()[~side].max().item(), 1 - gc.cpu()[side].min().item())
        print(f"sigma_z {sz:g} sigma_n {sn:g}: leakage {leak:.3e} (restatement {leak64:.3e}, "
              f"bound {lim:.2e})")
        assert (gc.cpu().double() - c64).abs().max().item() <= lim
        if stops:
            assert leak <= leak64 + lim and leak64 < 1e-6
        else:
            # only the luminance term is left: |dl| / phi_l = 1 / (4 sqrt(0.01)) = 2.5
            # at the first iteration, so the pixel next to the edge takes its
            # neighbour across it at h(0) h(1) exp(-2.5) = 7.7e-3 of a total weight
            # below 1; later iterations spread that, they do not undo it
            assert leak > 1e-3 and leak64 > 1e-3


# ---- the direction of the effect -------------------------------------------------
def test_denoises_and_stabilises(device):
    """On "planes" the denoised sequence has at most 0.25 of the noisy input's
    MSE against the clean signal and a lower temporal instability."""
    import nsm_amd
    frames, mvs, depth, normals, clean = S.inputs(BIG, "planes")
    fd, md, zd, nd = (dev_seq(device, s) for s in (frames, mvs, depth, normals))
    out = nsm_amd.svgf(fd, md, depth=zd, normals=nd, **REJECT)
    truth = torch.stack(clean).to(device)
    mse_in = (torch.stack(fd) - truth).pow(2).mean().item()
    mse_out = (out - truth).pow(2).mean().item()
    kw = dict(depth=zd, normals=nd, **REJECT)
    e_in = nsm_amd.measure_temporal_instability(fd, md, **kw).item()
    e_out = nsm_amd.measure_temporal_instability(out, md, **kw).item()
    print(f"MSE {mse_in:.5f} -> {mse_out:.5f} ({mse_out / mse_in:.3f}); "
          f"temporal instability {e_in:.4f} -> {e_out:.4f}")
    assert mse_out <= 0.25 * mse_in
    assert e_out < e_in


# ---- argument errors -------------------------------------------------------------
def test_argument_errors(device):
    """Each listed mistake raises ValueError (before any GPU work: the checks
    read shapes, types and devices only)."""
    import nsm_amd
    shape = (2, 1, 19, 37)
    frames, mvs, z, n = case(device, shape, "planes")
    ok = dict(depth=z, normals=n)
    bad_calls = [
        lambda: nsm_amd.svgf([f[0] for f in frames], mvs, **ok),                 # rank
        lambda: nsm_amd.svgf(frames, mvs[:-1], **ok),                            # length
        lambda: nsm_amd.svgf(frames, mvs, depth=z[:-1], normals=n),
        lambda: nsm_amd.svgf(frames, mvs, depth=z, normals=z),                   # shape
        lambda: nsm_amd.svgf(frames, [m[:, :1] for m in mvs], **ok),
        lambda: nsm_amd.svgf([f.expand(2, 2, 19, 37) for f in frames], mvs, **ok),   # C = 2
        lambda: nsm_amd.svgf(frames, mvs, depth=None, normals=n),
        lambda: nsm_amd.svgf(frames, mvs, depth=z, normals=None),
        lambda: nsm_amd.svgf(frames, mvs, iterations=-1, **ok),
        lambda: nsm_amd.svgf(frames, mvs, alpha=0.0, **ok),
        lambda: nsm_amd.svgf(frames, mvs, alpha=1.5, **ok),
        lambda: nsm_amd.svgf(frames, mvs, moments_alpha=0.0, **ok),
        lambda: nsm_amd.svgf(frames, mvs, moments_alpha=float("nan"), **ok),
        lambda: nsm_amd.svgf(frames, mvs, max_history=0, **ok),
        lambda: nsm_amd.svgf([f.cpu() for f in frames], mvs, **ok),              # CPU tensors
        lambda: nsm_amd.svgf(frames, mvs, depth=[t.cpu() for t in z], normals=n),
        lambda: nsm_amd.svgf([], None, depth=[], normals=[]),
        lambda: nsm_amd.atrous_filter(frames[0], z[0], n[0], out=frames[0]),     # aliasing
        lambda: nsm_amd.atrous_filter(frames[0], z[0], n[0], out=z[0]),
        lambda: nsm_amd.atrous_filter(frames[0], z[0], n[0], z[0], out=z[0]),
        lambda: nsm_amd.atrous_filter(frames[0], z[0], n[0], step=0),
        lambda: nsm_amd.atrous_filter(frames[0].cpu(), z[0], n[0]),
        lambda: nsm_amd.atrous_filter(frames[0], z[0], z[0]),
        lambda: nsm_amd.atrous_filter(frames[0], None, n[0]),
        lambda: nsm_amd.svgf_accumulate(frames[1], mvs[0], history=(frames[0],) * 3),
        lambda: nsm_amd.svgf_accumulate(frames[1], alpha=0.0),
        lambda: nsm_amd.svgf_accumulate(frames[1], max_history=0),
        lambda: nsm_amd.svgf_variance(frames[0], frames[0], z[0], z[0], z[0], n[0]),
        lambda: nsm_amd.SVGF(iterations=-1),
        lambda: nsm_amd.SVGF(alpha=2.0),
        lambda: nsm_amd.SVGF()(frames[0], None, None, n[0]),
        lambda: nsm_amd.SVGF()(frames[0], None, z[0], None),
        lambda: nsm_amd.SVGF()(frames[0].cpu(), None, z[0], n[0]),
    ]
    for i, f in enumerate(bad_calls):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"call {i} did not raise")
    f = nsm_amd.SVGF()
    f(frames[0], None, z[0], n[0])
    with pytest.raises(ValueError):
        f(frames[1][:, :, :5], None, z[1][:, :, :5], n[1][:, :, :5])
