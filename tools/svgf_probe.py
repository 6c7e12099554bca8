#!/usr/bin/env python3
"""Time the SVGF denoiser (nsm_svgf_accumulate / _variance / _atrous,
nsm_amd/svgf.py) with HIP events, and in the same process what it is measured
against:

  * each kernel alone (the a-trous iteration at every step 1 to 16, with the
    luminance term and as the plain depth-aware post filter), against a
    device-to-device copy of the bytes the pass must move, measured before and
    after so that its own spread shows;
  * the whole frame (SVGF streaming call: accumulate, variance fallback, five
    a-trous iterations, history hand-over) against the float32 restatement of
    the same passes from ATen ops on the GPU (what a user would otherwise run),
    and the error of one a-trous iteration of each against the same ATen ops in
    float64.

    python tools/svgf_probe.py [--shape 1x1x1080x1920] [--frames 4] [--reps 20]

Median (min .. max) of --reps after warm-up; kernel-only figures from 10
back-to-back launches per event pair over --frames different frame sets. Bytes
a pass must move, counted from shapes, per pixel (each plane once: neighbouring
pixels share taps): a-trous 8C + 24 (colour, variance, depth, normals in;
colour, variance out; 8C + 16 without variance), variance fallback 8C + 36,
accumulate 12C + 68 (both frames' depth and normals, motion vectors, history
colour, moments and length in; colour, moments, length, variance out). The
inputs are a planar two-region scene with noise (tests/svgf_util.py's "planes"
in the large), so that most tap weights are alive as in a rendered frame.
Prints one line per measurement and a final JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import nsm_amd  # noqa: E402
V = sys.modules["nsm_amd.svgf"]   # the module: nsm_amd.svgf is the function it exports

DEPTH_TOL, NORMAL_COS = 0.3, 0.2
SZ, SN, SL = 1.0, 128.0, 4.0
H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed_ms(fn, n, warmup=3):
    """(median, min, max) of n timings of fn()."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[n // 2], ts[0], ts[-1]


def fmt(t, div=1.0):
    return [round(v / div, 4) for v in t]


# ---- the float32 restatement from ATen ops -------------------------------------
def lum(c):
    return c[:, 0] if c.shape[1] == 1 else 0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]


def grad(z):
    p = F.pad(z, (1, 1, 1, 1), mode="replicate")
    H, W = z.shape[-2:]
    den_x = torch.full((W,), 2.0, device=z.device, dtype=z.dtype)
    den_y = torch.full((H, 1), 2.0, device=z.device, dtype=z.dtype)
    den_x[0] = den_x[-1] = den_y[0] = den_y[-1] = 1.0
    gx = (p[:, 0, 1:-1, 2:] - p[:, 0, 1:-1, :-2]) / den_x if W > 1 else torch.zeros_like(z[:, 0])
    gy = (p[:, 0, 2:, 1:-1] - p[:, 0, :-2, 1:-1]) / den_y if H > 1 else torch.zeros_like(z[:, 0])
    return gx, gy


def taps(planes, P, offsets):
    """planes zero-padded by P once; yields ((ox, oy), views..., inside) per offset."""
    H, W = planes[0].shape[-2:]
    padded = [F.pad(t, (P, P, P, P)) for t in planes]
    ones = F.pad(torch.ones(1, 1, H, W, device=planes[0].device, dtype=planes[0].dtype),
                 (P, P, P, P))
    for ox, oy in offsets:
        sl = (slice(None), slice(None), slice(P + oy, P + oy + H), slice(P + ox, P + ox + W))
        yield (ox, oy), [t[sl] for t in padded], ones[sl][:, 0]


def edge_exponent(z, n, g, zq, nq, ox, oy, sz, sn):
    ez = (z[:, 0] - zq[:, 0]).abs() / (sz * (g[0] * ox + g[1] * oy).abs() + 1e-8)
    return ez, (n * nq).sum(1).clamp(min=0) ** sn


def aten_atrous(c, v, z, n, step, sz=SZ, sn=SN, sl=SL):
    g, l = grad(z), lum(c)
    if v is not None:
        k = torch.tensor([[1, 2, 1], [2, 4, 2], [1, 2, 1]], device=c.device, dtype=c.dtype) / 16
        gv = F.conv2d(F.pad(v, (1, 1, 1, 1), mode="replicate"), k.view(1, 1, 3, 3))[:, 0]
        phi = sl * torch.sqrt(gv.clamp(min=0) + 1e-10)
    w0 = H5[2] * H5[2]
    sw, sc = torch.full_like(l, w0), w0 * c
    sv = w0 * w0 * v if v is not None else None
    offs = [(dx * step, dy * step) for dy in range(-2, 3) for dx in range(-2, 3) if dx or dy]
    planes = [c, z, n] + ([v] if v is not None else [])
    for (ox, oy), q, inside in taps(planes, 2 * step, offs):
        ez, wn = edge_exponent(z, n, g, q[1], q[2], ox, oy, sz, sn)
        e = ez + (l - lum(q[0])).abs() / phi if v is not None else ez
        w = H5[ox // step + 2] * H5[oy // step + 2] * torch.exp(-e) * wn * inside
        sw = sw + w
        sc = sc + w.unsqueeze(1) * q[0]
        if v is not None:
            sv = sv + (w * w).unsqueeze(1) * q[3]
    return sc / sw.unsqueeze(1), sv / (sw * sw).unsqueeze(1) if v is not None else None


def aten_variance(c, m, N, v, z, n, min_history=4, sz=SZ, sn=SN):
    g = grad(z)
    sw, sc, sm = torch.ones_like(z[:, 0]), c.clone(), m.clone()
    offs = [(dx, dy) for dy in range(-3, 4) for dx in range(-3, 4) if dx or dy]
    for (ox, oy), q, inside in taps([c, z, n, m], 3, offs):
        ez, wn = edge_exponent(z, n, g, q[1], q[2], ox, oy, sz, sn)
        w = (torch.exp(-ez) * wn * inside).unsqueeze(1)
        sw, sc, sm = sw + w[:, 0], sc + w * q[0], sm + w * q[3]
    M = sm / sw.unsqueeze(1)
    est = (M[:, 1:2] - M[:, 0:1] ** 2).clamp(min=0) * (min_history / N)
    short = N < min_history
    return torch.where(short, sc / sw.unsqueeze(1), c), torch.where(short, est, v)


def aten_accumulate(cur, z, n, zp, np_, mv, hist, alpha=0.2, max_history=32):
    B, C, H, W = cur.shape
    l = lum(cur).unsqueeze(1)
    if hist is None:
        return cur, torch.cat([l, l * l], 1), torch.ones_like(l), torch.zeros_like(l)
    x = torch.arange(W, device=cur.device, dtype=cur.dtype).view(1, 1, W)
    y = torch.arange(H, device=cur.device, dtype=cur.dtype).view(1, H, 1)
    px, py = x + mv[:, 0], y + mv[:, 1]
    ok = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    grid = torch.stack([2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1], dim=-1)
    s = F.grid_sample(torch.cat([hist[0], hist[1], zp, np_], 1), grid, mode="bilinear",
                      padding_mode="border", align_corners=True)
    hn = F.grid_sample(hist[2], grid, mode="nearest", padding_mode="border", align_corners=True)
    ok &= (z[:, 0] - s[:, C + 2]).abs() <= DEPTH_TOL * z[:, 0].abs()
    ok &= (n * s[:, C + 3:]).sum(1) >= NORMAL_COS
    ok = ok.unsqueeze(1)
    N = torch.where(ok, (hn + 1).clamp(max=max_history), torch.ones_like(hn))
    a = torch.clamp(1 / N, min=alpha)
    c = torch.where(ok, cur + (1 - a) * (s[:, :C] - cur), cur)
    m1 = torch.where(ok, l + (1 - a) * (s[:, C:C + 1] - l), l)
    m2 = torch.where(ok, l * l + (1 - a) * (s[:, C + 1:C + 2] - l * l), l * l)
    return c, torch.cat([m1, m2], 1), N, (m2 - m1 * m1).clamp(min=0)


class AtenSVGF:
    """SVGF (defaults) from ATen ops in float32, streaming."""

    def __init__(self, iterations=5):
        self.iterations, self.hist, self.z, self.n = iterations, None, None, None

    def __call__(self, cur, mv, z, n):
        c, m, N, v = aten_accumulate(cur, z, n, self.z, self.n, mv, self.hist)
        keep = c
        c, v = aten_variance(c, m, N, v, z, n)
        for i in range(self.iterations):
            c, v = aten_atrous(c, v, z, n, 1 << i)
            if i == 0:
                keep = c
        self.hist, self.z, self.n = (keep, m, N), z, n
        return c


def scene(B, C, H, W, n, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    frames, mvs, depth, normals = [], [], [], []
    for t in range(n):
        u = (torch.arange(W, device=dev, dtype=torch.float32) - 1.25 * t).view(1, 1, 1, W)
        v = (torch.arange(H, device=dev, dtype=torch.float32) + 0.75 * t).view(1, 1, H, 1)
        side = ((u - W / 2) * 0.94 + (v - H / 2) * 0.34) > 0.05
        z = torch.where(side, 9.0 - 0.0009 * u + 0.00172 * v, 1.2 + 0.0013 * u + 0.00071 * v)
        depth.append(z.expand(B, 1, H, W).contiguous())
        base = torch.where(side.expand(1, 3, H, W),
                           torch.tensor([-0.5, 0.3, 0.8], device=dev).view(1, 3, 1, 1),
                           torch.tensor([0.2, 0.1, 1.0], device=dev).view(1, 3, 1, 1))
        normals.append(F.normalize(base + 0.02 * torch.randn(B, 3, H, W, device=dev, generator=g),
                                   dim=1))
        s = 0.5 + 0.2 * torch.tanh((0.8 * (u - 0.45 * W) + 0.6 * (v - 0.5 * H)) / (0.3 * max(H, W)))
        frames.append((s + 0.15 * torch.randn(B, C, H, W, device=dev, generator=g)).clamp(0, 1))
        mv = torch.empty(B, 2, H, W, device=dev)
        mv[:, 0], mv[:, 1] = -1.25, 0.75
        mvs.append(mv)
    return frames, mvs, depth, normals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x1x1080x1920")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--aten-reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, C, H, W = (int(v) for v in args.shape.split("x"))
    n, pix = args.frames, B * H * W
    frames, mvs, depth, normals = scene(B, C, H, W, n, dev)
    rec = {"shape": [B, C, H, W], "frames": n, "lib": os.path.basename(nsm_amd.LIB_PATH)}

    def new(ch):
        return [torch.empty(B, ch, H, W, device=dev) for _ in range(n)]

    # realistic pass inputs: frame t accumulated on frame t-1's first-frame state
    state = [nsm_amd.svgf_accumulate(f) for f in frames]
    acc = [nsm_amd.svgf_accumulate(frames[t], mvs[t], depth=depth[t], normals=normals[t],
                                   prev_depth=depth[t - 1], prev_normals=normals[t - 1],
                                   history=state[t - 1][:3], depth_tol=DEPTH_TOL,
                                   normal_cos=NORMAL_COS) for t in range(n)]
    oc, om, on, ov, oc2, ov2 = new(C), new(2), new(1), new(1), new(C), new(1)
    var = [nsm_amd.svgf_variance(*acc[t], depth[t], normals[t])[1] for t in range(n)]

    def copy_ms(bytes_per_pixel):
        words = pix * bytes_per_pixel // 8      # half read, half written
        src = [torch.empty(words, device=dev) for _ in range(n)]
        dst = [torch.empty(words, device=dev) for _ in range(n)]

        def run():
            for i in range(10):
                dst[i % n].copy_(src[i % n])
        return fmt(timed_ms(run, args.reps), 10)

    def ten(fn):
        def run():
            for i in range(10):
                fn(i % n)
        return fmt(timed_ms(run, args.reps), 10)

    def report(name, ms, bpp, copy):
        r = {"ms_median_min_max": ms, "bytes_per_pixel": bpp,
             "TB_per_s": round(pix * bpp / (ms[0] * 1e-3) / 1e12, 2),
             "copy_ms_before_after": copy, "over_copy": round(ms[0] / min(c[0] for c in copy), 2)}
        rec[name] = r
        print(f"{args.shape} {name}: {ms[0]:.4f} ms ({ms[1]:.4f} .. {ms[2]:.4f}) = {r['TB_per_s']} "
              f"TB/s of {bpp} B/pixel; copy of the same bytes {[c[0] for c in copy]} ms "
              f"({r['over_copy']}x)", flush=True)

    bpp = 12 * C + 68
    before = copy_ms(bpp)
    ms = ten(lambda t: V._accumulate(frames[t], depth[t], normals[t], depth[t - 1], normals[t - 1],
                                     mvs[t], state[t - 1][:3], (1.0, 1.0), 0.2, 0.2, 32, DEPTH_TOL,
                                     NORMAL_COS, oc[t], om[t], on[t], ov[t]))
    report("accumulate", ms, bpp, [before, copy_ms(bpp)])
    bpp = 8 * C + 36
    before = copy_ms(bpp)
    ms = ten(lambda t: V._variance(acc[t][0], acc[t][1], acc[t][2], acc[t][3], depth[t], normals[t],
                                   4, SZ, SN, oc[t], ov[t]))
    report("variance_all_short", ms, bpp, [before, copy_ms(bpp)])
    ms = ten(lambda t: V._variance(acc[t][0], acc[t][1], acc[t][2], acc[t][3], depth[t], normals[t],
                                   1, SZ, SN, oc[t], ov[t]))
    report("variance_all_through", ms, bpp, [before, copy_ms(bpp)])
    bpp = 8 * C + 24
    before = copy_ms(bpp)
    for step in (1, 2, 4, 8, 16):
        ms = ten(lambda t: V._atrous(acc[t][0], var[t], depth[t], normals[t], step, SZ, SN, SL,
                                     oc2[t], ov2[t]))
        report(f"atrous_step{step}", ms, bpp, [before, copy_ms(bpp)])
    ms = ten(lambda t: V._atrous(acc[t][0], None, depth[t], normals[t], 1, SZ, SN, 0.0, oc2[t],
                                 None))
    report("atrous_step1_post_filter", ms, 8 * C + 16, [copy_ms(8 * C + 16)])

    # the whole frame, streaming over the n frame sets, against ATen
    kw = dict(depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
    fused, aten = nsm_amd.SVGF(**kw), AtenSVGF()
    fused(frames[0], None, depth[0], normals[0])
    aten.hist, aten.z, aten.n = state[0][:3], depth[0], normals[0]

    def stream(obj):
        def run():
            for t in range(n):
                obj(frames[t], mvs[t], depth[t], normals[t])
        return run

    rec["frame_ms_median_min_max"] = fmt(timed_ms(stream(fused), args.reps), n)
    rec["aten_frame_ms_median_min_max"] = fmt(timed_ms(stream(aten), args.aten_reps, warmup=1), n)
    rec["speedup_vs_aten"] = round(rec["aten_frame_ms_median_min_max"][0]
                                   / rec["frame_ms_median_min_max"][0], 1)
    # one a-trous iteration of each against the same ATen ops in float64
    t = n - 1
    a, av = nsm_amd.atrous_filter(acc[t][0], depth[t], normals[t], var[t], step=2)
    b, bv = aten_atrous(acc[t][0], var[t], depth[t], normals[t], 2)
    r, rv = aten_atrous(acc[t][0].double(), var[t].double(), depth[t].double(),
                        normals[t].double(), 2)
    rec["max_abs_err_vs_f64"] = [float((a.double() - r).abs().max()),
                                 float((av.double() - rv).abs().max())]
    rec["aten_max_abs_err_vs_f64"] = [float((b.double() - r).abs().max()),
                                      float((bv.double() - rv).abs().max())]
    print(f"{args.shape} frame: {rec['frame_ms_median_min_max']} ms vs ATen "
          f"{rec['aten_frame_ms_median_min_max']} ms ({rec['speedup_vs_aten']}x); one a-trous "
          f"iteration against ATen in float64 (colour, variance): max|d| "
          f"{rec['max_abs_err_vs_f64']} (ATen float32 {rec['aten_max_abs_err_vs_f64']})", flush=True)
    print(json.dumps({"svgf_probe": rec}))


if __name__ == "__main__":
    main()
