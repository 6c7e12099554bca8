#!/usr/bin/env python3
"""Time the learned feature extraction (nsm_amd.FeatureExtractor, csrc/nsm_extract.hip)
with HIP events, and in the same process, interleaved, what it is measured against:

  * the ATen route: the same nn.Sequential (Conv2d 1x1, LeakyReLU, Conv2d 1x1) from
    ATen ops, on contiguous and on channels_last input, the faster of the two taken;
    its result is compared with the fused one before anything is timed;
  * the copy ceiling: a device-to-device copy of the bytes the fused passes must
    move (forward: Cin + Cout planes; backward: Cin + Cout read, Cin more written
    with dx).

    python tools/extract_probe.py [--shapes 8x15x512x512,1x15x1080x1920] [--reps 20]
                                  [--no-aten] [--step]

Three passes per shape: forward (no_grad), forward + backward without dx, and with
dx (x.requires_grad), through the module and autograd; and the C entries alone on
preallocated buffers, the passes without the module's host work. Median and range of
--reps rounds after warm-up; a round times INNER back-to-back calls of each route in turn, so the routes see the same machine.
Inputs rotate over enough buffers to exceed the 256 MB Infinity Cache. The peak
memory of one forward + backward above what was allocated before it is reported for
both routes. --step adds GraphedTrainStep frames/s of ExtractedUnet(15 -> 4) against
the plain Unet(in_ch=4) on 8x512x512 crops, fp32 and bf16. Prints one line per case
and a final JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import nsm_amd  # noqa: E402
from nsm_amd._lib import call, lib, ptr, stream  # noqa: E402

INNER = 5
COUT, HIDDEN, SLOPE = 4, 16, 0.2


def summarize(ts):
    ts = sorted(ts)
    return round(ts[len(ts) // 2], 4), [round(ts[0], 4), round(ts[-1], 4)]


def time_routes(routes, reps):
    times = {k: [] for k in routes}
    t = 0
    for rnd in range(reps + 3):                               # 3 warm-up rounds
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER):
                t += 1
                fn(t)
            e1.record()
            torch.cuda.synchronize()
            if rnd >= 3:
                times[name].append(e0.elapsed_time(e1) / INNER)
    return times


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn(0)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def probe_shape(shape, reps, aten, dev, g):
    B, Cin, H, W = (int(v) for v in shape.split("x"))
    fused = nsm_amd.FeatureExtractor(Cin, COUT, HIDDEN, SLOPE).to(dev)
    plain = nn.Sequential(nn.Conv2d(Cin, HIDDEN, 1), nn.LeakyReLU(SLOPE),
                          nn.Conv2d(HIDDEN, COUT, 1)).to(dev)
    plain.load_state_dict(fused.net.state_dict())
    plane = 4 * B * H * W
    sets = max(2, -(-(512 << 20) // (Cin * plane)))
    xs = [torch.randn((B, Cin, H, W), device=dev, generator=g) for _ in range(sets)]
    xs_cl = [x.contiguous(memory_format=torch.channels_last) for x in xs] if aten else []
    xg = [x.clone().requires_grad_(True) for x in xs[:2]]
    xg_cl = [x.detach().clone(memory_format=torch.channels_last).requires_grad_(True)
             for x in xs[:2]] if aten else []
    dy = torch.randn((B, COUT, H, W), device=dev, generator=g)
    dy_cl = dy.contiguous(memory_format=torch.channels_last)

    def fwd(mod, pool):
        def f(t):
            with torch.no_grad():
                mod(pool[t % len(pool)])
        return f

    def fb(mod, pool, d):
        def f(t):
            x = pool[t % len(pool)]
            mod(x).backward(d)
            x.grad = None
            mod.zero_grad(set_to_none=True)
        return f

    nbytes = {"fwd": (Cin + COUT) * plane, "fwd_bwd": 2 * (Cin + COUT) * plane,
              "fwd_bwd_dx": (3 * Cin + 2 * COUT) * plane}
    copies = {}
    for k, n in nbytes.items():
        half = n // 2
        cs = max(2, -(-(512 << 20) // n))
        src = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(cs)]
        dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(cs)]
        copies[k] = (lambda s, d: lambda t: d[t % len(d)].copy_(s[t % len(s)]))(src, dst)

    # the routes agree before anything is timed
    with torch.no_grad():
        a, b = fused(xs[0]), plain(xs[0])
    diff = float((a - b).abs().max())
    assert diff <= 1e-4 * float(b.abs().max()), diff

    routes = {"fused_fwd": fwd(fused, xs), "fused_fwd_bwd": fb(fused, xs, dy),
              "fused_fwd_bwd_dx": fb(fused, xg, dy)}
    routes.update({"copy_" + k: f for k, f in copies.items()})
    # the C entries alone on preallocated buffers: the passes without the module's host work
    c1, c2 = fused.net[0], fused.net[2]
    pw = [ptr(c1.weight), ptr(c1.bias), ptr(c2.weight), ptr(c2.bias)]
    grads = [torch.empty_like(p) for p in (c1.weight, c1.bias, c2.weight, c2.bias)]
    gw = [ptr(t) for t in grads]
    keep = [torch.empty((B, COUT, H, W), device=dev), torch.empty((B, Cin, H, W), device=dev),
            torch.empty(lib.nsm_extract_bwd_ws(B, Cin, H, W, HIDDEN, COUT) // 4, device=dev)]
    yo, dxo, ws = (ptr(t) for t in keep)

    def k_fwd(t):
        call("nsm_extract_fwd", ptr(xs[t % sets]), B, Cin, H, W, pw[0], pw[1], HIDDEN, pw[2], pw[3],
             COUT, SLOPE, yo, stream())

    def k_bwd(dx):
        def f(t):
            call("nsm_extract_bwd", ptr(xs[t % sets]), ptr(dy), B, Cin, H, W, pw[0], pw[1], HIDDEN,
                 pw[2], pw[3], COUT, SLOPE, gw[0], gw[1], gw[2], gw[3], dx, ws, stream())
        return f
    routes.update({"kernel_fwd": k_fwd, "kernel_bwd": k_bwd(None), "kernel_bwd_dx": k_bwd(dxo)})
    if aten:
        routes.update({"aten_fwd": fwd(plain, xs), "aten_fwd_bwd": fb(plain, xs, dy),
                       "aten_fwd_bwd_dx": fb(plain, xg, dy),
                       "aten_cl_fwd": fwd(plain, xs_cl), "aten_cl_fwd_bwd": fb(plain, xs_cl, dy_cl),
                       "aten_cl_fwd_bwd_dx": fb(plain, xg_cl, dy_cl)})
    times = time_routes(routes, reps)
    r = {"bytes": nbytes, "sets": sets, "max_abs_diff_vs_aten": diff}
    for name, ts in times.items():
        r[name + "_ms"], r[name + "_ms_range"] = summarize(ts)
    r["peak_bytes_fused_fwd_bwd_dx"] = peak_of(fb(fused, xg, dy))
    print(f"{shape} C entries alone: forward {r['kernel_fwd_ms']:.4f} ms {r['kernel_fwd_ms_range']}, "
          f"backward {r['kernel_bwd_ms']:.4f} ms {r['kernel_bwd_ms_range']}, backward with dx "
          f"{r['kernel_bwd_dx_ms']:.4f} ms {r['kernel_bwd_dx_ms_range']}", flush=True)
    if aten:
        r["peak_bytes_aten_fwd_bwd_dx"] = peak_of(fb(plain, xg, dy))
    for k in nbytes:
        f = r[f"fused_{k}_ms"]
        r[f"{k}_copy_over_fused"] = round(r[f"copy_{k}_ms"] / f, 2)
        line = (f"{shape} {k}: fused {f:.4f} ms {r[f'fused_{k}_ms_range']}; D2D copy of "
                f"{nbytes[k] / 1e6:.0f} MB {r[f'copy_{k}_ms']:.4f} ms (copy / fused "
                f"{r[f'{k}_copy_over_fused']})")
        if aten:
            best = min(("aten_" + k, "aten_cl_" + k), key=lambda n: r[n + "_ms"])
            r[f"{k}_aten_best"] = best
            r[f"{k}_speedup_vs_aten"] = round(r[best + "_ms"] / f, 2)
            line += (f"; ATen {r[best + '_ms']:.4f} ms {r[best + '_ms_range']} ({best}; other "
                     f"layout {r[('aten_cl_' if best == 'aten_' + k else 'aten_') + k + '_ms']:.4f}"
                     f" ms): {r[f'{k}_speedup_vs_aten']}x")
        print(line, flush=True)
    print(f"{shape} peak memory of forward + backward (dx) above the inputs: fused "
          f"{r['peak_bytes_fused_fwd_bwd_dx'] / 1e6:.1f} MB, ATen "
          f"{r.get('peak_bytes_aten_fwd_bwd_dx', 0) / 1e6:.1f} MB", flush=True)
    return r


def probe_step(reps, dev):
    """GraphedTrainStep frames/s: the cascade against the plain 4-channel U-Net."""
    out = {}
    B, H = 8, 512
    for dtype in (torch.float32, torch.bfloat16):
        steps = {}
        for name, cin in (("unet4", 4), ("extract15", 15)):
            torch.manual_seed(0)
            unet = nsm_amd.Unet(in_ch=4, dropout_rate=0.2)
            model = unet if cin == 4 else nsm_amd.ExtractedUnet(nsm_amd.FeatureExtractor(15, 4),
                                                                unet)
            model = model.to(dev).train()
            model.set_compute_dtype(dtype)
            opt = nsm_amd.FlatAdamW(model.parameters(), lr=1e-4, weight_decay=1e-3,
                                    max_grad_norm=1.0, sanitize=True, seed=1)
            crit = nsm_amd.CustomLoss(dev, 0.9, vgg_weights=False)
            x = torch.randn(B, cin, H, H, device=dev)
            y = torch.rand(B, 1, H, H, device=dev)
            steps[name] = nsm_amd.GraphedTrainStep(model, crit, opt, x, y, warmup=2)
        times = time_routes({k: (lambda s: lambda t: s())(s) for k, s in steps.items()}, reps)
        tag = "fp32" if dtype == torch.float32 else "bf16"
        for name, ts in times.items():
            med, rng = summarize(ts)
            out[f"{tag}_{name}_ms"], out[f"{tag}_{name}_ms_range"] = med, rng
            out[f"{tag}_{name}_frames_per_s"] = round(B / (med * 1e-3), 1)
        out[f"{tag}_penalty_ms"] = round(out[f"{tag}_extract15_ms"] - out[f"{tag}_unet4_ms"], 4)
        print(f"GraphedTrainStep 8x512x512 {tag}: Unet(4) {out[f'{tag}_unet4_ms']:.3f} ms "
              f"{out[f'{tag}_unet4_ms_range']} = {out[f'{tag}_unet4_frames_per_s']} frames/s; "
              f"ExtractedUnet(15 -> 4) {out[f'{tag}_extract15_ms']:.3f} ms "
              f"{out[f'{tag}_extract15_ms_range']} = {out[f'{tag}_extract15_frames_per_s']} "
              f"frames/s; penalty {out[f'{tag}_penalty_ms']:.3f} ms", flush=True)
        del steps
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x15x512x512,1x15x1080x1920")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-aten", action="store_true", help="time the fused passes and the copy only")
    ap.add_argument("--step", action="store_true", help="GraphedTrainStep frames/s too")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rec = {"lib": os.path.basename(nsm_amd.LIB_PATH), "net": [HIDDEN, COUT, SLOPE]}
    for shape in filter(None, args.shapes.split(",")):
        rec[shape] = probe_shape(shape, args.reps, not args.no_aten, dev, g)
        torch.cuda.empty_cache()
    if args.step:
        rec["step"] = probe_step(args.reps, dev)
    print(json.dumps({"extract_probe": rec}))


if __name__ == "__main__":
    main()
