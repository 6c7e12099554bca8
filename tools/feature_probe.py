#!/usr/bin/env python3
"""Time the feature composition (nsm_feature_compose, nsm_amd/frames.py
compose_features) with HIP events, and in the same process, interleaved, what it
is measured against:

  * the ATen route: the same channels from ATen ops (slices, subtract, divides,
    `where`, multiply-adds, stack, reflect pad, nan_to_num, the normalisation);
    its result is compared with the kernel's before anything is timed;
  * the copy ceiling: a device-to-device copy of the bytes the pass must move,
    the raw planes the recipe reads plus the Cout planes it writes.

    python tools/feature_probe.py [--shapes 1x11x1080x1920,8x11x512x512] [--reps 20]
                                  [--no-aten]

The six-channel recipe z, z-zf, z/zf, cc/d, n.ne, ce over 11 raw channels, plain
(no pad, scrub or stats) and full (pad to 16, scrub, stats; the census is off in
the C-ABI timing and on in the compose_features one, as FramePipeline runs it). Median of
--reps rounds after warm-up; a round times 10 back-to-back calls of each route
in turn, so the routes see the same machine. Inputs and outputs rotate over
enough buffer sets to exceed the 256 MB Infinity Cache. Prints one line per case
and a final JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
import torch  # noqa: E402

import nsm_amd  # noqa: E402
from nsm_amd._lib import call, ptr, stream  # noqa: E402
from nsm_amd.frames import padded_size  # noqa: E402

EPS = 1e-8
LAYOUT = {"d": 0, "n": 1, "z": 4, "ne": 5, "zf": 8, "ce": 9, "cc": 10}
EXPRS = ["z", "z-zf", "z/zf", "cc/d", "n.ne", "ce"]
INNER = 10


def aten_compose(x, out, floor, pad, mean, div):
    """The recipe's channels of x from ATen ops, into out."""
    d, z, zf, ce, cc = x[:, 0], x[:, 4], x[:, 8], x[:, 9], x[:, 10]
    zero = torch.zeros((), device=x.device)
    c1 = z - zf
    c2 = torch.where(zf.abs() <= floor, zero, z / zf)
    c3 = torch.where(d.abs() <= floor, zero, cc / d)
    c4 = (x[:, 1] * x[:, 5] + x[:, 2] * x[:, 6]) + x[:, 3] * x[:, 7]
    if pad is None:                                       # plain: no pad, scrub or stats
        return torch.stack([z, c1, c2, c3, c4, ce], dim=1, out=out)
    y = torch.stack([z, c1, c2, c3, c4, ce], dim=1)
    if pad is not None and (pad[0] or pad[1]):
        y = torch.nn.functional.pad(y, (0, pad[1], 0, pad[0]), mode="reflect")
    y = torch.nan_to_num(y, nan=0.0, posinf=1.0, neginf=0.0)
    return torch.div(y - mean, div, out=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x11x1080x1920,8x11x512x512")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-aten", action="store_true", help="time the kernel and the copy only")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    recipe = nsm_amd.FeatureRecipe.parse(EXPRS, layout=LAYOUT)
    Cout, used = recipe.out_channels, len(recipe.planes_read())
    g = torch.Generator(device=dev).manual_seed(0)
    mean = torch.randn(Cout, device=dev, generator=g)
    std = torch.rand(Cout, device=dev, generator=g) + 0.5
    rec = {"lib": os.path.basename(nsm_amd.LIB_PATH), "recipe": EXPRS, "raw_planes_read": used}
    for shape in args.shapes.split(","):
        B, Cin, H, W = (int(v) for v in shape.split("x"))
        for full in (False, True):
            Hp, Wp = padded_size(H, W, 16) if full else (H, W)
            nbytes = 4 * B * (used * H * W + Cout * Hp * Wp)
            sets = max(2, -(-(512 << 20) // (4 * B * Cin * H * W)))
            xs = []
            for _ in range(sets):
                x = torch.randn((B, Cin, H, W), device=dev, generator=g)
                x.view(-1)[torch.randint(0, x.numel(), (64,), device=dev, generator=g)] = float("nan")
                x.view(-1)[torch.randint(0, x.numel(), (64,), device=dev, generator=g)] = float("inf")
                xs.append(x)
            outs = [torch.empty((B, Cout, Hp, Wp), device=dev) for _ in range(sets)]
            half = nbytes // 2
            srcs = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(sets)]
            dsts = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(sets)]
            rep = torch.zeros((B, 6), dtype=torch.int32, device=dev) if full else None
            m, s = (mean, std) if full else (None, None)
            am = mean.view(1, -1, 1, 1) if full else None
            adiv = (std + EPS).view(1, -1, 1, 1) if full else None
            pad = (Hp - H, Wp - W) if full else None

            def k_kernel(t):
                call("nsm_feature_compose", ptr(xs[t % sets]), B, Cin, H, W, Hp, Wp, recipe._ctable,
                     Cout, recipe.ratio_floor, ptr(m), ptr(s), EPS, int(full), -1, None,
                     ptr(outs[t % sets]), None, None, stream())

            def k_call(t):
                nsm_amd.compose_features(xs[t % sets], recipe, pad_multiple=16 if full else None,
                                         scrub=full, stats=(mean, std) if full else None,
                                         out=outs[t % sets], report=rep)

            def k_aten(t):
                aten_compose(xs[t % sets], outs[t % sets], recipe.ratio_floor, pad, am, adiv)

            def k_copy(t):
                dsts[t % sets].copy_(srcs[t % sets])

            # the two routes agree (NaNs where the other has them) before anything is timed
            a = nsm_amd.compose_features(xs[0], recipe, pad_multiple=16 if full else None,
                                         scrub=full, stats=(mean, std) if full else None)
            b = aten_compose(xs[0], torch.empty_like(a), recipe.ratio_floor, pad, am, adiv)
            assert torch.equal(torch.isnan(a), torch.isnan(b))
            fin = torch.isfinite(a) & torch.isfinite(b)
            diff = float((a[fin] - b[fin]).abs().max().item())
            assert torch.equal(a[fin], b[fin]) or diff <= 1e-5 * float(b[fin].abs().max().item()), diff

            routes = {"kernel": k_kernel, "call": k_call, "copy": k_copy}
            if not args.no_aten:
                routes["aten"] = k_aten
            times = {k: [] for k in routes}
            t = 0
            for rnd in range(args.reps + 3):                      # 3 warm-up rounds
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
            r = {"bytes": nbytes, "sets": sets, "out": [B, Cout, Hp, Wp],
                 "max_abs_diff_vs_aten": diff}
            for name, ts in times.items():
                ts.sort()
                r[name + "_ms"] = round(ts[len(ts) // 2], 4)
                r[name + "_ms_range"] = [round(ts[0], 4), round(ts[-1], 4)]
            r["kernel_TB_per_s"] = round(nbytes / (r["kernel_ms"] * 1e-3) / 1e12, 2)
            r["copy_over_kernel"] = round(r["copy_ms"] / r["kernel_ms"], 2)
            if "aten_ms" in r:
                r["speedup_vs_aten"] = round(r["aten_ms"] / r["kernel_ms"], 1)
            key = f"{shape}{'-full' if full else '-plain'}"
            rec[key] = r
            print(f"{key}: kernel {r['kernel_ms']:.4f} ms = {r['kernel_TB_per_s']} TB/s of "
                  f"{nbytes / 1e6:.1f} MB (compose_features {r['call_ms']:.4f} ms); ATen "
                  f"{r.get('aten_ms', float('nan')):.4f} ms ({r.get('speedup_vs_aten', 'n/a')}x); D2D "
                  f"copy of the same bytes {r['copy_ms']:.4f} ms (copy / kernel "
                  f"{r['copy_over_kernel']})", flush=True)
            del xs, outs, srcs, dsts
            torch.cuda.empty_cache()
    print(json.dumps({"feature_probe": rec}))


if __name__ == "__main__":
    main()
