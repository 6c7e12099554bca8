#!/usr/bin/env python3
"""Time the training-patch gather (nsm_patch_gather, nsm_amd/patches.py) with HIP
events, and in the same process what it is measured against:

  * the ATen route: the same batch from ATen ops (per-sample slice, flip, stack,
    the normalisation), driven by the same draws; its result is compared with
    the kernel's before anything is timed;
  * the copy ceiling: a device-to-device copy of the bytes the pass must move,
    the patch bytes read plus the patch bytes written (counted from shapes).

    python tools/patch_probe.py [--frames 64] [--frame 7x1024x2048] [--patch 512x512]
                                [--batches 8,64] [--reps 20]

Median of --reps after warm-up, 10 back-to-back calls per event pair. The pool
(64 frames of 7 x 1024 x 2048 plus labels: 4.3 GB) is far larger than the 256 MB
Infinity Cache and every call draws new frames and offsets (order="random"); the
outputs and the copy's buffers rotate over enough sets to exceed 256 MB too.
Prints one line per batch size and a final JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
import torch  # noqa: E402

import nsm_amd  # noqa: E402
from nsm_amd._lib import call, ptr, stream  # noqa: E402

EPS = 1e-8


def median_ms(fn, n, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[n // 2]


def aten_batch(s, draws, hs, out):
    """The batch of `draws` (a host list) from ATen ops, into out = (x, y)."""
    ph, pw = s.patch
    xs, ys = [], []
    for fr, oy, ox, hf, vf, e, _, _ in draws:
        v = s.inputs[fr, :, oy:oy + ph, ox:ox + pw]
        y = s.labels[fr, e:e + 1, oy:oy + ph, ox:ox + pw]
        if hf:
            v, y = v.flip(2) * hs, y.flip(2)
        xs.append(v)
        ys.append(y)
    torch.stack(ys, out=out[1])
    x = torch.stack(xs)
    torch.div(x - s.means.view(1, -1, 1, 1), s.stds.view(1, -1, 1, 1) + EPS, out=out[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--frame", default="7x1024x2048", help="a frame, CxHxW")
    ap.add_argument("--patch", default="512x512")
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    C, H, W = (int(v) for v in args.frame.split("x"))
    ph, pw = (int(v) for v in args.patch.split("x"))
    N = args.frames
    g = torch.Generator(device=dev).manual_seed(0)
    inputs = torch.empty((N, C, H, W), device=dev)
    labels = torch.empty((N, 1, H, W), device=dev)
    for i in range(N):
        inputs[i] = torch.randn((C, H, W), device=dev, generator=g)
        labels[i] = torch.rand((1, H, W), device=dev, generator=g)
    means = torch.randn(C, device=dev, generator=g)
    stds = torch.rand(C, device=dev, generator=g) + 0.5
    hsign = torch.ones(C)
    hsign[1::3] = -1.0
    hs = hsign.to(dev).view(C, 1, 1)
    rec = {"pool": [N, C, H, W], "patch": [ph, pw], "lib": os.path.basename(nsm_amd.LIB_PATH)}
    for B in (int(v) for v in args.batches.split(",")):
        s = nsm_amd.PatchSampler(inputs, labels, patch=(ph, pw), batch=B, stats=(means, stds),
                                 seed=1, order="random", hflip=True, hflip_sign=hsign,
                                 record_draws=True)
        nbytes = 2 * 4 * B * (C + 1) * ph * pw          # patch bytes read + patch bytes written
        sets = max(2, -(-(512 << 20) // (nbytes // 2)))
        outs = [(torch.empty((B, C, ph, pw), device=dev), torch.empty((B, 1, ph, pw), device=dev))
                for _ in range(sets)]
        srcs = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(sets)]
        dsts = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(sets)]

        # the two routes agree: labels exactly, patches up to the division's last bit
        x, y = s.next(out=outs[0])
        ax, ay = aten_batch(s, s.last_draws.tolist(), hs, outs[1])
        assert s.last_draws.tolist() == s.draws(0).tolist()
        assert torch.equal(y, ay)
        diff = float((x - ax).abs().max().item())
        assert diff <= 1e-5 * float(ax.abs().max().item()), diff
        host_draws = [s.draws(t).tolist() for t in range(16)]
        state = {"t": 0}

        def k_gather():
            for _ in range(10):
                t = state["t"] = state["t"] + 1
                o = outs[t % sets]
                call("nsm_patch_gather", ptr(inputs), ptr(labels), N, C, 1, H, W, B, ph, pw,
                     ptr(s.means), ptr(s.stds), EPS, ptr(s.hflip_sign), None, -1, None, 1, 1, 1, 0,
                     0, N, 0, 1, None, t, None, ptr(o[0]), ptr(o[1]), None, stream())

        def k_call():
            for _ in range(10):
                t = state["t"] = state["t"] + 1
                s.next(out=outs[t % sets])

        def k_aten():
            for _ in range(10):
                t = state["t"] = state["t"] + 1
                aten_batch(s, host_draws[t % 16], hs, outs[t % sets])

        def k_copy():
            for _ in range(10):
                t = state["t"] = state["t"] + 1
                dsts[t % sets].copy_(srcs[t % sets])

        r = {"bytes": nbytes, "sets": sets, "max_abs_diff_vs_aten": diff}
        r["copy_ms"] = [round(median_ms(k_copy, args.reps) / 10, 4)]
        r["gather_ms"] = round(median_ms(k_gather, args.reps) / 10, 4)
        r["call_ms"] = round(median_ms(k_call, args.reps) / 10, 4)
        r["aten_ms"] = round(median_ms(k_aten, args.reps) / 10, 4)
        r["copy_ms"].append(round(median_ms(k_copy, args.reps) / 10, 4))
        r["gather_TB_per_s"] = round(nbytes / (r["gather_ms"] * 1e-3) / 1e12, 2)
        r["speedup_vs_aten"] = round(r["aten_ms"] / r["gather_ms"], 1)
        r["copy_over_gather"] = round(min(r["copy_ms"]) / r["gather_ms"], 2)
        rec[f"B{B}"] = r
        print(f"B={B} {C}x{ph}x{pw} from {N} frames of {C}x{H}x{W}: gather {r['gather_ms']:.4f} ms = "
              f"{r['gather_TB_per_s']} TB/s of {nbytes / 1e6:.1f} MB (sampler.next {r['call_ms']:.4f} "
              f"ms); ATen {r['aten_ms']:.4f} ms ({r['speedup_vs_aten']}x); D2D copy of the same bytes "
              f"{r['copy_ms']} ms (copy / gather {r['copy_over_gather']})", flush=True)
        del s, outs, srcs, dsts
        torch.cuda.empty_cache()
    print(json.dumps({"patch_probe": rec}))


if __name__ == "__main__":
    main()
