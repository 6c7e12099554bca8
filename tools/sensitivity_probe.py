#!/usr/bin/env python3
"""Time nsm_amd.feature_sensitivity (the paper's Eq. 1 on one captured eval
forward) against the loop a user would otherwise write, on the same device, in
interleaved runs: 1x7x512x512, R = 4, all 7 channels, fp32 and bf16.

    python tools/sensitivity_probe.py [--res 512] [--repeats 4] [--chunk 8] [--rounds 7]

The hand-written loop: per channel and repeat one `torch.randn_like(x)`, the add
on one plane, an eager eval `model(x)` and `.abs().mean().item()`. The library
path is timed twice: a held FeatureSensitivity (the capture paid once, outside
the timing: update() plus reading the result) and the one-shot call (capture
included). Times are wall-clock milliseconds around a device synchronisation,
median over the rounds. The two new kernels are timed on their own with HIP
events (median of 20) at the chunk's shape. Prints one line per mode and a final
JSON record."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nsm_amd  # noqa: E402
from nsm_amd.sensitivity import sens_reduce, sens_variants  # noqa: E402
from oracle.weights import make_state, synthetic_batch  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn, n=20, warmup=3):
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


def hand_loop(model, x, sigma, repeats, factor):
    """What the issue's user writes today."""
    C = x.shape[1]
    was = model.training
    model.eval()
    S = []
    with torch.no_grad():
        base = model(x).clone()
        for i in range(C):
            s = factor * sigma[i]
            tot = 0.0
            for _ in range(repeats):
                noise = torch.randn_like(x)
                xp = x.clone()
                xp[:, i] = x[:, i] + noise[:, i] * s
                tot += (model(xp) - base).abs().mean().item()
            S.append(tot / repeats / s)
    model.train(was)
    return S


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    C, H, R, factor = 7, args.res, args.repeats, 0.1
    model = nsm_amd.Unet(in_ch=C, dropout_rate=0.0)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_state(C, 42).items()})
    model = model.to(dev).eval()
    x = torch.from_numpy(synthetic_batch(1, C, H, H)[0]).to(dev)
    sigma = [1.0] * C
    recs = []
    for name, dtype in (("fp32", None), ("bf16", torch.bfloat16)):
        model.set_compute_dtype(dtype)
        held = nsm_amd.FeatureSensitivity(model, sigma, repeats=R, factor=factor,
                                          chunk=args.chunk, seed=1)

        def held_run():
            held.reset()
            held.update(x)
            return held.compute().absolute.cpu()

        def one_shot():
            return nsm_amd.feature_sensitivity(model, x, sigma, repeats=R, factor=factor,
                                               chunk=args.chunk, seed=1).absolute.cpu()

        def hand():
            return hand_loop(model, x, sigma, R, factor)

        for fn in (held_run, one_shot, hand):   # warm-up: capture, allocator, weight layouts
            fn()
        t = {"held": [], "one_shot": [], "hand": []}
        for _ in range(args.rounds):            # interleaved
            t["hand"].append(wall_ms(hand))
            t["held"].append(wall_ms(held_run))
            t["one_shot"].append(wall_ms(one_shot))
        rec = {"mode": name, "res": H, "channels": C, "repeats": R, "chunk": args.chunk,
               "hand_loop_ms": round(median(t["hand"]), 2),
               "held_ms": round(median(t["held"]), 2),
               "one_shot_ms": round(median(t["one_shot"]), 2),
               "absolute_held": [round(v, 6) for v in held_run().tolist()],
               "absolute_hand": [round(v, 6) for v in hand()]}
        print(f"{name} 1x{C}x{H}x{H} R={R}: hand-written loop {rec['hand_loop_ms']} ms, held "
              f"FeatureSensitivity {rec['held_ms']} ms, one-shot call (with capture) "
              f"{rec['one_shot_ms']} ms", flush=True)
        recs.append(rec)
    model.set_compute_dtype(None)

    # the two kernels at the chunk's shape
    n = args.chunk
    sig = torch.ones(C, device=dev)
    ch = torch.arange(C, dtype=torch.int32, device=dev)
    slots = torch.empty((n, C, H, H), device=dev)
    outs = torch.rand((n, H * H), device=dev)
    base = torch.rand((1, H * H), device=dev)
    psum = torch.empty((C * R, nsm_amd.lib.nsm_sens_blocks(H * H), 2), device=dev)
    kern = {
        "sens_variants_ms": round(event_ms(
            lambda: sens_variants(x, sig, ch, R, factor, 1, n, slots, None, 1)), 4),
        "sens_reduce_ms": round(event_ms(
            lambda: sens_reduce(outs, base, 1, 1, C, R, psum)), 4),
        "variants_MB": round(2 * n * C * H * H * 4 / 1e6, 1),
        "reduce_MB": round(2 * n * H * H * 4 / 1e6, 1),
    }
    print(f"kernels at chunk {n}: sens_variants {kern['sens_variants_ms']} ms "
          f"({kern['variants_MB']} MB), sens_reduce {kern['sens_reduce_ms']} ms "
          f"({kern['reduce_MB']} MB)", flush=True)
    print(json.dumps({"sensitivity_probe": recs, "kernels": kern}))


if __name__ == "__main__":
    main()
