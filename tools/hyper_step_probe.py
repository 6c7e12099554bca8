#!/usr/bin/env python3
"""What a learning-rate (or max_norm) change costs GraphedTrainStep, and what
reading the two values from the device costs a replay: the argument path
(default) against `device_hyper=True`, in one process, on 7x512x512 inputs.

    python tools/hyper_step_probe.py [--dtype f32] [--batch 8] [--steps 20] [--windows 3]
                                     [--changes 3] [--reps 50]

(a) the change itself, --changes times per path, alternating:
      * argument path: the call after `lr` moved re-captures the whole step;
        timed on the host (perf_counter around the call and a device
        synchronise, the capture being host work), with a call that only replays
        beside it;
      * device path: the same call uploads the pair (`sync_hyper`: one
        nsm_hyper_set launch) and replays; timed the same way. The launch alone
        is the median of --reps HIP-event pairs around one nsm_hyper_set each,
        and of perf_counter around the host side of the call.
(b) --windows windows of --steps replays of either path, in the order a b a b
    ..., each between two HIP events after warm-up replays: ms per step and
    frames/s, with each path's window-to-window spread.
Both models start from the same weights and see the same batch. The probe reads
nothing outside the repository and prints one JSON record at the end."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
import torch  # noqa: E402

import nsm_amd  # noqa: E402

C, H = 7, 512
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def ev():
    return torch.cuda.Event(enable_timing=True)


def window_ms(fn, n, warmup=3):
    """ms per call over one window of n calls (events around the window)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = ev(), ev()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def wall_ms(fn):
    """Host ms of one call, the device drained before and after."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def build(dev, dtype, device_hyper, x, y):
    torch.manual_seed(0)
    m = nsm_amd.Unet(in_ch=C, dropout_rate=0.2).to(dev).train()
    if dtype != torch.float32:
        m.set_compute_dtype(dtype)
    opt = nsm_amd.FlatAdamW(m.parameters(), lr=7e-4, weight_decay=1e-3, max_grad_norm=1.0,
                            sanitize=True, device_hyper=device_hyper)
    crit = nsm_amd.CustomLoss(dev, 0.9, vgg_weights=False)
    return opt, nsm_amd.GraphedTrainStep(m, crit, opt, x, y, warmup=2)


def set_launch_times(opt, reps):
    """The nsm_hyper_set launch alone: device ms (events) and host ms per call."""
    dev_ms, host_ms = [], []
    for i in range(reps + 3):
        opt.param_groups[0]["lr"] = 7e-4 * (1.0 + 1e-3 * (i + 1))    # always another pair
        a, b = ev(), ev()
        a.record()
        t = time.perf_counter()
        opt.sync_hyper()
        h = (time.perf_counter() - t) * 1e3
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            dev_ms.append(a.elapsed_time(b))
            host_ms.append(h)
    opt.param_groups[0]["lr"] = 7e-4
    opt.sync_hyper()
    return sorted(dev_ms)[reps // 2], sorted(host_ms)[reps // 2]


def spread_pct(v):
    return round(100 * (max(v) - min(v)) / sorted(v)[len(v) // 2], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f32", choices=list(DTYPES))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--changes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hyper_step_probe: needs a ROCm GPU (timings are device events)")
    dev = torch.device("cuda:0")
    B = args.batch
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, C, H, H, device=dev, generator=g)
    y = torch.randint(0, 256, (B, 1, H, H), device=dev, generator=g).float() / 255.0
    oa, a = build(dev, DTYPES[args.dtype], False, x, y)
    ob, b = build(dev, DTYPES[args.dtype], True, x, y)
    r = {"a_change_call_ms": [], "a_replay_call_ms": [], "b_change_call_ms": [],
         "b_replay_call_ms": [], "a_replay_ms": [], "b_replay_ms": []}
    for _ in range(3):
        a()
        b()
    # (a) the change
    for i in range(args.changes):
        lr = 7e-4 / (2.0 + i)
        for opt, step, k in ((oa, a, "a"), (ob, b, "b")):
            r[k + "_replay_call_ms"].append(wall_ms(step))
            opt.param_groups[0]["lr"] = lr
            r[k + "_change_call_ms"].append(wall_ms(step))
    r["captures"] = {"a": a.captures, "b": b.captures}
    d, h = set_launch_times(ob, args.reps)
    r["hyper_set_device_ms"], r["hyper_set_host_ms"] = round(d, 4), round(h, 4)
    # (b) the replay, a b a b ...
    for _ in range(args.windows):
        r["a_replay_ms"].append(window_ms(a, args.steps))
        r["b_replay_ms"].append(window_ms(b, args.steps))
    r = {k: ([round(v, 3) for v in vs] if isinstance(vs, list) else vs) for k, vs in r.items()}
    for k in ("a", "b"):
        w = r[k + "_replay_ms"]
        r[k + "_spread_pct"] = spread_pct(w)
        r[k + "_frames_per_s"] = [round(B / v * 1e3, 1) for v in w]
    ma, mb = sorted(r["a_replay_ms"])[args.windows // 2], sorted(r["b_replay_ms"])[args.windows // 2]
    r["b_over_a_median"] = round(mb / ma, 4)
    print(f"{args.dtype} B={B}: lr change, argument path (re-capture) {r['a_change_call_ms']} ms "
          f"per call vs plain replay call {r['a_replay_call_ms']}; device path (upload + replay) "
          f"{r['b_change_call_ms']} vs {r['b_replay_call_ms']}; captures {r['captures']}; "
          f"nsm_hyper_set {r['hyper_set_device_ms']} ms on the device, {r['hyper_set_host_ms']} ms "
          f"on the host; replay windows a {r['a_replay_ms']} (spread {r['a_spread_pct']} %) "
          f"b {r['b_replay_ms']} (spread {r['b_spread_pct']} %), b/a {r['b_over_a_median']}",
          flush=True)
    rec = {"lib": os.path.basename(nsm_amd.LIB_PATH), "dtype": args.dtype, "batch": B,
           "input": [C, H, H], "steps": args.steps, "reps": args.reps}
    rec.update(r)
    print(json.dumps({"hyper_step_probe": rec}))


if __name__ == "__main__":
    main()
