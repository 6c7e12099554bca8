#!/usr/bin/env python3
"""Time the differentiable VGG19 perceptual loss (MultiLayerVGGLoss(
differentiable=True)) with HIP events: forward and backward separately, and
each element-wise pass of the backward chain against the bytes it moves
(counted from shapes) and the HBM rate.

    python tools/vgg_grad_time.py [--batch 8] [--res 512] [--seconds 1.0]

Random (He) weights: the work does not depend on their values. Prints one line
per pass and a final JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
import torch  # noqa: E402

from nsm_amd import MultiLayerVGGLoss, ops  # noqa: E402

HBM_MEASURED = 6.29e12   # float4 copy on the MI355X (8.0 TB/s spec)


def window(fn, seconds, warmup=3):
    """Mean ms of each timed section of fn() (a list of (start, end) event
    pairs per call) over a window of at least `seconds` of device time."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    sums, n, total = None, 0, 0.0
    while total < seconds * 1e3 or n < 5:
        pairs = fn()
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in pairs]
        sums = ms if sums is None else [s + m for s, m in zip(sums, ms)]
        total += sum(ms)
        n += 1
    return [s / n for s in sums], n


def ev():
    return torch.cuda.Event(enable_timing=True)


def median_ms(fn, n=20):
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
    return sorted(ts)[n // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--seconds", type=float, default=1.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H = args.batch, args.res
    g = torch.Generator(device=dev).manual_seed(0)
    o = torch.sigmoid(torch.randn(B, 1, H, H, device=dev, generator=g)).requires_grad_(True)
    t = torch.rand(B, 1, H, H, device=dev, generator=g)

    plain = MultiLayerVGGLoss(dev)
    diff = MultiLayerVGGLoss(dev, differentiable=True)

    def step_plain():
        a, b = ev(), ev()
        a.record()
        plain(o, t)
        b.record()
        return [(a, b)]

    def step_diff():
        a, b, c = ev(), ev(), ev()
        a.record()
        loss = diff(o, t)
        b.record()
        loss.backward()
        c.record()
        o.grad = None
        return [(a, b), (b, c)]

    (p_ms,), n_p = window(step_plain, args.seconds)
    (f_ms, b_ms), n_d = window(step_diff, args.seconds)
    print(f"B={B} 1x{H}x{H}: default forward {p_ms:.3f} ms ({n_p} calls); differentiable forward "
          f"{f_ms:.3f} ms, backward {b_ms:.3f} ms ({n_d} calls)", flush=True)

    # the element-wise passes of the chain, one by one, at the chain's shapes
    gs = torch.ones((), device=dev)
    rows, passes, tot_bytes, tot_ms = [], [], 0, 0.0
    h, taps = H, set(diff.feature_layers)
    for idx, m in enumerate(diff.features):
        if idx > max(taps):
            break
        if isinstance(m, torch.nn.Conv2d):
            rows.append({"idx": idx, "C": m.out_channels, "h": h, "pool": False,
                         "tap": idx in taps})
        elif isinstance(m, torch.nn.MaxPool2d):
            rows[-1]["pool"] = True
            h //= 2
    last = rows[-1]["idx"]
    for r in reversed(rows):
        C, h, n = r["C"], r["h"], B * r["h"] * r["h"] * r["C"]
        y = torch.randn(B * h * h, C, device=dev)
        tt = torch.randn(B * h * h, C, device=dev) if r["tap"] else None
        if r["pool"]:
            gp = torch.randn(B * (h // 2) * (h // 2), C, device=dev)
            ms = median_ms(lambda: ops.maxpool2_bwd(gp, y, tt, B, h, h, 1e-3, gs))
            by, what = 4 * (n // 4 + n + n + (n if r["tap"] else 0)), "maxpool2_bwd"
        elif r["idx"] == last:
            ms = median_ms(lambda: ops.vgg_tap_relu_bwd(None, y, tt, 1e-3, gs))
            by, what = 4 * 3 * n, "tap (no incoming g)"
        else:
            gg = torch.randn(B * h * h, C, device=dev)
            ms = median_ms(lambda: ops.vgg_tap_relu_bwd(gg, y, tt, 1e-3, gs, relu=True))
            by, what = 4 * (3 * n + (n if r["tap"] else 0)), "tap_relu_bwd"
        what += "+tap" if r["tap"] and r["idx"] != last else ""
        passes.append({"features": r["idx"], "pass": what, "MB": round(by / 1e6, 1),
                       "us": round(ms * 1e3, 1), "TB_per_s": round(by / ms / 1e9, 2)})
        tot_bytes += by
        tot_ms += ms
        del y, tt
    g32 = torch.randn(B * H * H, 32, device=dev)
    grad = torch.empty(B, 1, H, H, device=dev)
    ms = median_ms(lambda: ops.vgg_prep_bwd(g32, o.detach(), diff.denom, grad))
    by = B * H * H * (128 + 4 + 4)   # a 128-B line per pixel is fetched for 12 useful bytes
    passes.append({"features": "prep", "pass": "vgg_prep_bwd", "MB": round(by / 1e6, 1),
                   "us": round(ms * 1e3, 1), "TB_per_s": round(by / ms / 1e9, 2)})
    tot_bytes += by
    tot_ms += ms
    for p in passes:
        print(p, flush=True)
    rec = {"batch": B, "res": H, "default_forward_ms": round(p_ms, 3),
           "differentiable_forward_ms": round(f_ms, 3), "backward_ms": round(b_ms, 3),
           "elementwise_MB": round(tot_bytes / 1e6, 1), "elementwise_ms": round(tot_ms, 3),
           "elementwise_TB_per_s": round(tot_bytes / tot_ms / 1e9, 2),
           "elementwise_ms_at_hbm_rate": round(tot_bytes / HBM_MEASURED * 1e3, 3),
           "hbm_rate_TB_per_s": HBM_MEASURED / 1e12, "passes": passes}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
