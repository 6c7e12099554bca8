#!/usr/bin/env python3
"""Time the fused detail terms of CustomLoss (nsm_detail_loss_fwd/bwd) with HIP
events against the same formulas composed from ATen ops on the same device
(the reference's own code path, customLoss.py:139-185, with its filter kernels
built once): forward and forward+backward, median of 20 after warm-up, at
B=8 and B=64, 1x512x512.

    python tools/detail_loss_time.py [--batches 8 64] [--res 512] [--count-launches]

Bytes are counted from shapes: the forward reads o and t (2N floats), the
backward reads them again and writes the gradient (3N). --count-launches also
counts the device kernels of one forward+backward of each path with
torch.profiler. Prints one line per size and a final JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import nsm_amd  # noqa: E402

DW, GW = 0.1, 0.1


def ev():
    return torch.cuda.Event(enable_timing=True)


def median_ms(fn, n=20, warmup=3):
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
    return sorted(ts)[n // 2]


class AtenDetail:
    """detail_weight*(HF + PEN) + gradient_weight*SOB from ATen ops."""

    def __init__(self, dev):
        x = (torch.arange(5) - 2).expand(5, -1)
        k = torch.exp(-(x.pow(2) + x.t().pow(2)) / 2.0)
        self.g = (k / k.sum()).view(1, 1, 5, 5).to(dev)
        self.kx = torch.tensor([[-1., 0, 1], [-2, 0, 2], [-1, 0, 1]], device=dev).view(1, 1, 3, 3)
        self.ky = torch.tensor([[-1., -2, -1], [0, 0, 0], [1, 2, 1]], device=dev).view(1, 1, 3, 3)

    def hf(self, x):
        return x - F.conv2d(x, self.g, padding=2)

    def mag(self, x):
        gx, gy = F.conv2d(x, self.kx, padding=1), F.conv2d(x, self.ky, padding=1)
        return torch.sqrt(gx ** 2 + gy ** 2 + 1e-6)

    def __call__(self, o, t):
        high = F.l1_loss(self.hf(o), self.hf(t))
        m = ((t > 0.1) & (t < 0.9)).float()
        pen = F.l1_loss(o * m, t * m, reduction="sum") / (m.sum() + 1e-8)
        with torch.no_grad():
            tm = self.mag(t)
        sob = F.l1_loss(self.mag(o), tm)
        return DW * (high + pen) + GW * sob


def kernel_count(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type.name == "CUDA")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--count-launches", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    aten = AtenDetail(dev)
    recs = []
    for B in args.batches:
        H = args.res
        g = torch.Generator(device=dev).manual_seed(0)
        o = torch.sigmoid(2 * torch.randn(B, 1, H, H, device=dev, generator=g)).requires_grad_(True)
        t = torch.rand(B, 1, H, H, device=dev, generator=g)
        seed = torch.ones((), device=dev)

        def fused_fwd():
            return nsm_amd.detail_loss(o, t, DW, DW, GW)

        def fused_step():
            fused_fwd().backward(seed)
            o.grad = None

        def aten_fwd():
            return aten(o, t)

        def aten_step():
            aten_fwd().backward(seed)
            o.grad = None

        lf, la = fused_fwd().item(), aten_fwd().item()
        n = B * H * H
        rec = {"batch": B, "res": H,
               "fused_fwd_ms": round(median_ms(fused_fwd), 4),
               "fused_fwd_bwd_ms": round(median_ms(fused_step), 4),
               "aten_fwd_ms": round(median_ms(aten_fwd), 4),
               "aten_fwd_bwd_ms": round(median_ms(aten_step), 4),
               "fwd_MB": round(2 * n * 4 / 1e6, 1), "bwd_MB": round(3 * n * 4 / 1e6, 1),
               "fused_loss": lf, "aten_loss": la}
        rec["fused_bwd_ms"] = round(rec["fused_fwd_bwd_ms"] - rec["fused_fwd_ms"], 4)
        rec["fwd_TB_per_s"] = round(rec["fwd_MB"] / rec["fused_fwd_ms"] / 1e3, 2)
        rec["bwd_TB_per_s"] = round(rec["bwd_MB"] / max(rec["fused_bwd_ms"], 1e-6) / 1e3, 2)
        rec["speedup_fwd_bwd"] = round(rec["aten_fwd_bwd_ms"] / rec["fused_fwd_bwd_ms"], 2)
        if args.count_launches:
            rec["fused_kernels"] = kernel_count(fused_step)
            rec["aten_kernels"] = kernel_count(aten_step)
        print(f"B={B} 1x{H}x{H}: fused fwd {rec['fused_fwd_ms']:.3f} ms, fwd+bwd "
              f"{rec['fused_fwd_bwd_ms']:.3f} ms; ATen fwd {rec['aten_fwd_ms']:.3f} ms, fwd+bwd "
              f"{rec['aten_fwd_bwd_ms']:.3f} ms ({rec['speedup_fwd_bwd']}x)", flush=True)
        recs.append(rec)
        del o, t
    print(json.dumps({"detail_loss_time": recs}))


if __name__ == "__main__":
    main()
