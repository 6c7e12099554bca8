#!/usr/bin/env python3
"""Time the fused SSIM term (nsm_ssim_fwd/bwd) with HIP events at 8x1x512x512
and 1x1x1080x1920, and in the same process the fused detail terms
(nsm_detail_loss_fwd/bwd) and the ATen restatement of the same SSIM (an
F.conv2d chain plus autograd: what a user would otherwise run) on the same
device: forward and forward+backward, median of 20 after warm-up.

    python tools/ssim_probe.py [--shapes 8x512x512 1x1080x1920] [--reps 20]

Bytes are counted from shapes (N = B*H*W pixels, M = B*(H-10)*(W-10) windows):
the forward reads o and t (8N) and writes three coefficient planes (12M); the
backward reads o, t and the planes and writes the gradient (12N + 12M). Also
prints the loss of both paths and the rel-L2 distance of their gradients (both
float32) at the timed shapes. One line per shape and a final JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import nsm_amd  # noqa: E402


def ev():
    return torch.cuda.Event(enable_timing=True)


def median_ms(fn, n, warmup=3):
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


class AtenSsim:
    """1 - pytorch_msssim.ssim (defaults, data_range 1) from ATen ops."""

    def __init__(self, dev):
        c = torch.arange(11, dtype=torch.float32) - 5
        g = torch.exp(-(c ** 2) / (2 * 1.5 ** 2))
        g = (g / g.sum()).to(dev)
        self.gv, self.gh = g.view(1, 1, 11, 1), g.view(1, 1, 1, 11)

    def blur(self, x):
        return F.conv2d(F.conv2d(x, self.gv), self.gh)

    def __call__(self, o, t):
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        a, b = self.blur(o), self.blur(t)
        p, q, r = self.blur(o * o), self.blur(t * t), self.blur(o * t)
        cs = (2 * (r - a * b) + c2) / ((p - a * a) + (q - b * b) + c2)
        s = (2 * a * b + c1) / (a * a + b * b + c1) * cs
        return 1 - s.flatten(1).mean(1).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["8x512x512", "1x1080x1920"])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    aten = AtenSsim(dev)
    recs = []
    for spec in args.shapes:
        B, H, W = (int(v) for v in spec.split("x"))
        g = torch.Generator(device=dev).manual_seed(0)
        o = torch.sigmoid(2 * torch.randn(B, 1, H, W, device=dev, generator=g)).requires_grad_(True)
        t = torch.rand(B, 1, H, W, device=dev, generator=g)
        seed = torch.ones((), device=dev)

        def step(fwd):
            def run():
                fwd().backward(seed)
                o.grad = None
            return run

        paths = {
            "ssim": lambda: nsm_amd.ssim_loss(o, t),
            "detail": lambda: nsm_amd.detail_loss(o, t, 0.1, 0.1, 0.1),
            "aten": lambda: aten(o, t),
        }
        grads = {}
        for k in ("ssim", "aten"):
            paths[k]().backward(seed)
            grads[k], o.grad = o.grad, None
        grad_rel = ((grads["ssim"] - grads["aten"]).norm() / grads["aten"].norm()).item()
        n, m = B * H * W, B * (H - 10) * (W - 10)
        rec = {"shape": [B, 1, H, W], "fused_loss": paths["ssim"]().item(),
               "aten_loss": paths["aten"]().item(),
               "grad_rel_l2_vs_aten": float(f"{grad_rel:.3g}"),
               "metric_ms": round(median_ms(lambda: nsm_amd.ssim(o, t), args.reps), 4),
               "fwd_MB": round((8 * n + 12 * m) / 1e6, 1),
               "bwd_MB": round((12 * n + 12 * m) / 1e6, 1)}
        for k, fwd in paths.items():
            rec[k + "_fwd_ms"] = round(median_ms(fwd, args.reps), 4)
            rec[k + "_fwd_bwd_ms"] = round(median_ms(step(fwd), args.reps), 4)
        # the kernels alone: 10 back-to-back launches per event pair, so the
        # host's launch path is hidden behind the device's work
        from nsm_amd.losses import _ssim_bwd, _ssim_fwd
        od, grad = o.detach(), torch.empty_like(t)
        _, coef = _ssim_fwd(od, t, 1.0, 1.0, keep=True)
        rec["kernel_fwd_ms"] = round(median_ms(
            lambda: [_ssim_fwd(od, t, 1.0, 1.0, keep=True) for _ in range(10)], args.reps) / 10, 4)
        rec["kernel_bwd_ms"] = round(median_ms(
            lambda: [_ssim_bwd(od, t, coef, 1.0, seed, grad, False) for _ in range(10)],
            args.reps) / 10, 4)
        rec["speedup_fwd_bwd"] = round(rec["aten_fwd_bwd_ms"] / rec["ssim_fwd_bwd_ms"], 2)
        print(f"{spec}: ssim fwd {rec['ssim_fwd_ms']:.3f} ms, fwd+bwd {rec['ssim_fwd_bwd_ms']:.3f} "
              f"ms (metric only {rec['metric_ms']:.3f}); detail fwd {rec['detail_fwd_ms']:.3f}, "
              f"fwd+bwd {rec['detail_fwd_bwd_ms']:.3f}; ATen fwd {rec['aten_fwd_ms']:.3f}, fwd+bwd "
              f"{rec['aten_fwd_bwd_ms']:.3f} ({rec['speedup_fwd_bwd']}x); kernels alone fwd "
              f"{rec['kernel_fwd_ms']:.4f}, bwd {rec['kernel_bwd_ms']:.4f}; gradient against ATen rel-L2 "
              f"{rec['grad_rel_l2_vs_aten']:.1e}", flush=True)
        recs.append(rec)
        del o, t
    print(json.dumps({"ssim_probe": recs}))


if __name__ == "__main__":
    main()
