#!/usr/bin/env python3
"""Time the temporal-instability metric with motion-vector reprojection
(nsm_temporal_pair / nsm_temporal_finalize) with HIP events at 1x1x1080x1920,
T = 8, with depth and normal rejection, and in the same process the unadjusted
path (nsm_expdiff_mean) and an ATen restatement of the same metric
(F.grid_sample on frame, depth and normals plus elementwise ops: what a user
would otherwise run) on the same device. Median of 20 after warm-up.

    python tools/temporal_probe.py [--shape 1x1x1080x1920] [--frames 8] [--reps 20]
                                   [--mv random|smooth]

Bytes a pair must move are counted from shapes, per pixel: cur 4C, motion
vectors 8, depth 8 (both frames), normals 24 (both frames), the previous
frame's taps 4C (each previous pixel once: neighbouring pixels share taps).
--mv picks the motion field. Prints one line and a final JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import nsm_amd  # noqa: E402
from nsm_amd import temporal as T  # noqa: E402


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


def aten_metric(frames, mvs, depth, normals, alpha, depth_tol, normal_cos):
    """normalize="valid" from ATen ops (float32)."""
    B, C, H, W = frames[0].shape
    dev = frames[0].device
    x = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    y = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
    total = 0
    for t in range(1, len(frames)):
        px, py = x + mvs[t - 1][:, 0], y + mvs[t - 1][:, 1]
        ok = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
        grid = torch.stack([2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1], dim=-1)
        stack = torch.cat([frames[t - 1], depth[t - 1], normals[t - 1]], dim=1)
        s = F.grid_sample(stack, grid, mode="bilinear", padding_mode="border", align_corners=True)
        z = depth[t][:, 0]
        ok &= (z - s[:, C]).abs() <= depth_tol * z.abs()
        ok &= (normals[t] * s[:, C + 1:]).sum(1) >= normal_cos
        e = (torch.exp(alpha * (frames[t] - s[:, :C]).abs()) - 1) * ok.unsqueeze(1)
        total = total + e.sum() / (ok.sum() * C).clamp_min(1)
    return total / (len(frames) - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x1x1080x1920")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mv", choices=("random", "smooth"), default="random",
                    help="random: N(0, 2.5 px) per pixel (no two neighbours agree: the gathers' "
                         "worst case); smooth: a pan of (3.3, -1.7) px plus a slow 1.5 px wave "
                         "(a moving camera)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, C, H, W = (int(v) for v in args.shape.split("x"))
    n = args.frames
    g = torch.Generator(device=dev).manual_seed(0)
    frames = [torch.rand(B, C, H, W, device=dev, generator=g) for _ in range(n)]
    if args.mv == "random":
        mvs = [2.5 * torch.randn(B, 2, H, W, device=dev, generator=g) for _ in range(n - 1)]
    else:
        yy = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
        xx = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
        mvs = [torch.stack([3.3 + 1.5 * torch.sin(xx / 97 + yy / 61 + i).expand(B, H, W),
                            -1.7 + 1.5 * torch.cos(xx / 83 - yy / 71 + i).expand(B, H, W)], dim=1)
               .contiguous() for i in range(n - 1)]
    depth = [1 + torch.rand(B, 1, H, W, device=dev, generator=g) for _ in range(n)]
    normals = [F.normalize(torch.randn(B, 3, H, W, device=dev, generator=g)
                           + torch.tensor([0.0, 0.0, 2.0], device=dev).view(1, 3, 1, 1), dim=1)
               for _ in range(n)]
    kw = dict(depth=depth, normals=normals, depth_tol=0.3, normal_cos=0.2)

    def fused():
        return nsm_amd.measure_temporal_instability(frames, mvs, 5.0, **kw)

    def aten():
        return aten_metric(frames, mvs, depth, normals, 5.0, 0.3, 0.2)

    _, counts = nsm_amd.temporal_instability_terms(frames, mvs, 5.0, **kw)
    pix = B * H * W
    pair_bytes = pix * (4 * C + 8 + 8 + 24 + 4 * C)
    rec = {"shape": [B, C, H, W], "frames": n, "mv": args.mv,
           "lib": os.path.basename(nsm_amd.LIB_PATH), "value": fused().item(),
           "aten_value": aten().item(),
           "surviving_share": round(counts.sum().item() / ((n - 1) * pix * C), 4),
           "pair_MB": round(pair_bytes / 1e6, 1),
           "call_ms": round(median_ms(fused, args.reps), 4),
           "call_position_only_ms": round(median_ms(
               lambda: nsm_amd.measure_temporal_instability(frames, mvs, 5.0), args.reps), 4),
           "unadjusted_ms": round(median_ms(
               lambda: nsm_amd.measure_temporal_instability(frames, alpha=5.0), args.reps), 4),
           "aten_ms": round(median_ms(aten, args.reps), 4)}
    # the kernels alone: 10 back-to-back launches per event pair, so the host's
    # launch path is hidden behind the device's work
    per = T._blocks((B, C, H, W))
    psum = torch.empty((n - 1, B, per), dtype=torch.float32, device=dev)
    pcnt = torch.empty((n - 1, B, per), dtype=torch.int32, device=dev)

    def pairs(reject):
        def run():
            for i in range(10):
                t = 1 + i % (n - 1)
                T._launch_pair(frames[t], frames[t - 1], mvs[t - 1],
                               depth[t] if reject else None, depth[t - 1] if reject else None,
                               normals[t] if reject else None, normals[t - 1] if reject else None,
                               (1.0, 1.0), 5.0, 0.3, 0.2, psum[t - 1], pcnt[t - 1])
        return run

    rec["kernel_pair_ms"] = round(median_ms(pairs(True), args.reps) / 10, 4)
    rec["kernel_pair_position_only_ms"] = round(median_ms(pairs(False), args.reps) / 10, 4)
    rec["kernel_finalize_ms"] = round(median_ms(
        lambda: [T._finalize(psum, pcnt, n - 1, (B, C, H, W), per, "valid") for _ in range(10)],
        args.reps) / 10, 4)
    rec["pair_TB_per_s"] = round(pair_bytes / (rec["kernel_pair_ms"] * 1e-3) / 1e12, 2)
    rec["speedup_vs_aten"] = round(rec["aten_ms"] / rec["call_ms"], 1)
    print(f"{args.shape} x {n} frames, {args.mv} motion, {rec['lib']}: call {rec['call_ms']:.3f} ms "
          f"(position only {rec['call_position_only_ms']:.3f}, unadjusted {rec['unadjusted_ms']:.3f}); ATen "
          f"{rec['aten_ms']:.3f} ms ({rec['speedup_vs_aten']}x); pair kernel {rec['kernel_pair_ms']:.4f} ms "
          f"= {rec['pair_TB_per_s']} TB/s of {rec['pair_MB']} MB (position only "
          f"{rec['kernel_pair_position_only_ms']:.4f}); finalize {rec['kernel_finalize_ms']:.4f} ms; "
          f"value {rec['value']:.6f} vs ATen {rec['aten_value']:.6f}", flush=True)
    print(json.dumps({"temporal_probe": rec}))


if __name__ == "__main__":
    main()
