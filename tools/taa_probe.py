#!/usr/bin/env python3
"""Time the temporal anti-aliasing resolve (nsm_taa_resolve, nsm_amd/taa.py) with
HIP events, and in the same process what it is measured against:

  * the kernel alone, with and without the 3x3 neighbourhood clamp, and the
    metric's temporal_pair_kernel (the same gathers, no neighbourhood, no
    output plane), measured before and after so that its own spread shows;
  * the whole TemporalAA call against an ATen composition of the same pass
    (F.grid_sample on history / depth / normals, two max_pool2d for the
    bounds, clamp, lerp, where: what a user would otherwise run), and the error
    of one step of each against the same ATen ops in float64;
  * with --eval, one eval forward of the U-Net at the same resolution through
    GraphedUnet (bf16), for the pass's share of a frame.

    python tools/taa_probe.py [--shape 1x1x1080x1920] [--frames 8] [--reps 20]
                              [--mv random|smooth] [--eval]

Median of --reps after warm-up; kernel-only figures from 10 back-to-back
launches per event pair over --frames different frame sets (more bytes than the
256 MB Infinity Cache holds). Bytes a frame must move, counted from shapes, per
pixel: cur 4C, history 4C (each pixel once: neighbouring pixels share taps),
out 4C, motion vectors 8, and with rejection depth 8 and normals 24 (both
frames). Both conditions (position only, depth + normal rejection) are
measured. Prints one line per condition and a final JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import nsm_amd  # noqa: E402
from nsm_amd import taa as A  # noqa: E402
from nsm_amd import temporal as T  # noqa: E402

DEPTH_TOL, NORMAL_COS, BLEND = 0.3, 0.2, 0.1


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


def aten_step(cur, hist, mv, z, zp, n, np_, dtype=torch.float32):
    """One resolve from ATen ops in `dtype`: (out, accepted [B,H,W])."""
    cur, hist, mv = cur.to(dtype), hist.to(dtype), mv.to(dtype)
    B, C, H, W = cur.shape
    x = torch.arange(W, device=cur.device, dtype=dtype).view(1, 1, W)
    y = torch.arange(H, device=cur.device, dtype=dtype).view(1, H, 1)
    px, py = x + mv[:, 0], y + mv[:, 1]
    ok = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    grid = torch.stack([2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1], dim=-1)
    src = torch.cat([hist, zp.to(dtype), np_.to(dtype)], dim=1) if z is not None else hist
    s = F.grid_sample(src, grid, mode="bilinear", padding_mode="border", align_corners=True)
    if z is not None:
        z, n = z.to(dtype), n.to(dtype)
        ok &= (z[:, 0] - s[:, C]).abs() <= DEPTH_TOL * z[:, 0].abs()
        ok &= (n * s[:, C + 1:]).sum(1) >= NORMAL_COS
    hi = F.max_pool2d(cur, 3, stride=1, padding=1)      # -inf padding = replicated edges
    lo = -F.max_pool2d(-cur, 3, stride=1, padding=1)
    h = torch.minimum(torch.maximum(s[:, :C], lo), hi)
    keep = 1 - torch.tensor(BLEND, dtype=torch.float32).to(dtype).item()
    return torch.where(ok.unsqueeze(1), torch.lerp(cur, h, keep), cur), ok


class AtenTAA:
    """TemporalAA from ATen ops (float32), streaming, with its own copies of the
    previous depth and normals as TemporalAA keeps them."""

    def __init__(self):
        self.hist = self.z = self.n = None

    def __call__(self, cur, mv, z, n):
        if self.hist is None:
            self.hist = cur.clone()
        else:
            self.hist, _ = aten_step(cur, self.hist, mv, z, self.z, n, self.n)
        if z is not None:
            self.z, self.n = z.clone(), n.clone()
        return self.hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x1x1080x1920")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mv", choices=("random", "smooth"), default="random",
                    help="random: N(0, 2.5 px) per pixel (no two neighbours agree: the gathers' "
                         "worst case); smooth: a pan of (3.3, -1.7) px plus a slow 1.5 px wave "
                         "(a moving camera)")
    ap.add_argument("--eval", action="store_true",
                    help="also time one bf16 eval forward (7 input channels) at this resolution")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, C, H, W = (int(v) for v in args.shape.split("x"))
    n = args.frames
    g = torch.Generator(device=dev).manual_seed(0)
    frames = [torch.rand(B, C, H, W, device=dev, generator=g) for _ in range(n)]
    if args.mv == "random":
        mvs = [2.5 * torch.randn(B, 2, H, W, device=dev, generator=g) for _ in range(n)]
    else:
        yy = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
        xx = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
        mvs = [torch.stack([3.3 + 1.5 * torch.sin(xx / 97 + yy / 61 + i).expand(B, H, W),
                            -1.7 + 1.5 * torch.cos(xx / 83 - yy / 71 + i).expand(B, H, W)], dim=1)
               .contiguous() for i in range(n)]
    depth = [1 + torch.rand(B, 1, H, W, device=dev, generator=g) for _ in range(n)]
    normals = [F.normalize(torch.randn(B, 3, H, W, device=dev, generator=g)
                           + torch.tensor([0.0, 0.0, 2.0], device=dev).view(1, 3, 1, 1), dim=1)
               for _ in range(n)]
    outs = [torch.empty(B, C, H, W, device=dev) for _ in range(n)]
    per = T._blocks((B, C, H, W))
    psum = torch.empty((n, B, per), dtype=torch.float32, device=dev)
    pcnt = torch.empty((n, B, per), dtype=torch.int32, device=dev)
    pix = B * H * W
    rec = {"shape": [B, C, H, W], "frames": n, "mv": args.mv,
           "lib": os.path.basename(nsm_amd.LIB_PATH)}

    def rej(seq, t, reject):
        return seq[t] if reject else None

    def taa_kernel(reject, clamp):
        def run():
            for i in range(10):
                t = i % n
                A._launch(frames[t], frames[t - 1], mvs[t], rej(depth, t, reject),
                          rej(depth, t - 1, reject), rej(normals, t, reject),
                          rej(normals, t - 1, reject), (1.0, 1.0), BLEND, clamp, DEPTH_TOL,
                          NORMAL_COS, outs[t])
        return run

    def pair_kernel(reject):
        def run():
            for i in range(10):
                t = i % n
                T._launch_pair(frames[t], frames[t - 1], mvs[t], rej(depth, t, reject),
                               rej(depth, t - 1, reject), rej(normals, t, reject),
                               rej(normals, t - 1, reject), (1.0, 1.0), 5.0, DEPTH_TOL, NORMAL_COS,
                               psum[t], pcnt[t])
        return run

    for reject in (False, True):
        r = {}
        extra = 32 if reject else 0
        r["taa_bytes_per_pixel"] = 12 * C + 8 + extra
        r["pair_bytes_per_pixel"] = 8 * C + 8 + extra
        r["pair_kernel_ms"] = [round(median_ms(pair_kernel(reject), args.reps) / 10, 4)]
        r["taa_kernel_ms"] = round(median_ms(taa_kernel(reject, 1), args.reps) / 10, 4)
        r["taa_kernel_noclamp_ms"] = round(median_ms(taa_kernel(reject, 0), args.reps) / 10, 4)
        r["pair_kernel_ms"].append(round(median_ms(pair_kernel(reject), args.reps) / 10, 4))
        r["taa_kernel_TB_per_s"] = round(pix * r["taa_bytes_per_pixel"]
                                         / (r["taa_kernel_ms"] * 1e-3) / 1e12, 2)
        r["taa_over_pair"] = round(r["taa_kernel_ms"] / min(r["pair_kernel_ms"]), 3)
        r["byte_ratio"] = round(r["taa_bytes_per_pixel"] / r["pair_bytes_per_pixel"], 3)

        # the whole call, streaming over the n frame sets, against ATen
        kw = dict(depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
        fused, aten = nsm_amd.TemporalAA(BLEND, **kw), AtenTAA()

        def stream(obj):
            def run():
                for t in range(n):
                    obj(frames[t], mvs[t], rej(depth, t, reject), rej(normals, t, reject))
            return run

        r["call_ms"] = round(median_ms(stream(fused), args.reps) / n, 4)
        r["aten_call_ms"] = round(median_ms(stream(aten), args.reps) / n, 4)
        r["speedup_vs_aten"] = round(r["aten_call_ms"] / r["call_ms"], 1)
        r["call_TB_per_s"] = round(pix * r["taa_bytes_per_pixel"] / (r["call_ms"] * 1e-3) / 1e12, 2)
        # agreement on one step from the same history: both against the ATen ops in
        # float64, on the pixels where all three verdicts agree
        t, p = n - 1, n - 2
        step = (frames[t], frames[p], mvs[t], rej(depth, t, reject), rej(depth, p, reject),
                rej(normals, t, reject), rej(normals, p, reject))
        a, acc = nsm_amd.taa_resolve(*step[:3], depth=step[3], prev_depth=step[4], normals=step[5],
                                     prev_normals=step[6], blend=BLEND, return_mask=True, **kw)
        b, ok32 = aten_step(*step)
        ref, ok64 = aten_step(*step, dtype=torch.float64)
        same = ((acc[:, 0] == ok64) & (ok32 == ok64)).unsqueeze(1)
        r["accepted_share"] = round(acc.float().mean().item(), 4)
        r["verdicts_differing_from_f64"] = int((acc[:, 0] != ok64).sum().item())
        r["aten_verdicts_differing_from_f64"] = int((ok32 != ok64).sum().item())
        r["max_abs_err_vs_f64"] = float(((a.double() - ref).abs() * same).max().item())
        r["aten_max_abs_err_vs_f64"] = float(((b.double() - ref).abs() * same).max().item())
        rec["reject" if reject else "position"] = r
        print(f"{args.shape}, {args.mv} motion, {'depth+normal rejection' if reject else 'position only'}: "
              f"kernel {r['taa_kernel_ms']:.4f} ms = {r['taa_kernel_TB_per_s']} TB/s of "
              f"{r['taa_bytes_per_pixel']} B/pixel (no clamp {r['taa_kernel_noclamp_ms']:.4f}); pair "
              f"kernel {r['pair_kernel_ms']} ms, ratio {r['taa_over_pair']} (bytes {r['byte_ratio']}); "
              f"call {r['call_ms']:.4f} ms vs ATen {r['aten_call_ms']:.4f} ms "
              f"({r['speedup_vs_aten']}x); one step against ATen in float64: max|d| "
              f"{r['max_abs_err_vs_f64']:.2e} (ATen float32 {r['aten_max_abs_err_vs_f64']:.2e})", flush=True)

    if args.eval:
        model = nsm_amd.Unet(in_ch=7, dropout_rate=0.2).to(dev).eval()
        model.set_compute_dtype(torch.bfloat16)
        graphed = nsm_amd.GraphedUnet(model, torch.randn(B, 7, H, W, device=dev, generator=g))
        rec["eval_bf16_ms"] = round(median_ms(graphed.replay, args.reps), 4)
        rec["taa_share_of_eval_frame"] = round(
            rec["position"]["call_ms"] / (rec["eval_bf16_ms"] + rec["position"]["call_ms"]), 3)
        print(f"eval forward (bf16, graph replay) {rec['eval_bf16_ms']:.3f} ms", flush=True)
    print(json.dumps({"taa_probe": rec}))


if __name__ == "__main__":
    main()
