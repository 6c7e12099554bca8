#!/usr/bin/env python3
"""Time the inference frame path (nsm_frame_prep / nsm_frame_finish,
nsm_amd/frames.py) with HIP events, and in the same process what it is measured
against:

  * prepare_frames (pad + scrub + normalise) and finish_frames (scrub + clip +
    uint8 channels-last + the fp32 frame) against the same passes from ATen ops
    (F.pad(mode="reflect"), nan_to_num, the normalisation; nan_to_num, clamp,
    mul, to(uint8), permute), both sides without the `.any()` host checks;
  * each against a device-to-device copy of the bytes the pass must move
    (source + outputs, counted from shapes), on the same box: the ceiling;
  * with --eval, the whole FramePipeline replay against GraphedUnet alone at
    the padded size (bf16): the difference is the frame path's cost per frame.

    python tools/frame_probe.py [--shape 1x7x1080x1920] [--sets 32] [--reps 20] [--eval]

Median of --reps after warm-up, 10 back-to-back calls per event pair (the
kernels through the C ABI, and the Python calls with their host-side checks)
over --sets different buffers (32 of the smallest pass, 18.7 MB at 1080p, are
more bytes than the 256 MB Infinity Cache holds). The results
of both sides are compared before anything is timed. Prints one line per pass
and a final JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import nsm_amd  # noqa: E402
from nsm_amd._lib import call, ptr, stream  # noqa: E402
from nsm_amd.frames import padded_size  # noqa: E402


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


def aten_prep(x, pad, mean, std):
    y = F.pad(x, (0, pad[1], 0, pad[0]), mode="reflect") if any(pad) else x
    y = torch.nan_to_num(y, nan=0.0, posinf=1.0, neginf=0.0)
    return (y - mean) / (std + 1e-8)


def aten_finish(o, size):
    v = torch.nan_to_num(o[..., :size[0], :size[1]], nan=0.0, posinf=1.0, neginf=0.0).clamp(0, 1)
    u8 = (v * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return (u8[..., 0] if u8.shape[-1] == 1 else u8), v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x7x1080x1920", help="the raw frames, BxCxHxW")
    ap.add_argument("--out-channels", type=int, default=1, help="channels of the network's output")
    ap.add_argument("--sets", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--eval", action="store_true",
                    help="also time FramePipeline against GraphedUnet (bf16) at this shape")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, C, H, W = (int(v) for v in args.shape.split("x"))
    Hp, Wp = padded_size(H, W)
    Co, n = args.out_channels, args.sets
    g = torch.Generator(device=dev).manual_seed(0)
    raws = [torch.randn(B, C, H, W, device=dev, generator=g) for _ in range(n)]
    for r in raws:
        r.view(-1)[::100003] = float("nan")
    nets = [torch.rand(B, Co, Hp, Wp, device=dev, generator=g) * 1.2 - 0.1 for _ in range(n)]
    mean = torch.randn(C, device=dev, generator=g)
    std = torch.rand(C, device=dev, generator=g) + 0.5
    mean4, std4 = mean.view(1, C, 1, 1), std.view(1, C, 1, 1)
    ins = [torch.empty(B, C, Hp, Wp, device=dev) for _ in range(n)]
    u8s = [torch.empty((B, H, W) if Co == 1 else (B, H, W, Co), dtype=torch.uint8, device=dev)
           for _ in range(n)]
    f32s = [torch.empty(B, Co, H, W, device=dev) for _ in range(n)]
    rec = {"raw": [B, C, H, W], "padded": [Hp, Wp], "out_channels": Co, "sets": n,
           "lib": os.path.basename(nsm_amd.LIB_PATH)}

    # the two sides agree (prep up to the division's last bit, finish exactly)
    a = nsm_amd.prepare_frames(raws[0], stats=(mean, std))
    b = aten_prep(raws[0], (Hp - H, Wp - W), mean4, std4)
    rec["prep_max_abs_diff_vs_aten"] = float((a - b).abs().max().item())
    u8, f32 = aten_finish(nets[0], (H, W))
    got = nsm_amd.finish_frames(nets[0], (H, W), out_f32=f32s[0])
    assert torch.equal(got, u8) and torch.equal(f32s[0], f32)
    assert rec["prep_max_abs_diff_vs_aten"] <= 1e-5 * float(b.abs().max().item())

    def loop(fn):
        def run():
            for i in range(10):
                fn(i % n)
        return run

    def copy_ms(nbytes):
        src = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(n)]
        dst = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(n)]
        return median_ms(loop(lambda t: dst[t].copy_(src[t])), args.reps) / 10

    def k_prep(t):
        call("nsm_frame_prep", ptr(raws[t]), B, C, H, W, Hp, Wp, ptr(mean), ptr(std), 1e-8, 1,
             ptr(ins[t]), None, None, stream())

    def k_finish(with_f32):
        def run(t):
            call("nsm_frame_finish", ptr(nets[t]), B, Co, Hp, Wp, H, W, ptr(u8s[t]),
                 ptr(f32s[t]) if with_f32 else None, None, None, stream())
        return run

    # name: (bytes, the kernel through the C ABI, the Python call, the ATen ops)
    passes = {
        "prep": (4 * B * C * (H * W + Hp * Wp), k_prep,
                 lambda t: nsm_amd.prepare_frames(raws[t], stats=(mean, std), out=ins[t]),
                 lambda t: aten_prep(raws[t], (Hp - H, Wp - W), mean4, std4)),
        "finish": (B * Co * H * W * (4 + 4 + 1), k_finish(True),
                   lambda t: nsm_amd.finish_frames(nets[t], (H, W), out_u8=u8s[t], out_f32=f32s[t]),
                   lambda t: aten_finish(nets[t], (H, W))),
        "finish_u8_only": (B * Co * H * W * (4 + 1), k_finish(False),
                           lambda t: nsm_amd.finish_frames(nets[t], (H, W), out_u8=u8s[t]),
                           lambda t: aten_finish(nets[t], (H, W))[0]),
    }
    for name, (nbytes, kernel, fused, aten) in passes.items():
        r = {"bytes": nbytes}
        r["copy_ms"] = [round(copy_ms(nbytes), 4)]
        r["fused_ms"] = round(median_ms(loop(kernel), args.reps) / 10, 4)
        r["call_ms"] = round(median_ms(loop(fused), args.reps) / 10, 4)
        r["aten_ms"] = round(median_ms(loop(aten), args.reps) / 10, 4)
        r["copy_ms"].append(round(copy_ms(nbytes), 4))
        r["fused_TB_per_s"] = round(nbytes / (r["fused_ms"] * 1e-3) / 1e12, 2)
        r["speedup_vs_aten"] = round(r["aten_ms"] / r["fused_ms"], 1)
        r["fused_over_copy"] = round(r["fused_ms"] / min(r["copy_ms"]), 2)
        rec[name] = r
        print(f"{args.shape} {name}: kernel {r['fused_ms']:.4f} ms = {r['fused_TB_per_s']} TB/s of "
              f"{nbytes / 1e6:.1f} MB (Python call {r['call_ms']:.4f} ms); ATen {r['aten_ms']:.4f} ms "
              f"({r['speedup_vs_aten']}x); D2D copy of the same bytes {r['copy_ms']} ms (kernel / copy "
              f"{r['fused_over_copy']})", flush=True)

    if args.eval:
        model = nsm_amd.Unet(in_ch=C, out_ch=Co, dropout_rate=0.2).to(dev).eval()
        model.set_compute_dtype(torch.bfloat16)
        graphed = nsm_amd.GraphedUnet(model, torch.randn(B, C, Hp, Wp, device=dev, generator=g))
        pipe = nsm_amd.FramePipeline(model, raws[0], stats=(mean, std), crop=True)
        rec["graphed_unet_ms"] = [round(median_ms(graphed.replay, args.reps), 4)]
        rec["pipeline_ms"] = round(median_ms(pipe.replay, args.reps), 4)
        rec["graphed_unet_ms"].append(round(median_ms(graphed.replay, args.reps), 4))
        rec["frame_path_ms"] = round(rec["pipeline_ms"] - min(rec["graphed_unet_ms"]), 4)
        print(f"eval forward at {Hp}x{Wp} (bf16, graph replay) {rec['graphed_unet_ms']} ms; "
              f"FramePipeline replay {rec['pipeline_ms']:.4f} ms: the frame path costs "
              f"{rec['frame_path_ms']:.4f} ms per frame", flush=True)
    print(json.dumps({"frame_probe": rec}))


if __name__ == "__main__":
    main()
