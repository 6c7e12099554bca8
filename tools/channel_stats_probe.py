#!/usr/bin/env python3
"""Time ChannelStats.update (nsm_stats_partial + nsm_stats_merge, nsm_amd/stats.py)
with HIP events, and in the same process what the parent commit offers for the
same figures:

  * an ATen composition: torch.var_mean of the fp64 cast over dims (0, 2, 3) plus
    amin and amax;
  * nsm_channel_std (one block per channel, two sweeps, fp32, sigma only);
  * device copies of the same bytes as the bandwidth yardstick: ATen's
    vectorised elementwise kernel (x * 1 into a second buffer, 16 bytes per
    lane) and Tensor.copy_.

    python tools/channel_stats_probe.py [--rounds 30] [--shapes 8x7x512x512,1x7x1080x1920]

Every measurement is one event pair around one call on each of the rotated
input buffers: more than 256 MiB of distinct inputs, so the Infinity Cache
does not serve the reads (the copies' destinations rotate too). The rounds
interleave the methods in one process; median and minimum per call are
reported. Rates: the statistics pass reads the bytes once; a copy reads and
writes them, and `copy_TB_per_s` counts both. `fraction_of_copy` is the
pass's read rate over the faster copy's rate. Prints one line per shape and a
final JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
import torch  # noqa: E402

import nsm_amd  # noqa: E402
from nsm_amd._lib import call, lib, ptr, stream  # noqa: E402
from nsm_amd.stats import REC, _empty_state  # noqa: E402

ROTATE_BYTES = 320 << 20


def timed(fn, n):
    """ms per call of fn(i), i over the n rotated buffers, from one event pair."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def probe(shape, rounds, dev):
    B, C, H, W = shape
    nbytes = 4 * B * C * H * W
    n = -(-ROTATE_BYTES // nbytes) + 1
    g = torch.Generator(device=dev).manual_seed(0)
    xs = [1000 + 0.01 * torch.randn(shape, device=dev, generator=g) for _ in range(n)]
    dsts = [torch.empty_like(xs[0]) for _ in range(n)]
    acc = nsm_amd.ChannelStats(C)
    std = torch.empty(C, dtype=torch.float32, device=dev)
    per = lib.nsm_stats_blocks(H * W)
    ws = torch.empty(B * C * per * REC, dtype=torch.float64, device=dev)
    state = _empty_state(C, dev)

    def aten(i):
        var, mean = torch.var_mean(xs[i].double(), dim=(0, 2, 3), unbiased=False)
        return var, mean, xs[i].amin(dim=(0, 2, 3)), xs[i].amax(dim=(0, 2, 3))

    methods = {
        "update": lambda i: acc.update(xs[i]),
        "update_per_frame": lambda i: acc.update(xs[i], per_frame=True),
        "partial_kernel": lambda i: call("nsm_stats_partial", ptr(xs[i]), B, C, H * W, ptr(ws),
                                         stream()),
        "merge_kernel": lambda i: call("nsm_stats_merge", ptr(ws), B, C, per, None, ptr(state),
                                       stream()),
        "aten": aten,
        "channel_std": lambda i: call("nsm_channel_std", ptr(xs[i]), B, C, H, W, None, ptr(std),
                                      stream()),
        "copy_mul": lambda i: torch.mul(xs[i], 1.0, out=dsts[i]),
        "copy_": lambda i: dsts[i].copy_(xs[i]),
    }
    for k, fn in methods.items():   # warm-up: every kernel loaded, every buffer touched
        timed(fn, n)
    # the same n updates replayed from one HIP graph: the device's time for the two
    # launches, without the host's (two ctypes calls and the argument checks)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        acc.update(xs[0])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(n):
            acc.update(xs[i])
    replay = lambda i: graph.replay() if i == 0 else None  # noqa: E731
    methods = {"update_graph": replay, **methods}
    timed(replay, n)
    ts = {k: [] for k in methods}
    for _ in range(rounds):
        for k, fn in methods.items():
            ts[k].append(timed(fn, n))
    rec = {"shape": list(shape), "MB": round(nbytes / 1e6, 1), "buffers": n, "rounds": rounds}
    for k, v in ts.items():
        v = sorted(v)
        rec[k + "_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4)}
    tb = lambda ms, mult=1: mult * nbytes / (ms * 1e-3) / 1e12  # noqa: E731
    copy = max(tb(rec[k + "_ms"]["median"], 2) for k in ("copy_mul", "copy_"))
    rec["copy_TB_per_s"] = round(copy, 2)
    rec["update_read_TB_per_s"] = round(tb(rec["update_ms"]["median"]), 2)
    rec["fraction_of_copy"] = round(rec["update_read_TB_per_s"] / copy, 3)
    rec["partial_read_TB_per_s"] = round(tb(rec["partial_kernel_ms"]["median"]), 2)
    rec["update_graph_read_TB_per_s"] = round(tb(rec["update_graph_ms"]["median"]), 2)
    rec["graph_fraction_of_copy"] = round(rec["update_graph_read_TB_per_s"] / copy, 3)
    rec["speedup_vs_aten"] = round(rec["aten_ms"]["median"] / rec["update_ms"]["median"], 1)
    rec["speedup_vs_channel_std"] = round(
        rec["channel_std_ms"]["median"] / rec["update_ms"]["median"], 1)
    # agreement at this size, on the last buffer: sigma against the fp64 ATen figure
    res = nsm_amd.channel_stats(xs[-1])
    var, mean, _, _ = aten(n - 1)
    rec["sigma_rel_diff_vs_aten_f64"] = float(((res.stds - var.sqrt()).abs() / var.sqrt()).max())
    call("nsm_channel_std", ptr(xs[-1]), B, C, H, W, None, ptr(std), stream())
    rec["channel_std_rel_diff_vs_aten_f64"] = float(
        ((std.double() - res.std()).abs() / res.std()).max())
    print(f"{'x'.join(map(str, shape))} ({rec['MB']} MB, {n} buffers): update "
          f"{rec['update_ms']} ms = {rec['update_read_TB_per_s']} TB/s read, replayed from a "
          f"graph {rec['update_graph_ms']} = {rec['update_graph_read_TB_per_s']} TB/s "
          f"({rec['graph_fraction_of_copy']} of the copy), "
          f"(partial kernel alone {rec['partial_kernel_ms']} = {rec['partial_read_TB_per_s']} TB/s, "
          f"merge alone {rec['merge_kernel_ms']}), "
          f"{rec['fraction_of_copy']} of the copy's {rec['copy_TB_per_s']} TB/s (mul "
          f"{rec['copy_mul_ms']}, copy_ {rec['copy__ms']}); per-frame {rec['update_per_frame_ms']}; "
          f"ATen {rec['aten_ms']} ({rec['speedup_vs_aten']}x); nsm_channel_std "
          f"{rec['channel_std_ms']} ({rec['speedup_vs_channel_std']}x)", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x7x512x512,1x7x1080x1920")
    ap.add_argument("--rounds", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    recs = [probe(tuple(int(v) for v in s.split("x")), args.rounds, dev)
            for s in args.shapes.split(",")]
    print(json.dumps({"channel_stats_probe": {"lib": os.path.basename(nsm_amd.LIB_PATH),
                                              "shapes": recs}}))


if __name__ == "__main__":
    main()
