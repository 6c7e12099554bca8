#!/usr/bin/env python3
"""Time the validation pass (nsm_amd/validation.py) with HIP events against what
the parent commit offers for the same figures, in one process, the methods
interleaved; median (and minimum) of --rounds measurements after a warm-up.

(a) The metrics pass (nsm_metrics_partial + nsm_metrics_merge through
    ImageMetrics.update with the per-image table) against the same six figures
    per image composed from ATen ops (fp64 difference, isfinite masks, sums,
    amax), at 1x1x1080x1920 and 8x1x512x512. One event pair around one call on
    each of the rotated buffer pairs: more than 256 MiB of distinct inputs, so
    the Infinity Cache does not serve the reads. Both read output and target
    once at least; `read_TB_per_s` counts the two tensors once.
(b) One validation batch through Validator (graph replay; `compute()` once per
    measurement of --batches batches, inside the timed window) against the loop
    a user writes without it: eager eval forward under no_grad, the criterion,
    `criterion.l1`, two `.item()` calls per batch (main.py:611-625). 8x7x512x512
    in fp32 and under bf16 autocast. The losses of both are compared.

    python tools/validation_probe.py [--rounds 20] [--batches 5] [--skip-b]

Prints one line per measurement and a final JSON record."""
import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
import torch  # noqa: E402

import nsm_amd  # noqa: E402

ROTATE_BYTES = 320 << 20


def timed(fn, n):
    """ms per call of fn(i), i over n, from one event pair."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4)}


def aten_records(o, t, lo=0.0, hi=1.0):
    """[B, 6] fp64: the record of every image from ATen ops."""
    B = o.shape[0]
    o, t = o.reshape(B, -1), t.reshape(B, -1)
    fin = torch.isfinite(o) & torch.isfinite(t)
    d = torch.where(fin, (o.double() - t.double()).abs(), 0.0)
    return torch.stack([fin.sum(1).double(), d.sum(1), (d * d).sum(1), d.amax(1),
                        (~fin).sum(1).double(),
                        (fin & ((o < lo) | (o > hi))).sum(1).double()], dim=1)


def probe_metrics(shape, rounds, dev):
    nbytes = 2 * 4 * torch.Size(shape).numel()
    n = -(-ROTATE_BYTES // nbytes) + 1
    g = torch.Generator(device=dev).manual_seed(0)
    os_ = [torch.rand(shape, device=dev, generator=g) for _ in range(n)]
    ts_ = [torch.rand(shape, device=dev, generator=g) for _ in range(n)]
    acc = nsm_amd.ImageMetrics()
    methods = {"metrics": lambda i: acc.update(os_[i], ts_[i], per_image=True),
               "aten": lambda i: aten_records(os_[i], ts_[i])}
    for fn in methods.values():
        timed(fn, n)
    # the same n updates replayed from one graph: the device's time for the two launches
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(n):
            acc.update(os_[i], ts_[i], per_image=True)
    methods = {"metrics_graph": lambda i: graph.replay() if i == 0 else None, **methods}
    timed(methods["metrics_graph"], n)
    ms = {k: [] for k in methods}
    for _ in range(rounds):
        for k, fn in methods.items():
            ms[k].append(timed(fn, n))
    rec = {"shape": list(shape), "MB_read": round(nbytes / 1e6, 1), "buffers": n, "rounds": rounds}
    for k, v in ms.items():
        rec[k + "_ms"] = stats(v)
    tb = lambda t: nbytes / (t * 1e-3) / 1e12  # noqa: E731
    rec["metrics_read_TB_per_s"] = round(tb(rec["metrics_ms"]["median"]), 2)
    rec["metrics_graph_read_TB_per_s"] = round(tb(rec["metrics_graph_ms"]["median"]), 2)
    rec["speedup_vs_aten"] = round(rec["aten_ms"]["median"] / rec["metrics_ms"]["median"], 1)
    got = nsm_amd.ImageMetrics().update(os_[-1], ts_[-1], per_image=True)
    ref = aten_records(os_[-1], ts_[-1])
    rec["max_rel_diff_vs_aten"] = float(((got - ref).abs() / ref.abs().clamp_min(1e-300)).max())
    print(f"(a) {'x'.join(map(str, shape))}: metrics {rec['metrics_ms']} ms = "
          f"{rec['metrics_read_TB_per_s']} TB/s read, from a graph {rec['metrics_graph_ms']} = "
          f"{rec['metrics_graph_read_TB_per_s']} TB/s; ATen {rec['aten_ms']} "
          f"({rec['speedup_vs_aten']}x); rel diff {rec['max_rel_diff_vs_aten']:.1e}", flush=True)
    return rec


def probe_validator(shape, mode, rounds, batches, dev):
    B, C, H, W = shape
    torch.manual_seed(0)
    m = nsm_amd.Unet(in_ch=C).to(dev).eval()
    crit = nsm_amd.CustomLoss(dev, 0.9, vgg_weights=False)
    g = torch.Generator(device=dev).manual_seed(1)
    data = [(torch.randn(shape, device=dev, generator=g),
             torch.rand((B, 1, H, W), device=dev, generator=g)) for _ in range(batches)]

    def ctx():
        return torch.autocast("cuda", dtype=torch.bfloat16) if mode == "bf16" \
            else contextlib.nullcontext()

    last = {}

    def baseline(_):
        val_loss = val_l1 = 0.0
        with torch.no_grad(), ctx():
            for x, y in data:
                out = m(x)
                loss = crit(out, y, x)
                l1 = crit.l1(out, y)
                val_loss += loss.item()
                val_l1 += l1.item()
        last["baseline"] = (val_loss / batches, val_l1 / batches)

    with ctx():
        val = nsm_amd.Validator(m, crit, *data[0])

    def graphed(_):
        val.reset()
        for x, y in data:
            val.update(x, y)
        res = val.compute()
        last["validator"] = (res.loss, res.l1_loss)
        last["mse"] = res.metrics.mse

    methods = {"validator": graphed, "baseline": baseline}
    for fn in methods.values():
        for _ in range(3):
            timed(fn, 1)
    ms = {k: [] for k in methods}
    for _ in range(rounds):
        for k, fn in methods.items():
            ms[k].append(timed(fn, 1) / batches)
    rec = {"shape": list(shape), "mode": mode, "batches": batches, "rounds": rounds}
    for k, v in ms.items():
        rec[k + "_ms_per_batch"] = stats(v)
    rec["speedup"] = round(rec["baseline_ms_per_batch"]["median"]
                           / rec["validator_ms_per_batch"]["median"], 3)
    rec["loss"] = {k: last[k] for k in ("validator", "baseline")}
    rec["mse"] = last["mse"]
    print(f"(b) {'x'.join(map(str, shape))} {mode}: Validator {rec['validator_ms_per_batch']} "
          f"ms a batch, the eager loop {rec['baseline_ms_per_batch']} ({rec['speedup']}x); "
          f"(loss, l1) {last['validator']} against {last['baseline']}", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--metric-shapes", default="1x1x1080x1920,8x1x512x512")
    ap.add_argument("--val-shape", default="8x7x512x512")
    ap.add_argument("--skip-b", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    shape = lambda s: tuple(int(v) for v in s.split("x"))  # noqa: E731
    out = {"lib": os.path.basename(nsm_amd.LIB_PATH),
           "metrics": [probe_metrics(shape(s), args.rounds, dev)
                       for s in args.metric_shapes.split(",")]}
    if not args.skip_b:
        out["validator"] = [probe_validator(shape(args.val_shape), mode, args.rounds,
                                            args.batches, dev) for mode in ("fp32", "bf16")]
    print(json.dumps({"validation_probe": out}))


if __name__ == "__main__":
    main()
