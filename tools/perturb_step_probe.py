#!/usr/bin/env python3
"""Time the perturbation-loss training step (EnhancedCustomLoss, the paper's
Eq. 2) with HIP events: forward, the criterion with its three perturbed
forwards, backward and the FlatAdamW device tail, on 7x512x512 inputs.

    python tools/perturb_step_probe.py [--configs f32:8,bf16:8,bf16:64] [--steps 20]
                                       [--reps 20]

Per configuration (compute dtype : batch), in one process and alternating, so
that a difference can be read against the spread of the repeated run:
  (a) the eager step as it was: fused=False, noise="torch" (timed three times:
      first, between and last);
  (b) the eager step with fused=True, noise="device" (timed twice);
  (c) (b) replayed from GraphedTrainStep (timed twice).
Each window is --steps steps between two events after warm-up steps of the same
kind. Alone, as the median of --reps event pairs around one call each:
  * nsm_perturb_variants (device noise, P = 3) against three torch.randn_like +
    nsm_perturb, on the step's input, both from a std computed before; the
    nsm_channel_std launch both paths start with; and the whole perturb_input
    call (std included) of either noise source;
  * the fused loss node, forward + backward, against the 1 + P L1 nodes and the
    0-dim arithmetic that combines them, on the step's output shape.
The models of (a) and (b)/(c) start from the same weights; the probe reads
nothing outside the repository and prints one JSON record at the end."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pcss-unet_amd"))
import torch  # noqa: E402

import nsm_amd  # noqa: E402
from nsm_amd import losses as LS  # noqa: E402
from nsm_amd._lib import call, ptr, stream  # noqa: E402

C, H, P = 7, 512, 3
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


def build(dev, dtype, fused, noise):
    torch.manual_seed(0)
    m = nsm_amd.Unet(in_ch=C, dropout_rate=0.2).to(dev).train()
    if dtype != torch.float32:
        m.set_compute_dtype(dtype)
    opt = nsm_amd.FlatAdamW(m.parameters(), lr=7e-4, weight_decay=1e-3, max_grad_norm=1.0,
                            sanitize=True)
    crit = nsm_amd.EnhancedCustomLoss(dev, alpha=0.9, perturb_weight=0.5, vgg_weights=False,
                                      fused=fused, noise=noise)
    return m, opt, crit


def eager(m, opt, crit, x, y):
    def step():
        total, _ = crit(m, m(x), y, x)
        total.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    return step


def step_times(dev, dtype, B, steps):
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, C, H, H, device=dev, generator=g)
    y = torch.randint(0, 256, (B, 1, H, H), device=dev, generator=g).float() / 255.0
    ma, oa, ca = build(dev, dtype, False, "torch")
    mb, ob, cb = build(dev, dtype, True, "device")
    a, b = eager(ma, oa, ca, x, y), eager(mb, ob, cb, x, y)
    r = {"a_eager_ms": [], "b_eager_fused_ms": [], "c_replay_ms": []}
    r["a_eager_ms"].append(window_ms(a, steps))
    r["b_eager_fused_ms"].append(window_ms(b, steps))
    r["a_eager_ms"].append(window_ms(a, steps))
    r["b_eager_fused_ms"].append(window_ms(b, steps))
    graphed = nsm_amd.GraphedTrainStep(mb, cb, ob, x, y, warmup=1)
    r["c_replay_ms"].append(window_ms(graphed, steps))
    r["a_eager_ms"].append(window_ms(a, steps))
    r["c_replay_ms"].append(window_ms(graphed, steps))
    cb.check_range_now()
    # the weight-preparation launch every forward starts with (four per step)
    sws = list(mb.__dict__.get("_step_weights", {}).values())
    r["prep_weights_ms"] = [median_ms(sw.run, 10) for sw in sws]
    r = {k: [round(v, 3) for v in vs] for k, vs in r.items()}
    am = sorted(r["a_eager_ms"])[1]
    r["a_spread_pct"] = round(100 * (max(r["a_eager_ms"]) - min(r["a_eager_ms"])) / am, 2)
    for k in ("a_eager_ms", "b_eager_fused_ms", "c_replay_ms"):
        r[k.replace("_ms", "_frames_per_s")] = round(B / min(r[k]) * 1e3, 1)
    r["b_over_a"] = round(min(r["b_eager_fused_ms"]) / am, 4)
    r["c_over_a"] = round(min(r["c_replay_ms"]) / am, 4)
    return r, x


def kernel_times(dev, x, reps):
    B = x.shape[0]
    r = {}
    Cx, Hx, Wx = x.shape[1:]
    std = torch.empty(Cx, dtype=torch.float32, device=dev)
    out = torch.empty((P,) + tuple(x.shape), dtype=torch.float32, device=dev)

    def channel_std():
        call("nsm_channel_std", ptr(x), B, Cx, Hx, Wx, None, ptr(std), stream())

    def variants():
        call("nsm_perturb_variants", ptr(x), ptr(std), None, 1234, None, P, B, Cx, Hx, Wx, 0.01,
             ptr(out), stream())

    def randn_perturb():
        for i in range(P):
            n = torch.randn_like(x)
            call("nsm_perturb", ptr(x), ptr(n), ptr(std), B, Cx, Hx, Wx, 0.01, ptr(out[i]),
                 stream())

    # what both paths run first (unchanged), then the two ways to the P variants
    r["channel_std_ms"] = median_ms(channel_std, reps)
    r["perturb_3x_randn_nsm_perturb_ms"] = [median_ms(randn_perturb, reps)]
    r["perturb_variants_ms"] = median_ms(variants, reps)
    r["perturb_3x_randn_nsm_perturb_ms"].append(median_ms(randn_perturb, reps))
    # bytes the one launch must move: x once and P outputs
    r["perturb_variants_GB_per_s"] = round((1 + P) * x.numel() * 4 / r["perturb_variants_ms"] / 1e6, 1)
    old, new = nsm_amd.PerturbationLoss(), nsm_amd.PerturbationLoss(noise="device")
    r["perturb_input_torch_ms"] = [median_ms(lambda: old.perturb_input(x), reps)]
    r["perturb_input_device_ms"] = median_ms(lambda: new.perturb_input(x), reps)
    r["perturb_input_torch_ms"].append(median_ms(lambda: old.perturb_input(x), reps))
    g = torch.Generator(device=dev).manual_seed(2)
    o = torch.rand(B, 1, H, H, device=dev, generator=g).requires_grad_(True)
    t = torch.rand(B, 1, H, H, device=dev, generator=g)
    ps = [(o.detach() + 0.01 * torch.randn(B, 1, H, H, device=dev, generator=g)) for _ in range(P)]

    def nodes():
        tot = 0
        for p in ps:
            tot = tot + LS.l1_loss(o, p)
        total = 0.9 * LS.l1_loss(o, t) + 0.5 * (tot / P)
        total.backward()
        o.grad = None

    def fused():
        LS._PertLossFn.apply(o, t, 0.9, 0.5, None, *ps)[0].backward()
        o.grad = None

    r["loss_nodes_fwd_bwd_ms"] = [median_ms(nodes, reps)]
    r["loss_fused_fwd_bwd_ms"] = median_ms(fused, reps)
    r["loss_nodes_fwd_bwd_ms"].append(median_ms(nodes, reps))
    # forward reads o, t and P outputs; backward reads them again and writes the gradient
    r["loss_fused_GB_per_s"] = round((2 * (2 + P) + 1) * o.numel() * 4
                                     / r["loss_fused_fwd_bwd_ms"] / 1e6, 1)
    return {k: ([round(v, 4) for v in vs] if isinstance(vs, list) else round(vs, 4))
            for k, vs in r.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="f32:8,bf16:8,bf16:64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perturb_step_probe: needs a ROCm GPU (timings are device events)")
    dev = torch.device("cuda:0")
    rec = {"lib": os.path.basename(nsm_amd.LIB_PATH), "steps": args.steps, "reps": args.reps,
           "input": [C, H, H], "P": P}
    for cfg in args.configs.split(","):
        name, b = cfg.split(":")
        B = int(b)
        r, x = step_times(dev, DTYPES[name], B, args.steps)
        r["kernels"] = kernel_times(dev, x, args.reps)
        rec[f"{name}_B{B}"] = r
        k = r["kernels"]
        print(f"{name} B={B}: (a) eager {r['a_eager_ms']} ms/step (spread {r['a_spread_pct']} %), "
              f"(b) eager fused+device noise {r['b_eager_fused_ms']}, (c) replay {r['c_replay_ms']}; "
              f"frames/s a {r['a_eager_frames_per_s']} b {r['b_eager_fused_frames_per_s']} "
              f"c {r['c_replay_frames_per_s']}; channel_std {k['channel_std_ms']} ms; variants "
              f"{k['perturb_variants_ms']} ms vs {k['perturb_3x_randn_nsm_perturb_ms']}; "
              f"perturb_input {k['perturb_input_device_ms']} ms vs {k['perturb_input_torch_ms']}; "
              f"loss fwd+bwd {k['loss_fused_fwd_bwd_ms']} ms "
              f"vs {k['loss_nodes_fwd_bwd_ms']}", flush=True)
        del x
        torch.cuda.empty_cache()
    print(json.dumps({"perturb_step_probe": rec}))


if __name__ == "__main__":
    main()
