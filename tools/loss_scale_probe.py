#!/usr/bin/env python3
"""What the dynamic loss scaler costs in the device tail: FlatAdamW's step on the
Unet's own flat parameter buffer (15.7 M parameters) with a static loss scale
(`grad_scale=`, nsm_grad_tail) and with a device scaler (`grad_scaler=`,
nsm_grad_tail_scaled), alternating in one process on buffers of their own, each
step timed with HIP events.

    python3 tools/loss_scale_probe.py [measured steps, default 20] [warm-up, default 5]

Prints the median, minimum and maximum of each and one JSON line. Both take the
same gradient (scaled by 1024, a taken step) and the scaler's growth interval is
never reached, so the two do the same work apart from the scaler's reads and
its update in tail_finalize_kernel."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pcss-unet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import nsm_amd
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warm = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shapes = [p.shape for p in nsm_amd.Unet(in_ch=7).parameters()]
    scale = 1024.0
    scaler = nsm_amd.GradScaler(init_scale=scale, growth_interval=1 << 30, device=dev)
    opts = {}
    for name, kw in (("static", dict(grad_scale=scale)), ("scaled", dict(grad_scaler=scaler))):
        ps = [torch.nn.Parameter(torch.randn(s, device=dev) * 0.02) for s in shapes]
        opt = nsm_amd.FlatAdamW(ps, lr=7e-4, max_grad_norm=1.0, sanitize=True, seed=1, **kw)
        g = torch.randn(opt.flat.numel(), device=dev) * (1e-4 * scale)   # unscaled norm < 1
        off = 0
        for p in ps:
            p.grad = g[off:off + p.numel()].view_as(p)
            off += p.numel()
        opts[name] = opt
    times = {name: [] for name in opts}
    for it in range(warm + iters):
        # strict alternation: each step runs after the other optimizer's, whose
        # 0.25 GB of operands have displaced its own from the Infinity Cache (two
        # steps of one optimizer in a row measure 160 us, not 190)
        for name, opt in opts.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            opt.step()
            t1.record()
            t1.synchronize()
            if it >= warm:
                times[name].append(t0.elapsed_time(t1) * 1e3)
    out = {"elements": opts["static"].flat.numel(), "steps": iters}
    for name, ts in times.items():
        taken = opts[name].steps_taken()
        assert taken == warm + iters, (name, taken)
        out[name] = {"median_us": round(statistics.median(ts), 1), "min_us": round(min(ts), 1),
                     "max_us": round(max(ts), 1), "all_us": [round(t, 1) for t in ts]}
        print(f"{name}: median {out[name]['median_us']} us, min {out[name]['min_us']}, "
              f"max {out[name]['max_us']} over {iters} steps")
    assert scaler.last()["scale"] == scale
    print(json.dumps(out))


if __name__ == "__main__":
    main()
