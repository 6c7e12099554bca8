#!/usr/bin/env python3
"""Kernel times of the three device-tail update kernels (tail_adamw_kernel,
tail_adam_kernel, tail_sgd_kernel with and without momentum) on the Unet's own
flat parameter buffer, side by side in one process. Run it under the kernel
trace and summarise:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \
        python3 tools/optim_tail_probe.py [iterations]
    python3 tools/kstats.py OUT/.../run_kernel_stats.csv

The four optimizers step in turn on buffers of their own (about 0.7 GiB in
all), so no kernel finds its operands in the 256 MiB Infinity Cache left there
by its previous launch, as in a training step, where the forward and backward
run in between. Prints the bytes each kernel moves per launch."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pcss-unet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import nsm_amd
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shapes = [p.shape for p in nsm_amd.Unet(in_ch=7).parameters()]
    kw = dict(lr=7e-4, max_grad_norm=1.0, sanitize=True, seed=1)
    opts = []
    for cls, okw, bytes_per in ((nsm_amd.FlatAdamW, {}, 28), (nsm_amd.FlatAdam, {}, 28),
                                (nsm_amd.FlatSGD, {"momentum": 0.9}, 20),
                                (nsm_amd.FlatSGD, {"momentum": 0.0}, 12)):
        ps = [torch.nn.Parameter(torch.randn(s, device=dev) * 0.02) for s in shapes]
        opt = cls(ps, **okw, **kw)
        g = torch.randn(opt.flat.numel(), device=dev) * 1e-4    # norm < 1: a taken step
        off = 0
        for p in ps:
            p.grad = g[off:off + p.numel()].view_as(p)
            off += p.numel()
        opts.append((opt, bytes_per))
    for _ in range(iters):
        for opt, _ in opts:
            opt.step()
    torch.cuda.synchronize()
    for opt, bytes_per in opts:
        n = opt.flat.numel()
        mu = opt.param_groups[0].get("momentum")
        print(f"{type(opt).__name__}{'' if mu is None else f'(momentum={mu})'}: {n} elements, "
              f"{opt.steps_taken()} steps taken, {bytes_per} B/element = "
              f"{n * bytes_per / 1e6:.1f} MB per launch")


if __name__ == "__main__":
    main()
