"""The paper's feature-sensitivity analysis (§3.2, Eq. 1): which input channels
(G-buffers) does the network's output depend on?

    S_i = E[ |phi(f_i + eps_i) - phi(f_i)| ] / (factor * sigma_i),
          eps_i ~ N(0, factor * sigma_i) per pixel of channel i only
    s_i = S_i / sum_j S_j            (the paper rejects buffers with s_i < 1.5 %)

`absolute` is S_i, `relative` is s_i, `signed` is Eq. 1 read literally (without
the absolute value: the mean drift of the output, near zero for a symmetric
perturbation), and `terms` [C', R, B, 2] holds, per variant and image, the sum
of |d| and of d over the output pixels, so that any other normalisation can be
formed without a second pass.

The expectation runs over R repeats, the images of the batch and the output
pixels. The work is a plan of N = B * (1 + C' * R) image slots: the B
unperturbed images first, then variant (i, r) of image b at slot
B + ((i_idx * R + r) * B + b). One GraphedUnet is captured for `chunk` slots;
each step of the loop writes `chunk` slots of the plan straight into its static
input (nsm_sens_variants), replays the eval forward and folds the outputs
against the kept base outputs (nsm_sens_reduce). The last chunk's filler slots
hold a base image and are ignored. Nothing synchronises with the host: the
results are device tensors, and reading them is the only wait.

`sigma`: a [C] tensor or sequence, one float for every channel, or "batch" for
the unbiased per-channel std of the given batch (nsm_channel_std, what
PerturbationLoss.perturb_input uses). Inputs normalised by FrameLoader have a
dataset sigma of 1. For raw inputs the paper's sigma_i ("aggregating all pixels
in the dataset") is dataset_stats(...).stds or ChannelStats (nsm_amd/stats.py).
"""
from collections import namedtuple

import torch

from ._lib import call, lib, ptr, require_gpu, stream
from .infer import GraphedUnet

SensitivityResult = namedtuple("SensitivityResult", "absolute relative signed terms")

_MASK64 = (1 << 64) - 1
_SEED_STEP = 0x9E3779B97F4A7C15   # successive update() calls draw from distant keys


def _check_args(shape, sigma, repeats, factor, channels, chunk, noises=None):
    """Host-side argument checks (no GPU work). Returns the channel list."""
    if len(shape) != 4:
        raise ValueError(f"feature sensitivity: inputs must be [B,C,H,W], got {tuple(shape)}")
    B, C, H, W = shape
    if isinstance(repeats, bool) or not isinstance(repeats, int) or repeats < 1:
        raise ValueError(f"feature sensitivity: repeats must be an integer >= 1, got {repeats!r}")
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"feature sensitivity: chunk must be an integer >= 1, got {chunk!r}")
    if not float(factor) > 0:
        raise ValueError(f"feature sensitivity: factor must be > 0, got {factor!r}")
    if isinstance(sigma, str):
        if sigma != "batch":
            raise ValueError(f"feature sensitivity: sigma must be a [C] tensor or sequence, a "
                             f"float or 'batch', got {sigma!r}")
    elif torch.is_tensor(sigma):
        if sigma.dim() > 1 or (sigma.dim() == 1 and sigma.numel() != C):
            raise ValueError(f"feature sensitivity: sigma is {tuple(sigma.shape)}, expected ({C},)")
    elif not isinstance(sigma, (int, float)):
        try:
            n = len(sigma)
        except TypeError:
            raise ValueError(f"feature sensitivity: sigma must be a [C] tensor or sequence, a "
                             f"float or 'batch', got {sigma!r}") from None
        if n != C:
            raise ValueError(f"feature sensitivity: sigma has {n} entries, expected {C}")
    chans = list(range(C)) if channels is None else [int(c) for c in channels]
    if not chans:
        raise ValueError("feature sensitivity: channels is empty")
    for c in chans:
        if not 0 <= c < C:
            raise ValueError(f"feature sensitivity: channel {c} out of range for {C} channels")
    if len(set(chans)) != len(chans):
        raise ValueError(f"feature sensitivity: channels repeats an index: {chans}")
    if noises is not None:
        want = (len(chans), repeats, B, H, W)
        if not torch.is_tensor(noises) or tuple(noises.shape) != want:
            got = tuple(noises.shape) if torch.is_tensor(noises) else type(noises).__name__
            raise ValueError(f"feature sensitivity: noises is {got}, expected {want}")
    if chunk * C > 65535:
        raise ValueError(f"feature sensitivity: chunk * C = {chunk * C} exceeds 65535 planes")
    return chans


def _draw_seed():
    # torch's host generator: a CPU tensor, no device involved
    return int(torch.randint(0, 1 << 62, (1,), dtype=torch.int64))


def sens_variants(x, sigma, channels, repeats, factor, first, n, out, noises=None, seed=0):
    """Write the slots [first, first + n) of the plan into `out` [n,C,H,W] (fp32,
    contiguous, on x's device). x [B,C,H,W] fp32, sigma [C] fp32 and `channels`
    (an int32 tensor of indices below C, or None for all) live on the device."""
    B, C, H, W = x.shape
    Cs = channels.numel() if channels is not None else C
    call("nsm_sens_variants", ptr(x), ptr(sigma), ptr(channels), ptr(noises), seed & _MASK64,
         B, C, H, W, Cs, repeats, float(factor), first, n, ptr(out), stream())
    return out


def sens_reduce(out, base, first, B, Cs, repeats, psum):
    """Fold the outputs `out` [n_slots, n] of the slots [first, first + n_slots)
    against `base` [B, n] into psum [Cs * repeats * B, nsm_sens_blocks(n), 2]."""
    n_slots, n = out.shape
    call("nsm_sens_reduce", ptr(out), ptr(base), first, n_slots, B, Cs, repeats, n, ptr(psum),
         stream())
    return psum


class FeatureSensitivity:
    """feature_sensitivity as the expectation over a dataset: update(inputs) per
    batch, compute() for the result so far, reset() to start over.

    The sums of |d|, of d and the element counts are kept per channel in device
    fp64 accumulators, so the batches of a sequence give what one call on their
    concatenation gives, up to the order of summation. The captured forward is
    kept between updates and re-captured when the input shape or the model's
    compute dtype changes. `sigma="batch"` takes each batch's own std. With the
    device generator each update draws from a key of its own. compute() returns
    device tensors (`terms` are those of the last update) without a host
    synchronisation."""

    def __init__(self, model, sigma, repeats=4, factor=0.1, channels=None, chunk=8, seed=None):
        C = model.conv2.conv[0].in_channels // 4 if hasattr(model, "conv2") else None
        if C is not None:
            _check_args((1, C, 2, 2), sigma, repeats, factor, channels, chunk)
        self.model, self.sigma = model, sigma
        self.repeats, self.factor, self.channels, self.chunk = repeats, float(factor), channels, chunk
        self.seed = _draw_seed() if seed is None else int(seed)
        self._graph = self._graph_key = None
        self._acc = self._chan = self._res = None
        self._updates = 0

    def reset(self):
        if self._acc is not None:
            self._acc.zero_()
        self._res = None
        self._updates = 0

    def _sigma_dev(self, x):
        C, dev = x.shape[1], x.device
        if isinstance(self.sigma, str):
            std = torch.empty(C, dtype=torch.float32, device=dev)
            B, _, H, W = x.shape
            call("nsm_channel_std", ptr(x), B, C, H, W, None, ptr(std), stream())
            return std
        if torch.is_tensor(self.sigma):
            s = self.sigma.detach().to(device=dev, dtype=torch.float32)
            return (s.expand(C) if s.dim() == 0 else s).contiguous()
        if isinstance(self.sigma, (int, float)):
            return torch.full((C,), float(self.sigma), dtype=torch.float32, device=dev)
        return torch.tensor([float(v) for v in self.sigma], dtype=torch.float32, device=dev)

    def _captured(self, x):
        shape = (self.chunk,) + tuple(x.shape[1:])
        key = (shape, x.device, getattr(self.model, "compute_dtype", None))
        if self._graph is None or self._graph_key != key:
            example = torch.zeros(shape, dtype=torch.float32, device=x.device)
            example[:] = x[0]
            self._graph, self._graph_key = GraphedUnet(self.model, example), key
        return self._graph

    def update(self, inputs, noises=None):
        if not torch.is_tensor(inputs):
            raise ValueError("feature sensitivity: inputs must be a [B,C,H,W] tensor")
        chans = _check_args(tuple(inputs.shape), self.sigma, self.repeats, self.factor,
                            self.channels, self.chunk, noises)
        dev = require_gpu(inputs, "feature-sensitivity inputs").device
        x = inputs.detach().contiguous().to(torch.float32)
        B, C, H, W = x.shape
        Cs, R, chunk = len(chans), self.repeats, self.chunk
        if B * (1 + Cs * R) >= 1 << 31:
            raise ValueError("feature sensitivity: too many variants")
        sig = self._sigma_dev(x)
        if self._chan is None or self._chan.device != dev:
            self._chan = torch.tensor(chans, dtype=torch.int32, device=dev)
        if self._acc is None or self._acc.device != dev:
            self._acc = torch.zeros((Cs, 3), dtype=torch.float64, device=dev)
        nz = None
        if noises is not None:
            nz = noises.detach().to(device=dev, dtype=torch.float32).contiguous()
        seed = (self.seed + self._updates * _SEED_STEP) & _MASK64
        g = self._captured(x)
        out = g.static_out
        if out.dtype != torch.float32 or not out.is_contiguous() or out.shape[0] != chunk:
            raise RuntimeError(f"feature sensitivity: the model's output must be contiguous fp32 "
                               f"[chunk, ...], got {tuple(out.shape)} {out.dtype}")
        out = out.view(chunk, -1)
        n = out.shape[1]
        per = lib.nsm_sens_blocks(n)
        if per <= 0:
            raise ValueError(f"feature sensitivity: unsupported output size {n}")
        V = Cs * R * B
        base = torch.empty((B, n), dtype=torch.float32, device=dev)
        psum = torch.empty((V, per, 2), dtype=torch.float32, device=dev)
        for first in range(0, B + V, chunk):
            sens_variants(x, sig, self._chan, R, self.factor, first, chunk, g.static_in, nz, seed)
            g.replay()
            if first < B:   # the base outputs are kept from the first replays
                nb = min(chunk, B - first)
                base[first:first + nb].copy_(out[:nb])
            if first + chunk > B:
                sens_reduce(out, base, first, B, Cs, R, psum)
        terms = torch.empty((Cs, R, B, 2), dtype=torch.float32, device=dev)
        res = [torch.empty(Cs, dtype=torch.float32, device=dev) for _ in range(3)]
        call("nsm_sens_finalize", ptr(psum), Cs, R, B, n, ptr(sig), ptr(self._chan), self.factor,
             ptr(terms), ptr(self._acc), ptr(res[0]), ptr(res[1]), ptr(res[2]), stream())
        self._res = SensitivityResult(res[0], res[2], res[1], terms)
        self._updates += 1

    def compute(self):
        if self._res is None:
            raise RuntimeError("FeatureSensitivity.compute() before the first update()")
        return self._res


def feature_sensitivity(model, inputs, sigma, *, repeats=4, factor=0.1, channels=None, chunk=8,
                        seed=None, noises=None):
    """SensitivityResult(absolute [C'], relative [C'], signed [C'], terms
    [C',R,B,2]) of `model` on `inputs` [B,C,H,W] (on the GPU, any size the model
    accepts), as fp32 device tensors; see the module docstring.

    The model runs in eval mode under no_grad in the compute dtype it is set
    to, and its training flag is restored. `channels` restricts the analysis to
    a subset (C' entries, in the given order). `noises` [C',R,B,H,W] supplies
    the standard normals (parity tests); otherwise they come from the device
    generator keyed by `seed` (None: drawn once from torch's host generator).
    Argument errors raise ValueError before any GPU work. Every call captures
    the forward anew: for more than one batch use FeatureSensitivity."""
    if not torch.is_tensor(inputs):
        raise ValueError("feature sensitivity: inputs must be a [B,C,H,W] tensor")
    _check_args(tuple(inputs.shape), sigma, repeats, factor, channels, chunk, noises)
    acc = FeatureSensitivity(model, sigma, repeats=repeats, factor=factor, channels=channels,
                             chunk=chunk, seed=seed)
    acc.update(inputs, noises=noises)
    return acc.compute()
