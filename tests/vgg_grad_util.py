"""Shared helpers of the VGG-gradient tests (test infrastructure): the seeded
cases, the float64 autograd reference of the perceptual loss, and the
fixed-decision gradient.

The gradient of sum_i w_i * mean|f_i(o) - f_i(t)| is piecewise constant in the
features: the discrete decisions are sign(y - t) at the taps, the ReLU masks
y > 0 and the argmax of every pool window. With those held fixed (taken from a
given set of activations) the map upstream -> d/do is linear:
`fixed_decision_grad` evaluates it in float64 with conv_transpose2d, so a
comparison against it leaves only the rounding of the convolutions.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vgg_ref as V

# the constants of the fp32 path, as doubles: float32(0.485) and ATen's
# float32(0.229) + float32(1e-8)
MEAN64 = float(np.float32(V.MEAN))
DENOM64 = float(np.float32(V.STD) + np.float32(V.EPS))

CONV_IDX = tuple(i for i, kind, _, _ in V.layers() if kind == "conv" and i <= max(V.FEATURE_LAYERS))

# (B, H, W, seed): cases at which fp32 CPU autograd stays within 3e-7 of the
# float64 one (the reference sits far from its own sign / mask flips)
CASES = {"b1_40x72": (1, 40, 72, 1), "b2_96x128": (2, 96, 128, 2), "b1_32x48": (1, 32, 48, 3)}


def nhwc(x):  # [B,C,H,W] -> [B*H*W, C]
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


def nchw(y, B, H, W):
    return y.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def inputs(name):
    """(o, t) of a case: o = sigmoid(randn) drawn first, t = rand second, from
    one generator."""
    B, H, W, seed = CASES[name]
    gen = torch.Generator().manual_seed(seed)
    o = torch.sigmoid(torch.randn(B, 1, H, W, generator=gen))
    t = torch.rand(B, 1, H, W, generator=gen)
    return o, t


@functools.lru_cache(maxsize=None)
def state64():
    return {k: v.double() for k, v in V.standin_state().items()}


def prep64(img):
    """oracle.vgg_ref.prep in float64 (same constants as the fp32 path)."""
    x = torch.nan_to_num(torch.clamp(img.double(), 0.0, 1.0), nan=0.5, posinf=1.0, neginf=0.0)
    return (x.repeat(1, 3, 1, 1) - MEAN64) / DENOM64


def weights64():
    return [float(w) for w in V.normalized_weights()]


@functools.lru_cache(maxsize=None)
def autograd64(name):
    """(loss, d loss / d o, {conv idx: pre-ReLU output of [o; t], float64}) of
    the plain float64 autograd evaluation. Computed once per case; callers must
    not modify what they get."""
    o, t = inputs(name)
    B = o.shape[0]
    o64 = o.double().requires_grad_(True)
    acts = V.features(state64(), prep64(torch.cat([o64, t.double()])), CONV_IDX)
    loss = 0.0
    for w, idx in zip(weights64(), V.FEATURE_LAYERS):
        loss = loss + w * F.l1_loss(acts[idx][:B], acts[idx][B:])
    loss.backward()
    return loss.detach(), o64.grad.detach(), {k: v.detach() for k, v in acts.items()}


def fixed_decision_grad(o, acts, sd=None, upstream=1.0):
    """d loss / d o in float64 with every discrete decision read from `acts` =
    {conv idx: pre-ReLU output [2B, C, h, w]} (images 0..B-1: output, B..2B-1:
    target; any float dtype). o: [B,1,H,W] (its clamp mask is the one decision
    taken from the input)."""
    sd = state64() if sd is None else sd
    B = o.shape[0]
    wts = dict(zip(V.FEATURE_LAYERS, weights64()))
    g, relu, pool = None, False, False
    for idx, kind, _, _ in reversed([l for l in V.layers() if l[0] <= max(V.FEATURE_LAYERS)]):
        if kind == "relu":
            relu = True
            continue
        if kind == "pool":
            pool = True
            continue
        y, yt = acts[idx][:B], acts[idx][B:]
        if pool:
            # ATen's window scan: first maximum in row-major order, NaN wins
            m, ind = F.max_pool2d(y, 2, 2, return_indices=True)
            g = F.max_unpool2d(g * (m > 0), ind, 2, 2, output_size=y.shape[-2:])
        elif relu and g is not None:
            g = g * (y > 0)
        if idx in wts:
            tap = (wts[idx] * upstream / y.numel()) * torch.sign(y.double() - yt.double())
            g = tap if g is None else g + tap
        relu = pool = False
        g = F.conv_transpose2d(g, sd[f"{idx}.weight"], padding=1)
    inside = (o >= 0) & (o <= 1)
    return g.sum(1, keepdim=True) / DENOM64 * inside
