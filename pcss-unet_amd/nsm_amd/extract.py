"""Learned feature extraction: the paper's "2-layer deep 1x1 convolution
network" (§3.2) that compresses the composed G-buffer channels U to the U-Net's
four inputs and is trained end to end with it: the yardstick a hand-selected
channel subset is measured against.

    ext = FeatureExtractor(15, 4)                  # 15 -> 16 -> 4, LeakyReLU(0.2)
    model = ExtractedUnet(ext, Unet(in_ch=4)).cuda()
    opt = make_optimizer(model.parameters(), ...)  # the extractor's four parameters too
    out = model(x15)                               # [B,15,H,W] fp32 -> the U-Net's output

`FeatureExtractor` holds the plain torch module (`self.net`: Conv2d 1x1,
LeakyReLU, Conv2d 1x1), so its state_dict and initialisation are torch's and a
checkpoint moves freely between the two. On a GPU tensor the forward and the
backward are one fused pass each (csrc/nsm_extract.hip): the hidden activations
never reach memory, only `x` is kept for the backward, and the parameter
gradients are reduced without atomics in a fixed order, so a step is bitwise
reproducible and graph-capturable. On a CPU tensor it runs `self.net`.
"""
import torch
import torch.nn as nn

from ._lib import call, lib, ptr, stream

MAX_IN, MAX_HIDDEN, MAX_OUT = 32, 32, 16


def extract_bwd_plan(B, Cin, H, W, hidden, Cout):
    """The backward's work split (host-only): {"grid": blocks, "tiles": tiles of
    `tile_units` units of `unit_pixels` consecutive columns of a row, "grid_cap":
    the most blocks any shape gets, "partial": floats of one block's partial}.
    Block k folds the tiles k, k + grid, ..."""
    import ctypes
    plan = (ctypes.c_int32 * 6)()
    call("nsm_extract_bwd_plan", B, Cin, H, W, hidden, Cout, plan)
    keys = ("grid", "tiles", "tile_units", "unit_pixels", "grid_cap", "partial")
    return dict(zip(keys, (int(v) for v in plan)))


def _check(x, w1, b1, w2, b2, what):
    for t, name in ((x, "x"), (w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2")):
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
        if not t.is_cuda:
            raise ValueError(f"{what}: {name} must be on a ROCm GPU device (got {t.device})")
    Hd, Cin = w1.shape[0], w1.shape[1]
    Cout = w2.shape[0]
    if x.dim() != 4 or x.shape[1] != Cin:
        raise ValueError(f"{what}: x must be [B,{Cin},H,W], got {tuple(x.shape)}")
    if w1.numel() != Hd * Cin or b1.numel() != Hd or w2.numel() != Cout * Hd or \
            w2.shape[1] != Hd or b2.numel() != Cout:
        raise ValueError(f"{what}: parameter shapes {tuple(w1.shape)}, {tuple(b1.shape)}, "
                         f"{tuple(w2.shape)}, {tuple(b2.shape)} are not those of two 1x1 "
                         "convolutions")
    return Cin, Hd, Cout


def extract_forward(x, w1, b1, w2, b2, negative_slope, out=None):
    """y [B,Cout,H,W] of the two 1x1 convolutions around LeakyReLU(negative_slope)
    over x [B,Cin,H,W] (fp32, on the GPU), one launch. The parameters are
    Conv2d's ([Hd,Cin,1,1] or [Hd,Cin], [Hd], [Cout,Hd,1,1] or [Cout,Hd], [Cout]).
    No autograd."""
    Cin, Hd, Cout = _check(x, w1, b1, w2, b2, "extract_forward")
    x = x.detach().contiguous()
    B, _, H, W = x.shape
    if out is None:
        out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)
    call("nsm_extract_fwd", ptr(x), B, Cin, H, W, ptr(w1.detach().contiguous()),
         ptr(b1.detach().contiguous()), Hd, ptr(w2.detach().contiguous()),
         ptr(b2.detach().contiguous()), Cout, float(negative_slope), ptr(out), stream())
    return out


def extract_backward(x, dy, w1, b1, w2, b2, negative_slope, need_dx=True):
    """(dx or None, dw1, db1, dw2, db2) from x, dy and the parameters: one
    streaming launch and the fixed-order merge of its block partials. The hidden
    activations are recomputed with the forward's arithmetic; the gradients come
    in the parameters' shapes. Bitwise reproducible."""
    Cin, Hd, Cout = _check(x, w1, b1, w2, b2, "extract_backward")
    x = x.detach().contiguous()
    dy = dy.detach().contiguous()
    B, _, H, W = x.shape
    if tuple(dy.shape) != (B, Cout, H, W) or dy.dtype != torch.float32 or dy.device != x.device:
        raise ValueError(f"extract_backward: dy must be float32 {(B, Cout, H, W)} on {x.device}, "
                         f"got {dy.dtype} {tuple(dy.shape)} on {dy.device}")
    dev = x.device
    nbytes = lib.nsm_extract_bwd_ws(B, Cin, H, W, Hd, Cout)
    if nbytes <= 0:
        raise ValueError(f"extract_backward: unsupported shape {tuple(x.shape)} -> {Hd} -> {Cout}")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    dw1, db1, dw2, db2 = (torch.empty_like(t, memory_format=torch.contiguous_format)
                          for t in (w1, b1, w2, b2))
    dx = torch.empty_like(x) if need_dx else None
    call("nsm_extract_bwd", ptr(x), ptr(dy), B, Cin, H, W, ptr(w1.detach().contiguous()),
         ptr(b1.detach().contiguous()), Hd, ptr(w2.detach().contiguous()),
         ptr(b2.detach().contiguous()), Cout, float(negative_slope), ptr(dw1), ptr(db1), ptr(dw2),
         ptr(db2), ptr(dx), ptr(ws), stream())
    return dx, dw1, db1, dw2, db2


class _ExtractFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, slope):
        ctx.slope = slope
        ctx.save_for_backward(x, w1, b1, w2, b2)
        return extract_forward(x, w1, b1, w2, b2, slope)

    @staticmethod
    def backward(ctx, dy):
        x, w1, b1, w2, b2 = ctx.saved_tensors
        dx, dw1, db1, dw2, db2 = extract_backward(x, dy, w1, b1, w2, b2, ctx.slope,
                                                  need_dx=ctx.needs_input_grad[0])
        return dx, dw1, db1, dw2, db2, None


class FeatureExtractor(nn.Module):
    """The per-pixel MLP in_channels -> hidden -> out_channels (1 <= in_channels,
    hidden <= 32, 1 <= out_channels <= 16; the paper's is 15 -> 16 -> 4). Input
    [B,C,H,W] or [C,H,W] ([1,C,H,W]), float32: it computes in fp32 inside any
    autocast region, and the U-Net behind it picks its own compute dtype."""

    def __init__(self, in_channels=15, out_channels=4, hidden=16, negative_slope=0.2):
        super().__init__()
        for v, name, hi in ((in_channels, "in_channels", MAX_IN), (hidden, "hidden", MAX_HIDDEN),
                            (out_channels, "out_channels", MAX_OUT)):
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= hi:
                raise ValueError(f"FeatureExtractor: {name} must be an integer in [1, {hi}], got "
                                 f"{v!r}")
        self.in_channels, self.out_channels, self.hidden = in_channels, out_channels, hidden
        self.negative_slope = float(negative_slope)
        self.net = nn.Sequential(nn.Conv2d(in_channels, hidden, 1),
                                 nn.LeakyReLU(self.negative_slope),
                                 nn.Conv2d(hidden, out_channels, 1))

    def forward(self, x):
        if not torch.is_tensor(x) or x.dim() not in (3, 4):
            got = tuple(x.shape) if torch.is_tensor(x) else type(x).__name__
            raise ValueError(f"FeatureExtractor: input must be [B,C,H,W] or [C,H,W], got {got}")
        if x.dtype != torch.float32:
            raise ValueError(f"FeatureExtractor: input must be float32, got {x.dtype}")
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if x.shape[1] != self.in_channels:
            raise ValueError(f"FeatureExtractor: built for {self.in_channels} channels, got "
                             f"{x.shape[1]}")
        if not x.is_cuda:
            return self.net(x)
        c1, c2 = self.net[0], self.net[2]
        with torch.autocast("cuda", enabled=False):
            return _ExtractFn.apply(x, c1.weight, c1.bias, c2.weight, c2.bias, self.negative_slope)


class ExtractedUnet(nn.Module):
    """The paper's cascade: forward(x) = unet(extractor(x)), trained end to end.
    What GraphedTrainStep, GraphedUnet / FramePipeline and feature_sensitivity
    read from a model is delegated to the U-Net."""

    def __init__(self, extractor, unet):
        super().__init__()
        want = getattr(unet, "in_ch", None)
        if extractor.out_channels != want:
            raise ValueError(f"ExtractedUnet: the extractor gives {extractor.out_channels} "
                             f"channels, the U-Net takes {want}")
        self.extractor, self.unet = extractor, unet

    def forward(self, x):
        return self.unet(self.extractor(x))

    @property
    def _grad_allreduce(self):
        return self.unet._grad_allreduce

    @property
    def compute_dtype(self):
        return self.unet.compute_dtype

    def set_compute_dtype(self, dtype):
        self.unet.set_compute_dtype(dtype)
        return self

    def data_parallel(self, *args, **kwargs):
        raise NotImplementedError("ExtractedUnet.data_parallel: the extractor's gradients are not "
                                  "in the U-Net's all-reduce buckets, so the ranks would drift "
                                  "apart; data-parallel training of the cascade is not supported")

    overlap_grad_allreduce = data_parallel
