"""Losses of the hot path on the libnsm kernels.

* `L1Loss` / `l1_loss`: nn.L1Loss (mean) — customLoss.py:96,134.
* `CustomLoss(device, alpha=0.9)`: returns alpha*L1 + (1-alpha)*vgg
  (customLoss.py:129-193). The reference's VGG term is a DETACHED constant
  (`torch.tensor(total_loss, requires_grad=True)`, customLoss.py:90), so the
  gradient is exactly alpha*sign(o-t)/N. The VGG19 perceptual value
  (`nsm_amd.vgg.MultiLayerVGGLoss`, on the libnsm kernels) needs the ImageNet
  weights the reference downloads at construction (customLoss.py:20,97). By
  default (`vgg_weights="auto"`) the torchvision checkpoint is taken from
  $NSM_VGG19_WEIGHTS or torch.hub's cache (`<hub>/checkpoints/
  vgg19-dcbb9e9d.pth`, loaded with weights_only=True); when neither exists the
  loss warns once that its VGG term is 0. Other values: a .pth path, a
  state_dict, a MultiLayerVGGLoss, "random", or False (term off, no warning);
  any `vgg=<callable(out, target)>` overrides. The gradient is the same either
  way. `vgg_grad=True` (opt-in; departs from the reference, matches the paper's
  loss) keeps the value and lets the VGG term carry its gradient:
  alpha*sign(o-t)/N + (1-alpha)*dVGG/do, from one autograd node whose backward
  runs the VGG chain (nsm_amd.vgg) and then accumulates the L1 gradient into
  the same buffer. It needs nsm_amd's own VGG stack: with `vgg=<callable>` or
  without weights it raises ValueError.
  `detail_weight` / `gradient_weight` (opt-in, default 0: the path above,
  unchanged) switch on the reference's `enhanced_loss` (customLoss.py:139-185):
  base + detail_weight*(HF + PEN) + gradient_weight*SOB with the high-frequency
  L1 (image minus its 5x5 Gaussian blur), the penumbra L1 (0.1 < target < 0.9)
  and the Sobel-magnitude L1, fused in nsm_detail_loss_fwd/bwd; still one
  autograd node and one gradient buffer. [B,1,H,W] only (ValueError otherwise).
  `detail_terms(output, target)` returns the three terms as device scalars.
  `ssim_weight` (opt-in, default 0: every path above, unchanged) adds the
  reference's commented-out structural-similarity term (customLoss.py:187-191,
  `1 - pytorch_msssim.ssim(output, target)`, weight 0.1 there):
  final = enhanced + ssim_weight*(1 - ssim), fused in nsm_ssim_fwd/bwd; one
  autograd node and one gradient buffer with every combination of `vgg_grad`,
  `detail_weight` and `gradient_weight` (backward order: VGG chain, L1, detail,
  SSIM). `ssim_data_range` (default 1.0, the range of the sigmoid output) is
  pytorch_msssim's `data_range`; the reference's literal call passes none and
  would have used that package's default 255, which on [0, 1] images makes the
  term almost constant (1 - ssim of the order 1e-5): `ssim_data_range=255.0`
  reproduces it. [B,1,H,W] with H, W >= 11 only (ValueError otherwise).
* `ssim(output, target, data_range=1.0, size_average=True)`: pytorch_msssim.ssim
  with its defaults (11-tap Gaussian window, sigma 1.5, K = (0.01, 0.03), valid
  windows, no clamp) as a detached device scalar, or the per-image [B] tensor
  with `size_average=False`; no host synchronisation. `ssim_loss(output,
  target, data_range=1.0)` is 1 - ssim, differentiable wrt `output`.
* The reference asserts `output.min() >= 0 and output.max() <= 1`
  (customLoss.py:131) with a host sync per call. Here a range-check kernel
  sets a sticky device flag that is copied to pinned host memory
  asynchronously; the next call raises the same AssertionError once that copy
  has landed (at most one step late, never a sync), and `check_range()`
  checks it immediately (synchronising).
* `PerturbationLoss(perturbation_count=3)`: pert_loss.py:7-90 — three
  no-grad forwards of the model on inputs perturbed by per-channel
  std * 0.01 Gaussian noise, mean L1 to the original output. `noise="device"`
  (opt-in; the default "torch" is that path unchanged) writes all variants
  with one nsm_perturb_variants launch that draws the noise inside the kernel
  (seeded from torch's CPU generator, or inside a graph capture from a device
  word of torch's graph-safe generator: new noise every replay).
* `EnhancedCustomLoss(device, alpha=0.9, perturb_weight=0.5)`: the wired
  perturbation-training loss of pert_loss.py:92-163 (§8f next-row #4). The
  reference's class cannot be constructed (it imports a `VGGLoss` that
  customLoss.py does not define); this one uses the `MultiLayerVGGLoss`
  CustomLoss uses and otherwise follows the reference: returns
  (total, {'l1_loss', 'vgg_loss', 'perturbation_loss', 'total_loss'}),
  total = alpha*L1 + (1-alpha)*vgg [+ perturb_weight*perturbation while
  training]. `detail_weight` / `gradient_weight` as in CustomLoss: when one
  is non-zero the detail terms join `total` and the dict gains
  'high_freq_loss', 'penumbra_loss' and 'gradient_loss' (device scalars).
  `ssim_weight` / `ssim_data_range` as in CustomLoss: with the weight on the
  term joins `total` and the dict gains 'ssim_loss' = 1 - ssim (device scalar).
  `fused=True` (opt-in; with `noise=`, `seed=`, `perturbation_count=` handed to
  its PerturbationLoss): while training with a perturbation weight the L1 node
  and the P perturbation nodes are ONE node on nsm_pert_loss_fwd/bwd; `total`
  is the kernel's alpha*l1 + (1-alpha)*vgg + perturb_weight*pert, the parts in
  the dict are detached views of its record (no 0-dim ATen arithmetic, no host
  sync), and the perturbed forwards keep the main forward's prepared weight
  layouts (unet.reuse_prepared_weights). `set_noises(t)` injects noises into
  every following call. GraphedTrainStep takes the criterion as main.py:265
  calls it ("The perturbation-loss step").
* `measure_temporal_instability(frames, motion_vectors=None, alpha=5.0)`:
  pert_loss.py:166-199, mean over consecutive frame pairs of
  mean(exp(alpha*|f_t - f_{t-1}|) - 1) (`nsm_expdiff_mean`). With
  `motion_vectors` each pixel is compared with its reprojected position in the
  previous frame (the paper's Eq. 3; the reference's branch is a stub that
  raises), with optional depth / normal rejection: nsm_amd/temporal.py, which
  also has `temporal_instability_terms`, `reproject` and the streaming
  `TemporalInstability`; all four are re-exported here.
"""
import ctypes
import os
import warnings

import torch
import torch.nn as nn

from ._lib import call, lib, ptr, require_gpu, stream
from .temporal import (TemporalInstability, measure_temporal_instability,  # noqa: F401
                       reproject, temporal_instability_terms)

VGG19_FILE = "vgg19-dcbb9e9d.pth"   # torchvision IMAGENET1K_V1 (customLoss.py:20)
_VGG_WARNED = []


def find_vgg19_checkpoint():
    """A locally cached torchvision VGG19 ImageNet checkpoint, or None."""
    env = os.environ.get("NSM_VGG19_WEIGHTS")
    cands = [env] if env else []
    try:
        cands.append(os.path.join(torch.hub.get_dir(), "checkpoints", VGG19_FILE))
    except Exception:  # noqa: BLE001  (hub dir unresolvable: no cache)
        pass
    for c in cands:
        if c and os.path.isfile(c):
            return c
    return None


class _RangeCheck:
    """Sticky device flag for `assert 0 <= output <= 1` (customLoss.py:131,
    pert_loss.py:131) without a host synchronisation."""

    def __init__(self, what):
        self.what = what
        self.flag = None
        self.host = None
        self.event = None

    def _raise_if_set(self):
        if self.host is not None and int(self.host[0]) != 0:
            self.host[0] = 0
            self.flag.zero_()
            raise AssertionError(f"{self.what}: output must be in [0, 1] (sigmoid output), "
                                 "customLoss.py:131")

    def prepare(self, device):
        """Allocate the flag, its pinned host copy and the event on `device`
        (outside any graph capture: a capture would record the flag's zeroing
        into every replay, which would make it non-sticky)."""
        if self.flag is None or self.flag.device != torch.device(device):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self.what}: the range flag must be allocated before graph "
                                   "capture (call prepare_capture(device) first)")
            self.flag = torch.zeros(1, dtype=torch.int32, device=device)
            self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
            self.event = torch.cuda.Event()

    def launch(self, o):
        self.prepare(o.device)
        if torch.cuda.is_current_stream_capturing():
            # a captured step (GraphedTrainStep): the sticky device flag only —
            # no event, no copy; check() reads the flag itself
            call("nsm_range_flag", ptr(o), o.numel(), 0.0, 1.0, ptr(self.flag), stream())
            self.captured = True
            return
        if self.event.query():
            self._raise_if_set()
        # eager: the kernel stores the sticky 1 straight into the pinned host
        # word (mapped into the device's address space; it only ever writes 1),
        # so no device-to-host copy is queued; the event orders the host's read
        call("nsm_range_flag", ptr(o), o.numel(), 0.0, 1.0, ptr(self.host), stream())
        self.event.record()

    def check(self):
        if getattr(self, "captured", False):
            torch.cuda.current_stream().synchronize()
            self.host.copy_(self.flag)
            self._raise_if_set()
        elif self.event is not None:
            self.event.synchronize()
            self._raise_if_set()


class _L1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, o, t, alpha):
        require_gpu(o, "L1 input")
        o_ = o.detach().contiguous().to(torch.float32)
        t_ = t.detach().contiguous().to(device=o.device, dtype=torch.float32)
        n = o_.numel()
        if t_.numel() != n:
            raise ValueError(f"l1: shape mismatch {tuple(o.shape)} vs {tuple(t.shape)}")
        nb = lib.nsm_loss_blocks(n)
        partial = torch.empty(nb, dtype=torch.float32, device=o.device)
        out = torch.empty((), dtype=torch.float32, device=o.device)
        call("nsm_l1_loss_fwd", ptr(o_), ptr(t_), n, float(alpha), ptr(partial), ptr(out), stream())
        ctx.save_for_backward(o_, t_)
        ctx.alpha = float(alpha)
        ctx.oshape = o.shape
        return out

    @staticmethod
    def backward(ctx, g):
        o_, t_ = ctx.saved_tensors
        grad = torch.empty_like(o_)
        g_ = g.detach().contiguous().to(torch.float32)
        call("nsm_l1_loss_bwd", ptr(o_), ptr(t_), o_.numel(), ctx.alpha, ptr(g_), ptr(grad), 0,
             stream())
        return grad.view(ctx.oshape), None, None


def l1_loss(output, target, alpha=1.0):
    return _L1Fn.apply(output, target, alpha)


class _CustomVggFn(torch.autograd.Function):
    """CustomLoss(vgg_grad=True): alpha*L1 + (1-alpha)*VGG as ONE node with one
    gradient tensor: the VGG backward chain writes (1-alpha) * dVGG/do, then
    nsm_l1_loss_bwd accumulates alpha*sign(o-t)/N into the same buffer."""

    @staticmethod
    def forward(ctx, o, t, alpha, vgg):
        from . import ops
        o_, t_ = vgg._inputs(o, t)
        n = o_.numel()
        partial = torch.empty(lib.nsm_loss_blocks(n), dtype=torch.float32, device=o_.device)
        out = torch.empty((), dtype=torch.float32, device=o_.device)
        call("nsm_l1_loss_fwd", ptr(o_), ptr(t_), n, float(alpha), ptr(partial), ptr(out), stream())
        with ops.stage("vgg.fwd"):
            v, saved = vgg._forward(o_, t_, keep=True)
        ctx.save_for_backward(o_, t_)
        ctx.vgg, ctx.acts = vgg, saved
        ctx.alpha, ctx.oshape = float(alpha), o.shape
        return out + (1 - alpha) * v     # the arithmetic of the detached default

    @staticmethod
    def backward(ctx, g):
        from . import ops
        o_, t_ = ctx.saved_tensors
        grad = torch.empty_like(o_)
        g_ = g.detach().contiguous().to(torch.float32)
        with ops.stage("vgg.bwd"):
            ctx.vgg._backward(ctx.acts, o_, g_, grad, scale=1 - ctx.alpha)
        call("nsm_l1_loss_bwd", ptr(o_), ptr(t_), o_.numel(), ctx.alpha, ptr(g_), ptr(grad), 1,
             stream())
        return grad.view(ctx.oshape), None, None, None


def _detail_inputs(o, t):
    """[B,1,H,W] fp32 contiguous output and target, as _L1Fn converts them."""
    require_gpu(o, "detail-term input")
    if o.dim() != 4 or o.shape[1] != 1:
        raise ValueError(f"detail terms: expected a [B,1,H,W] output, got {tuple(o.shape)} (the "
                         "reference's channel-mean branch, customLoss.py:119, is not supported)")
    o_ = o.detach().contiguous().to(torch.float32)
    t_ = t.detach().contiguous().to(device=o.device, dtype=torch.float32)
    if t_.shape != o_.shape:
        raise ValueError(f"detail terms: shape mismatch {tuple(o.shape)} vs {tuple(t.shape)}")
    return o_, t_


def _detail_fwd(o_, t_, w_hf, w_pen, w_sob, base=None):
    """The fused forward: a device vector (HF, PEN, SOB, M, base + weighted sum)."""
    B, _, H, W = o_.shape
    nb = lib.nsm_detail_blocks(B, H, W)
    if nb <= 0:
        raise ValueError(f"detail terms: unsupported shape {tuple(o_.shape)}")
    partial = torch.empty(4 * nb, dtype=torch.float32, device=o_.device)
    vec = torch.empty(5, dtype=torch.float32, device=o_.device)
    call("nsm_detail_loss_fwd", ptr(o_), ptr(t_), B, H, W, w_hf, w_pen, w_sob, ptr(base),
         ptr(partial), ptr(vec), stream())
    return vec


def _detail_bwd(o_, t_, w, vec, g_, grad, accumulate):
    B, _, H, W = o_.shape
    call("nsm_detail_loss_bwd", ptr(o_), ptr(t_), B, H, W, w[0], w[1], w[2],
         vec.data_ptr() + 3 * vec.element_size(), ptr(g_), ptr(grad), int(accumulate), stream())


class _DetailFn(torch.autograd.Function):
    """w_hf*HF + w_pen*PEN + w_sob*SOB (customLoss.py:139-185) as one node;
    also returns the three terms (detached)."""

    @staticmethod
    def forward(ctx, o, t, w_hf, w_pen, w_sob):
        o_, t_ = _detail_inputs(o, t)
        ctx.w = (float(w_hf), float(w_pen), float(w_sob))
        vec = _detail_fwd(o_, t_, *ctx.w)
        ctx.save_for_backward(o_, t_, vec)
        ctx.oshape = o.shape
        terms = (vec[0], vec[1], vec[2])
        ctx.mark_non_differentiable(*terms)
        ctx.set_materialize_grads(False)   # no zero-filled gradients for the three terms
        return (vec[4],) + terms

    @staticmethod
    def backward(ctx, g, *unused):
        o_, t_, vec = ctx.saved_tensors
        grad = torch.empty_like(o_)
        g_ = g.detach().contiguous().to(torch.float32)
        _detail_bwd(o_, t_, ctx.w, vec, g_, grad, False)
        return grad.view(ctx.oshape), None, None, None, None


def detail_loss(output, target, hf_weight=0.0, penumbra_weight=0.0, sobel_weight=0.0):
    """hf_weight*HF + penumbra_weight*PEN + sobel_weight*SOB, differentiable
    wrt `output` on the fused kernels."""
    return _DetailFn.apply(output, target, hf_weight, penumbra_weight, sobel_weight)[0]


def detail_terms(output, target):
    """(high_freq_loss, penumbra_loss, gradient_loss) of customLoss.py:139-181
    as detached device scalars, without a host synchronisation."""
    o_, t_ = _detail_inputs(output, target)
    vec = _detail_fwd(o_, t_, 0.0, 0.0, 0.0)
    return vec[0], vec[1], vec[2]


class _CustomDetailFn(torch.autograd.Function):
    """CustomLoss with a detail weight: base + detail_weight*(HF + PEN) +
    gradient_weight*SOB as ONE node with one gradient tensor. base is
    alpha*L1 + (1-alpha)*VGG; the VGG term is `vgg` (nsm_amd's stack, carrying
    its gradient: vgg_grad=True), or the detached value `vgg_value`, or absent.
    Backward: the VGG chain (if any), then nsm_l1_loss_bwd, then
    nsm_detail_loss_bwd accumulate into the same buffer."""

    @staticmethod
    def forward(ctx, o, t, alpha, vgg, vgg_value, detail_weight, gradient_weight):
        from . import ops
        o_, t_ = _detail_inputs(o, t)
        n = o_.numel()
        partial = torch.empty(lib.nsm_loss_blocks(n), dtype=torch.float32, device=o_.device)
        base = torch.empty((), dtype=torch.float32, device=o_.device)
        call("nsm_l1_loss_fwd", ptr(o_), ptr(t_), n, float(alpha), ptr(partial), ptr(base),
             stream())
        ctx.acts = None
        if vgg is not None:
            with ops.stage("vgg.fwd"):
                v, ctx.acts = vgg._forward(o_, t_, keep=True)
            base = base + (1 - alpha) * v            # the arithmetic of _CustomVggFn
        elif vgg_value is not None:
            base = base + (1 - alpha) * vgg_value    # the arithmetic of the detached default
        ctx.w = (float(detail_weight), float(detail_weight), float(gradient_weight))
        vec = _detail_fwd(o_, t_, *ctx.w, base=base)
        ctx.save_for_backward(o_, t_, vec)
        ctx.vgg, ctx.alpha, ctx.oshape = vgg, float(alpha), o.shape
        terms = (vec[0], vec[1], vec[2])
        ctx.mark_non_differentiable(*terms)
        ctx.set_materialize_grads(False)   # no zero-filled gradients for the three terms
        return (vec[4],) + terms

    @staticmethod
    def backward(ctx, g, *unused):
        from . import ops
        o_, t_, vec = ctx.saved_tensors
        grad = torch.empty_like(o_)
        g_ = g.detach().contiguous().to(torch.float32)
        if ctx.vgg is not None:
            with ops.stage("vgg.bwd"):
                ctx.vgg._backward(ctx.acts, o_, g_, grad, scale=1 - ctx.alpha)
        call("nsm_l1_loss_bwd", ptr(o_), ptr(t_), o_.numel(), ctx.alpha, ptr(g_), ptr(grad),
             1 if ctx.vgg is not None else 0, stream())
        _detail_bwd(o_, t_, ctx.w, vec, g_, grad, True)
        return grad.view(ctx.oshape), None, None, None, None, None, None


def _ssim_inputs(o, t):
    """[B,1,H,W] fp32 contiguous output and target, H and W at least the window."""
    require_gpu(o, "ssim input")
    if o.dim() != 4 or o.shape[1] != 1:
        raise ValueError(f"ssim: expected a [B,1,H,W] output, got {tuple(o.shape)}")
    if tuple(t.shape) != tuple(o.shape):
        raise ValueError(f"ssim: shape mismatch {tuple(o.shape)} vs {tuple(t.shape)}")
    if o.shape[2] < 11 or o.shape[3] < 11:
        raise ValueError(f"ssim: H and W must be at least the 11-pixel window, got "
                         f"{tuple(o.shape)}")
    o_ = o.detach().contiguous().to(torch.float32)
    t_ = t.detach().contiguous().to(device=o.device, dtype=torch.float32)
    return o_, t_


def _ssim_fwd(o_, t_, data_range, w=0.0, base=None, keep=False):
    """The fused forward: a device vector (ssim, 1 - ssim, base + w*(1 - ssim),
    ssim of each image) and, with `keep`, the coefficient planes of the backward."""
    B, _, H, W = o_.shape
    nb = lib.nsm_ssim_blocks(B, H, W)
    if nb <= 0 or not data_range > 0:
        raise ValueError(f"ssim: unsupported shape {tuple(o_.shape)} or data_range {data_range}")
    partial = torch.empty(nb, dtype=torch.float32, device=o_.device)
    vec = torch.empty(3 + B, dtype=torch.float32, device=o_.device)
    coef = (torch.empty(3 * B * (H - 10) * (W - 10), dtype=torch.float32, device=o_.device)
            if keep else None)
    call("nsm_ssim_fwd", ptr(o_), ptr(t_), B, H, W, float(data_range), float(w), ptr(base),
         ptr(partial), ptr(coef), ptr(vec), stream())
    return vec, coef


def _ssim_bwd(o_, t_, coef, w, g_, grad, accumulate):
    B, _, H, W = o_.shape
    call("nsm_ssim_bwd", ptr(o_), ptr(t_), ptr(coef), B, H, W, float(w), ptr(g_), ptr(grad),
         int(accumulate), stream())


def ssim(output, target, data_range=1.0, size_average=True):
    """pytorch_msssim.ssim(output, target, data_range) with its other defaults
    on [B,1,H,W] images, as a detached device scalar ([B] per-image values with
    size_average=False), without a host synchronisation. `data_range` defaults
    to 1.0 (sigmoid outputs), not to pytorch_msssim's 255."""
    o_, t_ = _ssim_inputs(output, target)
    vec, _ = _ssim_fwd(o_, t_, data_range)
    return vec[0] if size_average else vec[3:]


class _SsimFn(torch.autograd.Function):
    """weight * (1 - ssim) as one node; also returns 1 - ssim (detached)."""

    @staticmethod
    def forward(ctx, o, t, weight, data_range):
        o_, t_ = _ssim_inputs(o, t)
        ctx.w = float(weight)
        vec, coef = _ssim_fwd(o_, t_, data_range, ctx.w, keep=True)
        ctx.save_for_backward(o_, t_, coef)
        ctx.oshape = o.shape
        ctx.set_materialize_grads(False)   # no zero-filled gradient for the term
        term = vec[1]
        ctx.mark_non_differentiable(term)
        return vec[2], term

    @staticmethod
    def backward(ctx, g, *unused):
        o_, t_, coef = ctx.saved_tensors
        grad = torch.empty_like(o_)
        g_ = g.detach().contiguous().to(torch.float32)
        _ssim_bwd(o_, t_, coef, ctx.w, g_, grad, False)
        return grad.view(ctx.oshape), None, None, None


def ssim_loss(output, target, data_range=1.0):
    """1 - ssim(output, target, data_range), differentiable wrt `output` on the
    fused kernels (the term of customLoss.py:187-191)."""
    return _SsimFn.apply(output, target, 1.0, data_range)[0]


class _CustomSsimFn(torch.autograd.Function):
    """CustomLoss with an SSIM weight: enhanced + ssim_weight*(1 - ssim)
    (customLoss.py:187-191) as ONE node with one gradient tensor. enhanced is
    _CustomDetailFn's value (base when both detail weights are 0). Backward:
    the VGG chain (if any), nsm_l1_loss_bwd, nsm_detail_loss_bwd (if on), then
    nsm_ssim_bwd accumulate into the same buffer."""

    @staticmethod
    def forward(ctx, o, t, alpha, vgg, vgg_value, detail_weight, gradient_weight, ssim_weight,
                data_range):
        from . import ops
        o_, t_ = _ssim_inputs(o, t)
        n = o_.numel()
        partial = torch.empty(lib.nsm_loss_blocks(n), dtype=torch.float32, device=o_.device)
        base = torch.empty((), dtype=torch.float32, device=o_.device)
        call("nsm_l1_loss_fwd", ptr(o_), ptr(t_), n, float(alpha), ptr(partial), ptr(base),
             stream())
        ctx.acts = None
        if vgg is not None:
            with ops.stage("vgg.fwd"):
                v, ctx.acts = vgg._forward(o_, t_, keep=True)
            base = base + (1 - alpha) * v            # the arithmetic of _CustomVggFn
        elif vgg_value is not None:
            base = base + (1 - alpha) * vgg_value    # the arithmetic of the detached default
        ctx.w = (float(detail_weight), float(detail_weight), float(gradient_weight))
        ctx.detail = detail_weight != 0.0 or gradient_weight != 0.0
        dvec = None
        if ctx.detail:
            dvec = _detail_fwd(o_, t_, *ctx.w, base=base)
            base = dvec[4]
        ctx.ws = float(ssim_weight)
        vec, coef = _ssim_fwd(o_, t_, data_range, ctx.ws, base=base, keep=True)
        ctx.save_for_backward(o_, t_, coef, dvec)
        ctx.vgg, ctx.alpha, ctx.oshape = vgg, float(alpha), o.shape
        term = vec[1]
        ctx.mark_non_differentiable(term)
        ctx.set_materialize_grads(False)
        return vec[2], term

    @staticmethod
    def backward(ctx, g, *unused):
        from . import ops
        o_, t_, coef, dvec = ctx.saved_tensors
        grad = torch.empty_like(o_)
        g_ = g.detach().contiguous().to(torch.float32)
        if ctx.vgg is not None:
            with ops.stage("vgg.bwd"):
                ctx.vgg._backward(ctx.acts, o_, g_, grad, scale=1 - ctx.alpha)
        call("nsm_l1_loss_bwd", ptr(o_), ptr(t_), o_.numel(), ctx.alpha, ptr(g_), ptr(grad),
             1 if ctx.vgg is not None else 0, stream())
        if ctx.detail:
            _detail_bwd(o_, t_, ctx.w, dvec, g_, grad, True)
        _ssim_bwd(o_, t_, coef, ctx.ws, g_, grad, True)
        return (grad.view(ctx.oshape),) + (None,) * 8


class L1Loss(nn.Module):
    def forward(self, output, target):
        return l1_loss(output, target)


class CustomLoss(nn.Module):
    def __init__(self, device=None, alpha=0.9, vgg=None, vgg_weights="auto", check_range=True,
                 vgg_grad=False, detail_weight=0.0, gradient_weight=0.0, ssim_weight=0.0,
                 ssim_data_range=1.0):
        super().__init__()
        self.alpha = alpha
        self.l1 = L1Loss()
        self.vgg_grad = bool(vgg_grad)
        self.detail_weight = float(detail_weight)
        self.gradient_weight = float(gradient_weight)
        self.ssim_weight = float(ssim_weight)
        self.ssim_data_range = float(ssim_data_range)
        if self.vgg_grad and vgg is not None:
            raise ValueError("CustomLoss(vgg_grad=True) differentiates nsm_amd's own VGG stack: "
                             "it cannot be combined with a user-supplied vgg=<callable>")
        if vgg is not None and isinstance(vgg_weights, str) and vgg_weights == "auto":
            vgg_weights = None           # an explicit vgg callable wins
        if vgg is None and isinstance(vgg_weights, str) and vgg_weights == "auto":
            vgg_weights = find_vgg19_checkpoint()
            if vgg_weights is None and not _VGG_WARNED and not self.vgg_grad:
                _VGG_WARNED.append(True)
                warnings.warn(
                    "nsm_amd.CustomLoss: no VGG19 ImageNet checkpoint found ($NSM_VGG19_WEIGHTS "
                    f"or torch.hub cache {VGG19_FILE}); the perceptual term (customLoss.py:137, "
                    "weight 1-alpha) is 0 — the loss VALUE differs from the reference's, its "
                    "gradient (alpha*sign/N) does not", RuntimeWarning, stacklevel=2)
        if vgg_weights is False:
            vgg_weights = None
        if vgg_weights is not None:
            from .vgg import MultiLayerVGGLoss
            if isinstance(vgg_weights, MultiLayerVGGLoss):
                self.vgg_loss = vgg_weights
            elif isinstance(vgg_weights, str) and vgg_weights == "random":
                self.vgg_loss = MultiLayerVGGLoss(device)
            elif isinstance(vgg_weights, str):
                self.vgg_loss = MultiLayerVGGLoss.from_torchvision_checkpoint(vgg_weights, device)
            else:
                self.vgg_loss = MultiLayerVGGLoss(device, state_dict=vgg_weights)
            vgg = self.vgg_loss
        elif self.vgg_grad:
            raise ValueError("CustomLoss(vgg_grad=True) needs VGG weights (a checkpoint, a "
                             "state_dict, a MultiLayerVGGLoss or \"random\"): without them the "
                             "perceptual term is off and has no gradient")
        self.vgg = vgg
        self.device = device
        self.check_range = check_range
        self._range = _RangeCheck("CustomLoss")

    def forward(self, output, target, inputs=None):
        if self.check_range:
            require_gpu(output, "CustomLoss output")
            self._range.launch(output.detach().contiguous().to(torch.float32))
        if self.ssim_weight != 0.0:
            v = None
            if not self.vgg_grad and self.vgg is not None:
                v = torch.as_tensor(self.vgg(output, target), device=output.device).detach()
            return _CustomSsimFn.apply(output, target, self.alpha,
                                       self.vgg_loss if self.vgg_grad else None, v,
                                       self.detail_weight, self.gradient_weight,
                                       self.ssim_weight, self.ssim_data_range)[0]
        if self.detail_weight != 0.0 or self.gradient_weight != 0.0:
            v = None
            if not self.vgg_grad and self.vgg is not None:
                v = torch.as_tensor(self.vgg(output, target), device=output.device).detach()
            return _CustomDetailFn.apply(output, target, self.alpha,
                                         self.vgg_loss if self.vgg_grad else None, v,
                                         self.detail_weight, self.gradient_weight)[0]
        if self.vgg_grad:
            return _CustomVggFn.apply(output, target, self.alpha, self.vgg_loss)
        loss = l1_loss(output, target, self.alpha)
        if self.vgg is not None:
            v = self.vgg(output, target)
            loss = loss + (1 - self.alpha) * torch.as_tensor(v, device=loss.device).detach()
        return loss

    def check_range_now(self):
        """Raise now (host sync) if any output seen so far left [0, 1]."""
        self._range.check()

    def prepare_capture(self, device):
        """Allocate the range assert's device state before a graph capture
        (GraphedTrainStep calls it)."""
        if self.check_range:
            self._range.prepare(device)


PERT_MAX = 8    # NSM_PERT_MAX (include/nsm.h): variants of one fused launch
_NOISE_SOURCES = ("torch", "device")


def _check_pert_options(what, perturbation_count, noise, fused=False):
    if noise not in _NOISE_SOURCES:
        raise ValueError(f"{what}: noise must be \"torch\" or \"device\", got {noise!r}")
    if int(perturbation_count) != perturbation_count or perturbation_count < 1:
        raise ValueError(f"{what}: perturbation_count must be a whole number >= 1, got "
                         f"{perturbation_count!r}")
    if (fused or noise == "device") and perturbation_count > PERT_MAX:
        raise ValueError(f"{what}: the fused kernels take at most {PERT_MAX} variants, got "
                         f"perturbation_count={perturbation_count}")


def _check_noises(noises, count, shape):
    """Injected noises: a list of `count` tensors shaped like the input, or one
    [count, *shape] tensor. Host checks only."""
    shape = tuple(shape)
    if isinstance(noises, torch.Tensor):
        if tuple(noises.shape) != (count,) + shape:
            raise ValueError(f"perturbation noises: expected a {(count,) + shape} tensor, got "
                             f"{tuple(noises.shape)}")
        return
    if len(noises) != count:
        raise ValueError(f"perturbation noises: expected {count} tensors, got {len(noises)}")
    for i, n in enumerate(noises):
        if tuple(n.shape) != shape:
            raise ValueError(f"perturbation noises: noise {i} has shape {tuple(n.shape)}, the "
                             f"input {shape}")


class _PertLossFn(torch.autograd.Function):
    """alpha*L1(o, t) + (1-alpha)*vgg + w * mean_i L1(o, p_i) as ONE node on
    nsm_pert_loss_fwd / nsm_pert_loss_bwd: one pass over o, t and the P
    perturbed outputs each way. Returns (total, l1, pert): views of the
    kernel's record, the last two detached. `vgg` is a detached device scalar
    (its value joins `total`, no gradient) or None."""

    @staticmethod
    def forward(ctx, o, t, alpha, w, vgg, *pouts):
        require_gpu(o, "perturbation-loss output")
        o_ = o.detach().contiguous().to(torch.float32)
        t_ = t.detach().contiguous().to(device=o.device, dtype=torch.float32)
        ps = [p.detach().contiguous().to(device=o.device, dtype=torch.float32) for p in pouts]
        n, P = o_.numel(), len(ps)
        if t_.numel() != n or any(p.numel() != n for p in ps):
            raise ValueError(f"perturbation loss: shape mismatch, output {tuple(o.shape)}, target "
                             f"{tuple(t.shape)}, perturbed {[tuple(p.shape) for p in pouts]}")
        nb = lib.nsm_pert_loss_blocks(n)
        if nb <= 0 or not 1 <= P <= PERT_MAX:
            raise ValueError(f"perturbation loss: {n} elements, {P} perturbed outputs")
        partial = torch.empty((1 + P) * nb, dtype=torch.float32, device=o.device)
        rec = torch.empty(3 + P, dtype=torch.float32, device=o.device)
        v_ = None if vgg is None else vgg.detach().to(device=o.device, dtype=torch.float32)
        ctx.table = (ctypes.c_void_p * P)(*[p.data_ptr() for p in ps])
        call("nsm_pert_loss_fwd", ptr(o_), ptr(t_), ctx.table, P, n, float(alpha), float(w),
             ptr(v_), ptr(partial), ptr(rec), stream())
        ctx.save_for_backward(o_, t_, *ps)
        ctx.alpha, ctx.w, ctx.oshape = float(alpha), float(w), o.shape
        l1, pert = rec[0], rec[1]
        ctx.mark_non_differentiable(l1, pert)
        ctx.set_materialize_grads(False)
        return rec[2], l1, pert

    @staticmethod
    def backward(ctx, g, *unused):
        o_, t_, *ps = ctx.saved_tensors
        grad = torch.empty_like(o_)
        g_ = g.detach().contiguous().to(torch.float32)
        call("nsm_pert_loss_bwd", ptr(o_), ptr(t_), ctx.table, len(ps), o_.numel(), ctx.alpha,
             ctx.w, ptr(g_), ptr(grad), 0, stream())
        return (grad.view(ctx.oshape),) + (None,) * (4 + len(ps))


class PerturbationLoss(nn.Module):
    """pert_loss.py:7-90. `noise` selects where the Gaussian noise comes from:
    "torch" (default): one torch.randn_like and one nsm_perturb launch per
    variant, the reference's random stream; "device": nsm_channel_std, then ONE
    nsm_perturb_variants launch that writes all variants (views of one buffer)
    and draws the noise inside the kernel from a counter-based generator. Its
    seed is a host value from torch's CPU generator (so torch.manual_seed
    reproduces it; `seed=<int>` gives the loss a generator of its own instead),
    or, inside a graph capture, a device word from torch's graph-safe generator,
    so every replay draws new noise. Injected `noises` (a list, or one
    [P,B,C,H,W] tensor) go through the same kernel."""

    def __init__(self, perturbation_count=3, alpha=0.9, std_factor=0.01, noise="torch", seed=None):
        super().__init__()
        _check_pert_options("PerturbationLoss", perturbation_count, noise)
        if seed is not None and noise != "device":
            raise ValueError("PerturbationLoss: seed applies to noise=\"device\" only "
                             "(noise=\"torch\" follows torch's generators)")
        self.perturbation_count = perturbation_count
        self.alpha = alpha
        self.std_factor = std_factor
        self.noise = noise
        self._gen = None if seed is None else torch.Generator().manual_seed(int(seed))
        self.loss_fn = L1Loss()

    def _variants(self, x_, noises):
        """noise="device": all variants from one nsm_perturb_variants launch."""
        B, C, H, W = x_.shape
        P = int(self.perturbation_count)
        std = torch.empty(C, dtype=torch.float32, device=x_.device)
        call("nsm_channel_std", ptr(x_), B, C, H, W, None, ptr(std), stream())
        out = torch.empty((P,) + tuple(x_.shape), dtype=torch.float32, device=x_.device)
        z, seed, seed_t = None, 0, None
        if noises is not None:
            if not isinstance(noises, torch.Tensor):
                noises = torch.stack([n.to(device=x_.device, dtype=torch.float32)
                                      for n in noises])
            z = noises.to(device=x_.device, dtype=torch.float32).contiguous()
        elif torch.cuda.is_current_stream_capturing():
            # a captured step: the seed is device state, rewritten by every replay
            seed_t = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=x_.device)
        else:
            seed = int(torch.randint(0, 2 ** 62, (1,), generator=self._gen).item())
        call("nsm_perturb_variants", ptr(x_), ptr(std), ptr(z), seed, ptr(seed_t), P, B, C, H, W,
             self.std_factor, ptr(out), stream())
        return list(out.unbind(0))

    def perturb_input(self, x, noises=None):
        """Per-channel unbiased std over the batch, then x + n*std*0.01
        (pert_loss.py:26-59); `noises` (list of tensors shaped like x, or one
        stacked tensor) may be supplied for parity, else drawn from torch.randn
        (noise="torch") or inside the kernel (noise="device")."""
        if noises is not None:
            _check_noises(noises, int(self.perturbation_count), x.shape)
        require_gpu(x, "perturbation input")
        x_ = x.detach().contiguous().to(torch.float32)
        if self.noise == "device":
            return self._variants(x_, noises)
        B, C, H, W = x_.shape
        std = torch.empty(C, dtype=torch.float32, device=x.device)
        call("nsm_channel_std", ptr(x_), B, C, H, W, None, ptr(std), stream())
        outs = []
        for i in range(self.perturbation_count):
            n = noises[i] if noises is not None else torch.randn_like(x_)
            n = n.to(device=x.device, dtype=torch.float32).contiguous()
            o = torch.empty_like(x_)
            call("nsm_perturb", ptr(x_), ptr(n), ptr(std), B, C, H, W, self.std_factor, ptr(o),
                 stream())
            outs.append(o)
        return outs

    def forward(self, model, original_input, original_output, noises=None):
        pins = self.perturb_input(original_input, noises)
        with torch.no_grad():
            pouts = [model(p) for p in pins]
        total = 0
        for po in pouts:
            total = total + l1_loss(original_output, po)
        return total / len(pouts)


class EnhancedCustomLoss(nn.Module):
    def __init__(self, device=None, alpha=0.9, perturb_weight=0.5, vgg=None, vgg_weights="auto",
                 vgg_grad=False, detail_weight=0.0, gradient_weight=0.0, ssim_weight=0.0,
                 ssim_data_range=1.0, fused=False, noise="torch", seed=None,
                 perturbation_count=3):
        super().__init__()
        _check_pert_options("EnhancedCustomLoss", perturbation_count, noise, fused)
        self.fused = bool(fused)
        self._noises = None
        self._zero = {}
        self.alpha = alpha
        self.perturb_weight = perturb_weight
        self.l1 = L1Loss()
        self.vgg_grad = bool(vgg_grad)
        self.detail_weight = float(detail_weight)
        self.gradient_weight = float(gradient_weight)
        self.ssim_weight = float(ssim_weight)
        self.ssim_data_range = float(ssim_data_range)
        self.base = CustomLoss(device, alpha, vgg=vgg, vgg_weights=vgg_weights, vgg_grad=vgg_grad,
                               detail_weight=detail_weight, gradient_weight=gradient_weight,
                               ssim_weight=ssim_weight, ssim_data_range=ssim_data_range)
        self.vgg_loss = getattr(self.base, "vgg_loss", None) or vgg
        self.perturbation_loss = PerturbationLoss(perturbation_count=perturbation_count,
                                                  noise=noise, seed=seed)

    def prepare_capture(self, device):
        self.base._range.prepare(device)

    def check_range_now(self):
        self.base._range.check()

    def set_noises(self, noises):
        """Use `noises` (a list of perturbation_count tensors shaped like the
        input, or one [P,B,C,H,W] tensor) instead of drawn noise on every
        following call, until set_noises(None). The tensors are read, never
        copied, so a captured step (GraphedTrainStep) reads whatever they hold
        at each replay. A parity hook, as `forward(..., noises=)`."""
        if noises is not None:
            P = int(self.perturbation_loss.perturbation_count)
            first = noises[0] if len(noises) else None
            if first is None:
                raise ValueError(f"perturbation noises: expected {P} tensors, got 0")
            _check_noises(noises, P, first.shape)
        self._noises = noises

    def _fused_forward(self, model, output, target, inputs, noises):
        """fused=True while training with a perturbation weight: the L1 node and
        the P perturbation nodes as one _PertLossFn; the other terms beside it."""
        if self.vgg_grad:
            from .vgg import _VggFn
            vgg = _VggFn.apply(output, target, self.vgg_loss)
        elif self.vgg_loss is not None:
            vgg = torch.as_tensor(self.vgg_loss(output, target), device=output.device).detach()
        else:
            vgg = None
        pins = self.perturbation_loss.perturb_input(inputs, noises)
        # the weights are those of the forward that produced `output`: the
        # perturbed forwards keep its prepared layouts (bitwise the same results)
        from .unet import reuse_prepared_weights
        # (an extract.ExtractedUnet prepares its U-Net's layouts: the key is that module)
        with torch.no_grad(), reuse_prepared_weights(getattr(model, "unet", model)):
            pouts = [model(p) for p in pins]
        # a differentiated VGG term stays its own node: its value joins below
        total, l1, pert = _PertLossFn.apply(output, target, self.alpha, self.perturb_weight,
                                            None if self.vgg_grad else vgg, *pouts)
        if vgg is None:
            vgg = self._zero.get(output.device)
            if vgg is None:   # one fill per device, not one per step
                vgg = self._zero[output.device] = torch.zeros((), device=output.device)
        losses = {"l1_loss": l1, "vgg_loss": vgg.detach()}
        if self.vgg_grad:
            losses["vgg_loss"] = vgg
            total = total + (1 - self.alpha) * vgg
        if self.detail_weight != 0.0 or self.gradient_weight != 0.0:
            d, hf, pen, sob = _DetailFn.apply(output, target, self.detail_weight,
                                              self.detail_weight, self.gradient_weight)
            total = total + d
            losses.update(high_freq_loss=hf, penumbra_loss=pen, gradient_loss=sob)
        if self.ssim_weight != 0.0:
            s, term = _SsimFn.apply(output, target, self.ssim_weight, self.ssim_data_range)
            total = total + s
            losses["ssim_loss"] = term
        losses["perturbation_loss"] = pert
        losses["total_loss"] = total
        return total, losses

    def forward(self, model, output, target, inputs, noises=None):
        # pert_loss.py:131: the same [0, 1] assertion, as CustomLoss's device flag
        if noises is None:
            noises = self._noises
        if noises is not None and self.training and self.perturb_weight > 0:
            _check_noises(noises, int(self.perturbation_loss.perturbation_count), inputs.shape)
        require_gpu(output, "EnhancedCustomLoss output")
        self.base._range.launch(output.detach().contiguous().to(torch.float32))
        if self.fused and self.training and self.perturb_weight > 0:
            return self._fused_forward(model, output, target, inputs, noises)
        l1 = l1_loss(output, target)
        if self.vgg_grad:
            # the same value, carrying d vgg / d output (autograd adds it to the
            # L1 node's gradient: the returned losses stay separate tensors)
            from .vgg import _VggFn
            vgg = _VggFn.apply(output, target, self.vgg_loss)
        elif self.vgg_loss is not None:
            vgg = torch.as_tensor(self.vgg_loss(output, target), device=l1.device).detach()
        else:
            vgg = torch.zeros((), device=l1.device)
        # d(alpha*l1)/do reaches the L1 backward as gscale = alpha: alpha*sign/N
        basic = self.alpha * l1 + (1 - self.alpha) * vgg
        losses = {"l1_loss": l1, "vgg_loss": vgg}
        if self.detail_weight != 0.0 or self.gradient_weight != 0.0:
            # customLoss.py:161 + 185, the fused node beside the L1 one
            d, hf, pen, sob = _DetailFn.apply(output, target, self.detail_weight,
                                              self.detail_weight, self.gradient_weight)
            basic = basic + d
            losses.update(high_freq_loss=hf, penumbra_loss=pen, gradient_loss=sob)
        if self.ssim_weight != 0.0:
            # customLoss.py:187-191, its own node beside the L1 one
            s, term = _SsimFn.apply(output, target, self.ssim_weight, self.ssim_data_range)
            basic = basic + s
            losses["ssim_loss"] = term
        if self.training and self.perturb_weight > 0:
            pert = self.perturbation_loss(model, inputs, output, noises=noises)
            total = basic + self.perturb_weight * pert
            losses["perturbation_loss"] = pert
        else:
            total = basic
            losses["perturbation_loss"] = torch.zeros((), device=l1.device)
        losses["total_loss"] = total
        return total, losses
