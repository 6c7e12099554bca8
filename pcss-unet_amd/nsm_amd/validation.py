"""The validation pass: the other half of the reference's epoch
(`validate_direct`, main.py:583-664, called at main.py:514-545), and the image
error the paper reports its results in (Table 1 and §3.5: MSE against the
reference image; validate_consistency.py:119-120: MSE and PSNR).

    val = Validator(model, criterion, x0, y0)      # captured once, any model mode
    for x, y in val_loader:
        val.update(x.to(dev), y.to(dev))           # one graph launch, no host sync
    res = val.compute()                            # the only synchronisation
    scheduler.step(res)                            # float(res) is the mean total loss
    if res < best: ...
    res.metrics.mse, res.metrics.psnr              # over every image of the set

or `validate(model, val_loader, criterion)` for the whole of it.

Two launches (csrc/nsm_metrics.hip) follow the criterion inside the graph:
nsm_metrics_partial reads output and target once and writes one fp64 record
{count, sum|d|, sum d^2, max|d|, nonfinite, out_of_range} per block of every
image; nsm_metrics_merge folds them in a fixed order into the running record of
the set and, in the same launch, adds the criterion's device scalars and the
batch's L1 to an fp64 accumulator and writes the first `log_images` images'
records to a log. Nothing reads the device until compute().

`image_metrics(output, target)` and the streaming `ImageMetrics` give the same
figures for any pair of image batches.
"""
import contextlib
import ctypes
import math
from collections import namedtuple

import torch

from ._lib import call, lib, ptr, require_gpu, stream
from .infer import GraphedUnet

REC = 6            # doubles of a record: count, sum|d|, sum d^2, max|d|, nonfinite, out_of_range
MAX_SCALARS = 8    # NSM_METRICS_SCALARS (include/nsm.h)
_FIELDS = "count l1 mse psnr max_abs nonfinite out_of_range"


def psnr_of(mse):
    """validate_consistency.py:120: 20 * log10(1 / sqrt(mse)); inf at mse == 0."""
    if math.isnan(mse):
        return float("nan")
    return float("inf") if mse == 0 else 20.0 * math.log10(1.0 / math.sqrt(mse))


class MetricsResult(namedtuple("MetricsResult", _FIELDS + " per_image")):
    """Over every pair of finite samples: their `count`, `l1` = mean|d|, `mse` =
    mean d^2, `psnr` (validate_consistency.py:120; inf at mse == 0) and
    `max_abs` = max|d|, d = output - target in fp64; `nonfinite`: the pairs left
    out because either sample is NaN or +-Inf; `out_of_range`: the outputs of the
    counted pairs outside value_range. Python ints and floats; l1, mse and psnr
    are NaN at count == 0. `per_image`: None, or a PerImageMetrics of [B] tensors."""
    __slots__ = ()

    def __new__(cls, count, l1, mse, psnr, max_abs, nonfinite, out_of_range, per_image=None):
        return super().__new__(cls, count, l1, mse, psnr, max_abs, nonfinite, out_of_range,
                               per_image)


PerImageMetrics = namedtuple("PerImageMetrics", _FIELDS)
PerImageMetrics.__doc__ = """MetricsResult's figures of each image as [B] tensors:
count, nonfinite and out_of_range int64, the others fp64."""


def metrics_of(record, per_image=None):
    """MetricsResult of one record: 6 numbers {count, sum|d|, sum d^2, max|d|,
    nonfinite, out_of_range}. Host arithmetic only."""
    n, s1, s2, mx, bad, oor = (float(v) for v in record)
    nan = float("nan")
    l1, mse = (s1 / n, s2 / n) if n > 0 else (nan, nan)
    return MetricsResult(int(n), l1, mse, psnr_of(mse), mx, int(bad), int(oor), per_image)


def per_image_of(records):
    """PerImageMetrics of records [B, 6] (a per-image table or a Validator's log)."""
    n, s1, s2, mx, bad, oor = records.to(torch.float64).unbind(-1)
    l1, mse = s1 / n, s2 / n                 # 0 / 0: NaN at count == 0
    psnr = 20.0 * torch.log10(1.0 / torch.sqrt(mse))      # mse == 0: inf
    return PerImageMetrics(n.to(torch.int64), l1, mse, psnr, mx, bad.to(torch.int64),
                           oor.to(torch.int64))


def _check_range(value_range):
    try:
        lo, hi = (float(v) for v in value_range)
    except (TypeError, ValueError):
        raise ValueError(f"image metrics: value_range must be (lo, hi), got {value_range!r}") \
            from None
    if not lo <= hi:
        raise ValueError(f"image metrics: empty value_range ({lo}, {hi})")
    return lo, hi


def _pair(output, target, what="image metrics"):
    """Checks and casts: both [B,C,H,W] of one shape on one GPU -> fp32, contiguous."""
    for name, v in (("output", output), ("target", target)):
        if not torch.is_tensor(v) or v.dim() != 4:
            got = tuple(v.shape) if torch.is_tensor(v) else type(v).__name__
            raise ValueError(f"{what}: {name} must be a [B,C,H,W] tensor, got {got}")
    if output.shape != target.shape:
        raise ValueError(f"{what}: shape mismatch, output {tuple(output.shape)} and target "
                         f"{tuple(target.shape)}")
    if min(output.shape) < 1:
        raise ValueError(f"{what}: empty input {tuple(output.shape)}")
    require_gpu(output, f"{what} output")
    require_gpu(target, f"{what} target")
    if output.device != target.device:
        raise ValueError(f"{what}: output on {output.device}, target on {target.device}")
    n = output[0].numel()
    if lib.nsm_metrics_blocks(n) <= 0:
        raise ValueError(f"{what}: unsupported image size {tuple(output.shape[1:])}")
    o_ = output.detach().to(torch.float32).contiguous()
    t_ = target.detach().to(torch.float32).contiguous()
    return o_, t_, output.shape[0], n


def _launch(o_, t_, B, n, lo, hi, state, frames=None, scalars=(), acc=None, log=None):
    """nsm_metrics_partial + nsm_metrics_merge on the current stream."""
    per = lib.nsm_metrics_blocks(n)
    ws = torch.empty(B * per * REC, dtype=torch.float64, device=o_.device)
    call("nsm_metrics_partial", ptr(o_), ptr(t_), B, n, lo, hi, ptr(ws), stream())
    K = len(scalars)
    table = (ctypes.c_void_p * K)(*[s.data_ptr() for s in scalars]) if K else None
    cap = 0 if log is None else log.shape[0]
    call("nsm_metrics_merge", ptr(ws), B, per, table, K, ptr(frames), ptr(log), cap, ptr(state),
         ptr(acc), stream())


class ImageMetrics:
    """Running image-error figures: update(output, target) per batch, compute()
    for the MetricsResult so far, merge(other) for another accumulator's share
    (a second rank's shard), reset() to start over. The state is one fp64 record
    on the device; only compute() synchronises."""

    def __init__(self, value_range=(0.0, 1.0)):
        self.value_range = _check_range(value_range)
        self._state = None

    def _on(self, device):
        if self._state is None:
            self._state = torch.zeros(REC, dtype=torch.float64, device=device)
        elif self._state.device != device:
            raise ValueError(f"image metrics: the state lives on {self._state.device}, got a "
                             f"tensor on {device}")
        return self._state

    def reset(self):
        if self._state is not None:   # in place: a captured update keeps its pointer
            self._state.zero_()

    def update(self, output, target, per_image=False):
        """Fold a batch in. per_image=True returns the batch's own [B,6] fp64
        records (per_image_of reads them). No host synchronisation."""
        o_, t_, B, n = _pair(output, target)
        state = self._on(o_.device)
        frames = torch.empty((B, REC), dtype=torch.float64, device=o_.device) if per_image \
            else None
        _launch(o_, t_, B, n, *self.value_range, state, frames)
        return frames

    def merge(self, other):
        if not isinstance(other, ImageMetrics):
            raise ValueError(f"image metrics: cannot merge a {type(other).__name__}")
        if other._state is None:
            return self
        dev = other._state.device
        call("nsm_metrics_merge", ptr(other._state), 1, 1, None, 0, None, None, 0,
             ptr(self._on(dev)), None, stream())
        return self

    def compute(self):
        if self._state is None:
            raise RuntimeError("ImageMetrics.compute() before the first update()")
        return metrics_of(self._state.tolist())


def image_metrics(output, target, per_image=False, value_range=(0.0, 1.0)):
    """MetricsResult of output against target ([B,C,H,W] on the GPU; fp32, other
    dtypes are cast): one read of each. per_image=True fills `.per_image` with
    every image's figures as [B] device tensors. Reads the device once."""
    acc = ImageMetrics(value_range)
    frames = acc.update(output, target, per_image=per_image)
    if not per_image:
        return acc.compute()
    both = torch.cat([acc._state.unsqueeze(0), frames]).cpu()      # one wait
    return metrics_of(both[0].tolist(), per_image_of(frames))


class ValidationResult:
    """What validate_direct computes (main.py:624-642) and the image error of the
    set. `loss`: the mean over batches of the criterion's total — what
    validate_direct returns; float(result) is it, and results compare by it
    (`scheduler.step(result)`, `result < best`). `l1_loss`: the mean over batches
    of each batch's mean|output - target| (fp64, over the finite pairs).
    `parts`: the means over batches of the criterion's own parts
    ('l1_loss', 'vgg_loss', 'perturbation_loss', ... of EnhancedCustomLoss), also
    readable as attributes; `perturbation_loss` is 0.0 for a criterion without
    one, as in the reference. `batches`; `metrics`: a MetricsResult over all
    images; `per_image`: a PerImageMetrics of the logged images (CPU tensors), or
    None. Without a batch the losses are inf (main.py:641)."""

    def __init__(self, loss, l1_loss, parts, batches, metrics, per_image=None):
        self.loss, self.l1_loss, self.parts = float(loss), float(l1_loss), dict(parts)
        self.batches, self.metrics, self.per_image = int(batches), metrics, per_image
        self.parts.setdefault("perturbation_loss", 0.0)
        self.validator = None

    def __getattr__(self, name):          # the parts, as attributes
        parts = self.__dict__.get("parts", {})
        if name in parts:
            return parts[name]
        raise AttributeError(name)

    def __float__(self):
        return self.loss

    def __lt__(self, other):
        return self.loss < float(other)

    def __le__(self, other):
        return self.loss <= float(other)

    def __gt__(self, other):
        return self.loss > float(other)

    def __ge__(self, other):
        return self.loss >= float(other)

    def __repr__(self):
        return (f"ValidationResult(loss={self.loss!r}, l1_loss={self.l1_loss!r}, "
                f"parts={self.parts!r}, batches={self.batches}, metrics={self.metrics!r})")


def result_of(acc, state, names=(), log=None):
    """ValidationResult from the accumulators as numbers: acc = {batches, the
    total's sum, the named parts' sums, the batch L1s' sum, images seen}, state =
    the set's record, log = [k, 6] records or None. Host arithmetic only."""
    acc = [float(v) for v in acc]
    K = 1 + len(names)
    batches = int(acc[0])
    if batches > 0:
        mean = [v / batches for v in acc[1:2 + K]]       # main.py:641-642
    else:
        mean = [float("inf")] * (1 + K)
    parts = dict(zip(names, mean[1:K]))
    per_image = None
    if log is not None:
        log = torch.as_tensor(log, dtype=torch.float64).reshape(-1, REC)
        per_image = per_image_of(log[:min(int(acc[2 + K]), log.shape[0])])
    return ValidationResult(mean[0], mean[K], parts, batches, metrics_of(state), per_image)


class Validator(GraphedUnet):
    """One validation batch — eval forward, criterion, image metrics, the
    accumulators' update — captured in one graph; update(x, y) is one copy of
    each tensor and one graph launch, with no host synchronisation, and
    compute() reads the device once.

        val = Validator(model, criterion, example_x, example_y)
        val.update(x, y) ...; res = val.compute(); val.reset()

    The criterion is called as main.py:613-621 calls it: with a
    `perturbation_loss` attribute as `criterion(model, out, y, x)`, whose dict
    gives the parts; otherwise as `criterion(out, y, x)`. Its own train / eval
    mode stays as the caller set it (the reference's validate_direct leaves it
    too): a training-mode EnhancedCustomLoss with a perturbation weight runs its
    perturbed forwards and draws fresh noise in validation, as the reference's
    does; call `criterion.eval()` for the plain figure. `l1_loss` comes from the
    metrics pass (the reference's second `criterion.l1` read of both tensors is
    not made).

    A batch of another shape than the examples' (the last batch of a
    drop_last=False loader, the reference's setting) runs the same body eagerly,
    under the autocast state of the construction; graph=False runs every batch
    so. log_images=k keeps the records of the first k images of the set for
    `result.per_image`. value_range: the interval of `out_of_range`.

    The weights are handled as in GraphedUnet, whose capture this shares: frozen
    layouts, rewritten before a replay when a parameter's or buffer's version
    counter moved (training steps between two validations), and a RuntimeError
    when the parameters were re-allocated after the capture. Everything runs
    under no_grad; parameters, BN buffers and optimizer state are not touched,
    and the model's training flag is restored after construction and each call."""

    def __init__(self, model, criterion, example_x, example_y, graph=True, log_images=0,
                 value_range=(0.0, 1.0), static_weights=True, warmup=2):
        require_gpu(example_x, "Validator example input")
        require_gpu(example_y, "Validator example target")
        if isinstance(log_images, bool) or not isinstance(log_images, int) or log_images < 0:
            raise ValueError(f"Validator: log_images must be an integer >= 0, got {log_images!r}")
        self.value_range = _check_range(value_range)
        self.model, self.criterion = model, criterion
        self.has_pert = hasattr(criterion, "perturbation_loss")      # main.py:600
        dev = example_x.device
        self.shape, self.dtype = tuple(example_x.shape), example_x.dtype
        self.yshape = tuple(example_y.shape)
        self.static_in = example_x.detach().clone()
        self.static_y = example_y.detach().clone()
        self._autocast = (torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda"))
        self.names = None                 # the parts' names, from the first run of the body
        self._acc = torch.zeros(3 + MAX_SCALARS, dtype=torch.float64, device=dev)
        self._state = torch.zeros(REC, dtype=torch.float64, device=dev)
        self._log = torch.zeros((log_images, REC), dtype=torch.float64, device=dev) \
            if log_images else None
        if hasattr(criterion, "prepare_capture"):
            criterion.prepare_capture(dev)
        self.graph = self.frozen = None
        if graph:
            self._capture(model, warmup, static_weights)
            self.reset()                  # the warm-up runs and the capture counted batches

    def _run(self, x, y):
        out = self.model(x)
        if self.has_pert:                 # main.py:615-617
            total, parts = self.criterion(self.model, out, y, x)
            names = tuple(k for k in parts if k != "total_loss")
            scalars = [total] + [parts[k] for k in names]
        else:                             # main.py:620
            names, scalars = (), [self.criterion(out, y, x)]
        if len(scalars) > MAX_SCALARS:
            raise ValueError(f"Validator: the criterion returned {len(scalars) - 1} parts, at "
                             f"most {MAX_SCALARS - 1} are accumulated")
        if self.names is None:
            self.names = names
        elif names != self.names:
            raise ValueError(f"Validator: the criterion's parts changed from {self.names} to "
                             f"{names}")
        o_, t_, B, n = _pair(out, y, "Validator")
        scalars = [torch.as_tensor(s, device=o_.device).detach().to(torch.float32).reshape(())
                   for s in scalars]
        _launch(o_, t_, B, n, *self.value_range, self._state, None, scalars, self._acc, self._log)
        return out

    def _body(self):
        return self._run(self.static_in, self.static_y)

    def _eager(self, x, y):
        was = self.model.training
        self.model.eval()
        on, dtype = self._autocast
        ctx = torch.autocast("cuda", dtype=dtype) if on else contextlib.nullcontext()
        try:
            with torch.no_grad(), ctx:
                self._run(x, y)
        finally:
            self.model.train(was)

    def update(self, x, y):
        """One batch, on the device of the examples. No host synchronisation."""
        if self.graph is not None and tuple(x.shape) == self.shape \
                and tuple(y.shape) == self.yshape:
            self._check()
            self.static_in.copy_(x)
            self.static_y.copy_(y)
            self.graph.replay()
        else:
            self._eager(x, y)

    def reset(self):
        """Clear the accumulators, in place (the graph keeps their addresses)."""
        self._acc.zero_()
        self._state.zero_()
        if self._log is not None:
            self._log.zero_()

    def compute(self):
        """The ValidationResult of the batches since the last reset(); one wait."""
        tensors = [self._acc, self._state] + ([self._log.reshape(-1)] if self._log is not None
                                              else [])
        host = torch.cat(tensors).cpu()
        K = 1 + len(self.names or ())
        acc, state = host[:3 + K].tolist(), host[3 + MAX_SCALARS:3 + MAX_SCALARS + REC].tolist()
        log = host[3 + MAX_SCALARS + REC:] if self._log is not None else None
        res = result_of(acc, state, self.names or (), log)
        res.validator = self
        return res


def validate(model, loader, criterion, validator=None, device=None, **kw):
    """The whole of validate_direct (main.py:583-664) without its TensorBoard and
    logging: one pass over `loader` (batches of (inputs, labels)), moved to the
    model's device (or `device`), through `validator` or a Validator built from
    the first batch with **kw. Returns the ValidationResult; `.validator` is the
    Validator used: pass it back in at the next epoch to skip the capture."""
    if device is None:
        device = validator.static_in.device if validator is not None \
            else next(model.parameters()).device
    if validator is not None:
        validator.reset()
    for x, y in loader:
        x = x.to(device, non_blocking=True)
        y = y.to(device, non_blocking=True)
        if validator is None:
            validator = Validator(model, criterion, x, y, **kw)
        validator.update(x, y)
    if validator is None:                 # an empty loader: main.py:641
        return result_of([0.0] * 4, [0.0] * REC)
    return validator.compute()
