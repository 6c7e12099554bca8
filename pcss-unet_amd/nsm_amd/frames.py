"""The inference frame path: what the reference's inference.py wraps around
`model(x)` for every frame, on the device and inside the captured graph.

    raw frame -> reflect-pad to a multiple of 16 (inference.py:153-163)
              -> scrub NaN / +-Inf               (inference.py:170-173)
              -> [normalise, setdata.py:316: what a model trained through
                  FrameLoader needs, and what inference.py leaves out]
              -> eval forward
              -> scrub                            (inference.py:199-202)
              -> clip to [0,1], (v * 255) -> uint8, channels last
                 (save_output, inference.py:108-125; infer.py:79, main.py:457)

Two launches (csrc/nsm_frame.hip): `prepare_frames` is nsm_frame_prep,
`finish_frames` is nsm_frame_finish; each reads its source once and writes each
output once. Neither asks the host whether a NaN is there (the reference's
`isnan().any()` / `isinf().any()` each synchronise): the scrub is applied
unconditionally, which gives the same values, and the optional census counts
what it met into a device tensor that is read only when the caller asks.

    pipe = FramePipeline(model, example_raw_frames, stats=data_dir, crop=True)
    img = pipe(raw)              # uint8 [B,H,W] (or [B,H,W,C]): one copy, one graph launch
    frame = pipe.shadow          # the same frame, fp32 [B,C,H,W] in [0,1]
    pipe.report()                # {"nan": [...], ...} per image (synchronises)

The census `report` is an int32 [B,6] device tensor (`new_report`):
columns 0-2 the NaN, +Inf and -Inf among an image's raw samples (prepare_frames),
columns 3-5 the non-finite, the < 0 and the > 1 samples of the (cropped) network
output before the scrub and the clip (finish_frames); REPORT_KEYS names them.
"""
import os

import torch

from ._lib import call, lib, ptr, stream
from .data import MmapLiverDataset, _given_stats, load_stats
from .infer import GraphedUnet

REPORT_KEYS = ("nan", "posinf", "neginf", "out_nonfinite", "out_below_zero", "out_above_one")
_FINISH_CHANNELS = (1, 3, 4)   # save_output's cases (inference.py:111-128)


def new_report(batch, device):
    """A zeroed census tensor [batch, 6] int32 (see the module docstring)."""
    return torch.zeros((batch, 6), dtype=torch.int32, device=device)


def report_dict(report):
    """The census as {key: [count per image]} (REPORT_KEYS); reads the device."""
    cols = report.t().tolist()
    return dict(zip(REPORT_KEYS, cols))


def _frames_4d(x, what):
    """Host-side checks of a frame batch; [C,H,W] becomes [1,C,H,W]."""
    if not torch.is_tensor(x) or x.dim() not in (3, 4):
        got = tuple(x.shape) if torch.is_tensor(x) else type(x).__name__
        raise ValueError(f"{what} must be a [B,C,H,W] or [C,H,W] tensor, got {got}")
    if x.dtype != torch.float32:
        raise ValueError(f"{what} must be float32, got {x.dtype}")
    if not x.is_cuda:
        raise ValueError(f"{what} must be on a ROCm GPU device (got {x.device}); the frame path "
                         "has no CPU implementation")
    if min(x.shape) < 1:
        raise ValueError(f"{what} is empty: {tuple(x.shape)}")
    return x if x.dim() == 4 else x.unsqueeze(0)


def padded_size(H, W, pad_multiple=16):
    """(Hp, Wp): H and W rounded up to pad_multiple (inference.py:158-159);
    None or 1 keeps them. Raises ValueError where reflect padding cannot reach
    (the pad must be smaller than the dimension, as nn.ReflectionPad2d asks)."""
    if pad_multiple is None:
        return H, W
    if isinstance(pad_multiple, bool) or not isinstance(pad_multiple, int) or pad_multiple < 1:
        raise ValueError(f"pad_multiple must be an integer >= 1 or None, got {pad_multiple!r}")
    Hp, Wp = -(-H // pad_multiple) * pad_multiple, -(-W // pad_multiple) * pad_multiple
    for name, n, p in (("height", H, Hp), ("width", W, Wp)):
        if p - n >= n:
            raise ValueError(f"reflect padding the {name} {n} to {p} (a multiple of {pad_multiple}) "
                             f"needs a pad below the {name}, got {p - n}")
    return Hp, Wp


def _norm_of(stats, channels, device):
    """(means, stds) fp32 [C] on `device`, or None: what FrameLoader(stats=...)
    takes, or a directory holding train_stats.json."""
    if stats is None:
        return None
    if isinstance(stats, (str, os.PathLike)):
        st = load_stats(os.fspath(stats), None)
        if st is None:
            raise ValueError(f"no train_stats.json with means and stds under {os.fspath(stats)}")
        stats = st
    means, stds = _given_stats(stats, channels)
    return means.to(device).contiguous(), stds.to(device).contiguous()


def _check_buffer(t, shape, dtype, device, what):
    if (not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != dtype
            or t.device != device or not t.is_contiguous()):
        got = (tuple(t.shape), t.dtype, str(t.device)) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what} must be a contiguous {tuple(shape)} {dtype} tensor on {device}, "
                         f"got {got}")
    return t


def _census_ws(B, per, device):
    return torch.empty(B * per * 3, dtype=torch.int32, device=device)


def prepare_frames(x, *, pad_multiple=16, stats=None, scrub=True, eps=MmapLiverDataset.EPS,
                   out=None, report=None):
    """Raw frames x ([B,C,H,W] or [C,H,W], fp32, on the GPU) -> the network's
    input [B,C,Hp,Wp] fp32 in one pass: reflect-padded on the right and bottom
    to a multiple of `pad_multiple` (None or 1: no padding), scrubbed
    (scrub=True: NaN -> 0, +Inf -> 1, -Inf -> 0, padded copies too) and, with
    `stats`, normalised as the training loader does, bit for bit: (v - mean[c]) /
    (std[c] + eps). stats: a StatsResult, a (means, stds) pair or a directory
    holding train_stats.json; None is the reference's inference.py, which does
    not normalise. out: the result's buffer; report: a `new_report` tensor whose
    columns 0-2 receive the NaN / +Inf / -Inf counts of each image's own
    samples. No host synchronisation."""
    x = _frames_4d(x, "prepare_frames: x")
    B, C, H, W = x.shape
    Hp, Wp = padded_size(H, W, pad_multiple)
    dev = x.device
    per = lib.nsm_frame_blocks(C, Hp, Wp)
    if per <= 0:
        raise ValueError(f"prepare_frames: unsupported frame size {C} x {Hp} x {Wp}")
    if out is not None:
        _check_buffer(out, (B, C, Hp, Wp), torch.float32, dev, "prepare_frames: out")
    if report is not None:
        _check_buffer(report, (B, 6), torch.int32, dev, "report")
    norm = _norm_of(stats, C, dev)       # the last check; its copy is the first GPU work
    if out is None:
        out = torch.empty((B, C, Hp, Wp), dtype=torch.float32, device=dev)
    part = _census_ws(B, per, dev) if report is not None else None
    x = x.detach().contiguous()
    mean, std = norm if norm is not None else (None, None)
    call("nsm_frame_prep", ptr(x), B, C, H, W, Hp, Wp, ptr(mean), ptr(std), float(eps),
         int(bool(scrub)), ptr(out), ptr(part), ptr(report), stream())
    return out


def finish_frames(out, size=None, *, quantize=True, out_u8=None, out_f32=None, report=None):
    """The network's output ([B,C,Hp,Wp] or [C,Hp,Wp], fp32, C = 1, 3 or 4) ->
    the frame as save_output writes it, in one pass: the top-left size = (H, W)
    (None: all of it), scrubbed, clipped to [0,1], and `(v * 255)` truncated to
    uint8 with the channels last: [B,H,W] for C = 1, [B,H,W,C] otherwise.
    quantize=False returns the clipped fp32 frame [B,C,H,W] instead (what
    TemporalAA and the metrics take). Both are written when a buffer for the
    other one is given (out_u8 / out_f32; the uint8 buffer is [B,H,W,C] or, for
    C = 1, [B,H,W]). report: columns 3-5 receive the non-finite / < 0 / > 1
    counts of each image's cropped region before the scrub and the clip. No
    host synchronisation."""
    o = _frames_4d(out, "finish_frames: out")
    B, C, Hp, Wp = o.shape
    if C not in _FINISH_CHANNELS:
        raise ValueError(f"finish_frames: {C} channels; an image has 1, 3 or 4")
    if size is None:
        H, W = Hp, Wp
    else:
        try:
            H, W = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError(f"finish_frames: size must be (H, W) or None, got {size!r}") from None
        if H < 1 or W < 1 or H > Hp or W > Wp:
            raise ValueError(f"finish_frames: crop {H} x {W} does not fit the {Hp} x {Wp} frame")
    dev = o.device
    per = lib.nsm_frame_blocks(1, H, W)
    if per <= 0 or lib.nsm_frame_blocks(C, Hp, Wp) <= 0:
        raise ValueError(f"finish_frames: unsupported frame size {C} x {Hp} x {Wp}")
    u8_shape = (B, H, W) if C == 1 else (B, H, W, C)
    if report is not None:
        _check_buffer(report, (B, 6), torch.int32, dev, "report")
    u8 = f32 = None
    if out_u8 is not None:
        u8 = _check_buffer(out_u8, u8_shape, torch.uint8, dev, "finish_frames: out_u8")
    elif quantize:
        u8 = torch.empty(u8_shape, dtype=torch.uint8, device=dev)
    if out_f32 is not None:
        f32 = _check_buffer(out_f32, (B, C, H, W), torch.float32, dev, "finish_frames: out_f32")
    elif not quantize:
        f32 = torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
    part = _census_ws(B, per, dev) if report is not None else None
    o = o.detach().contiguous()
    call("nsm_frame_finish", ptr(o), B, C, Hp, Wp, H, W, ptr(u8), ptr(f32), ptr(part),
         ptr(report), stream())
    return u8 if quantize else f32


class FramePipeline(GraphedUnet):
    """prepare_frames -> eval forward -> finish_frames of a fixed raw frame
    shape, captured in one graph: a frame costs one copy into the raw buffer
    and one graph launch.

        pipe = FramePipeline(model, example)     # example: raw [B,C,H,W] fp32 on the GPU
        img = pipe(x)                            # uint8, x of the example's shape

    `pipe(x)` returns the graph's static uint8 tensor ([B,h,w], or [B,h,w,C] for
    a multi-channel output) and `pipe.shadow` the fp32 frame [B,C,h,w] of the
    same call; both are overwritten by the next call (clone to keep them).
    `pipe.raw` is the static raw input for callers who write it themselves
    (a loader's copy target): `pipe.replay()` then runs the graph. `pipe.report()`
    synchronises and returns the six per-image census counts of the last frame.

    The defaults are the reference's inference.py: crop=False keeps the padded
    size (the reference never crops back, its PNG has the padded size; crop=True
    returns the frame's own H x W), and stats=None does not normalise. A model
    trained on normalised inputs (FrameLoader, MmapLiverDataset) needs `stats=`
    (what FrameLoader(stats=...) takes, or the directory of train_stats.json), or
    it sees differently scaled inputs than in training.

    The model runs in the compute dtype it is set to; its output is fp32 in each
    of them (nsm_head_fwd writes float). Its training flag is restored after the
    capture. The weights are handled as in GraphedUnet, whose capture this
    shares: frozen layouts (static_weights=True), rewritten before a replay when
    a parameter's or buffer's version counter moved, and a RuntimeError when the
    parameters were re-allocated after the capture."""

    def __init__(self, model, example, *, pad_multiple=16, stats=None, scrub=True, crop=False,
                 static_weights=True, warmup=2):
        if not torch.is_tensor(example) or example.dim() != 4:
            got = tuple(example.shape) if torch.is_tensor(example) else type(example).__name__
            raise ValueError(f"FramePipeline: example must be a raw [B,C,H,W] batch, got {got}")
        example = _frames_4d(example, "FramePipeline: example")
        B, C, H, W = example.shape
        Hp, Wp = padded_size(H, W, pad_multiple)
        dev = example.device
        self.shape, self.dtype = (B, C, H, W), example.dtype
        self.size = (H, W) if crop else (Hp, Wp)
        self._prep = dict(pad_multiple=pad_multiple, stats=_norm_of(stats, C, dev), scrub=scrub)
        self.raw = example.detach().clone(memory_format=torch.contiguous_format)
        self.static_in = torch.empty((B, C, Hp, Wp), dtype=torch.float32, device=dev)
        self.shadow = self._report = None
        self._capture(model, warmup, static_weights)

    def _body(self):
        B = self.shape[0]
        self._report = torch.empty((B, 6), dtype=torch.int32, device=self.raw.device)
        prepare_frames(self.raw, out=self.static_in, report=self._report, **self._prep)
        o = self.model(self.static_in)      # fp32 in every compute dtype (finish_frames checks)
        self.shadow = torch.empty((B, o.shape[1]) + self.size, dtype=torch.float32, device=o.device)
        return finish_frames(o, self.size, out_f32=self.shadow, report=self._report)

    def __call__(self, x):
        if (not torch.is_tensor(x) or tuple(x.shape) != self.shape or x.dtype != self.dtype
                or x.device != self.raw.device):
            got = (tuple(x.shape), x.dtype, str(x.device)) if torch.is_tensor(x) else \
                type(x).__name__
            raise ValueError(f"FramePipeline captured for {self.shape} {self.dtype} on "
                             f"{self.raw.device}, got {got}")
        self._check()
        self.raw.copy_(x)
        self.graph.replay()
        return self.static_out

    def report(self):
        """{key: [count per image]} of the last frame (REPORT_KEYS). Waits for it."""
        return report_dict(self._report)
