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

A renderer that has the rasteriser's raw buffers and a model trained on channels
composed from them (features.FeatureRecipe) passes the recipe:
`compose_features` (csrc/nsm_features.hip, nsm_feature_compose) is
prepare_frames with the composition in front of the scrub and the emitter
offset of the paper's §3.1.1 behind it, still one pass, and
`FramePipeline(model, raw_example, recipe=..., emitter_channel=...)` captures it
in place of prepare_frames; columns 0-2 then count the composed values.
"""
import os

import torch

from ._lib import call, lib, ptr, stream
from .data import MmapLiverDataset, _given_stats, load_stats
from .features import FeatureRecipe
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


def _emitter_of(emitter, B, device):
    """The emitter offsets as a device [B] fp32 tensor: a float (every image), a
    sequence of B floats, or such a tensor itself."""
    if torch.is_tensor(emitter) and emitter.is_cuda:
        return _check_buffer(emitter, (B,), torch.float32, device, "compose_features: emitter")
    try:
        e = torch.as_tensor(emitter, dtype=torch.float32).reshape(-1)
    except (TypeError, ValueError, RuntimeError):
        e = None
    if e is None or e.numel() not in (1, B):
        raise ValueError(f"compose_features: emitter must be a number, {B} numbers (one per image) "
                         f"or a [{B}] float32 tensor on {device}, got {emitter!r}")
    return e.expand(B).contiguous().to(device)


def compose_features(x, recipe, *, pad_multiple=None, stats=None, scrub=False,
                     eps=MmapLiverDataset.EPS, emitter_channel=None, emitter=None, out=None,
                     report=None):
    """Raw G-buffers x ([B,Cin,H,W] or [Cin,H,W], fp32, on the GPU) -> the
    recipe's channels [B,Cout,Hp,Wp] fp32 in one pass, per output sample in this
    order: compose the term from the raw values at the (reflected) source pixel,
    count it into the census, scrub (scrub=True: NaN -> 0, +Inf -> 1, -Inf -> 0),
    add `emitter[b]` on `emitter_channel` only (the dc offset of the paper's
    §3.1.1; every other channel keeps its bits), and with `stats` normalise,
    (v - mean[c]) / (std[c] + eps) over the COMPOSED channel c. The defaults are
    the plain composition (what the stats pass and the patch pool take);
    pad_multiple, stats, scrub, out and report are prepare_frames's, with stats
    of Cout entries and the census (report columns 0-2) counting the composed
    values of an image's own pixels before the scrub. emitter: a float, B floats
    or a device [B] fp32 tensor (read by the kernel: a captured call follows new
    values); it goes with emitter_channel, both or neither. The recipe travels
    in the kernel's arguments: nothing is uploaded for it. No host
    synchronisation (host-side emitter numbers are one small upload; a device
    tensor is used as it is)."""
    if not isinstance(recipe, FeatureRecipe):
        raise ValueError(f"compose_features: recipe must be a FeatureRecipe, got "
                         f"{type(recipe).__name__}")
    x = _frames_4d(x, "compose_features: x")
    B, Cin, H, W = x.shape
    recipe.check_input(Cin, "compose_features")
    Cout = recipe.out_channels
    Hp, Wp = padded_size(H, W, pad_multiple)
    dev = x.device
    per = lib.nsm_feature_blocks(Cout, Hp, Wp)
    if per <= 0 or Cin * H * W >= 1 << 31:
        raise ValueError(f"compose_features: unsupported frame size {Cin} x {H} x {W} -> "
                         f"{Cout} x {Hp} x {Wp}")
    if (emitter_channel is None) != (emitter is None):
        raise ValueError("compose_features: emitter_channel and emitter go together, got "
                         f"{emitter_channel!r} and {emitter!r}")
    if emitter_channel is not None and (isinstance(emitter_channel, bool)
                                        or not isinstance(emitter_channel, int)
                                        or not 0 <= emitter_channel < Cout):
        raise ValueError(f"compose_features: emitter_channel must be in [0, {Cout}), got "
                         f"{emitter_channel!r}")
    if out is not None:
        _check_buffer(out, (B, Cout, Hp, Wp), torch.float32, dev, "compose_features: out")
    if report is not None:
        _check_buffer(report, (B, 6), torch.int32, dev, "report")
    em = _emitter_of(emitter, B, dev) if emitter is not None else None
    norm = _norm_of(stats, Cout, dev)    # the last check; its copy is GPU work
    if out is None:
        out = torch.empty((B, Cout, Hp, Wp), dtype=torch.float32, device=dev)
    part = _census_ws(B, per, dev) if report is not None else None
    x = x.detach().contiguous()
    mean, std = norm if norm is not None else (None, None)
    call("nsm_feature_compose", ptr(x), B, Cin, H, W, Hp, Wp, recipe._ctable, Cout,
         recipe.ratio_floor, ptr(mean), ptr(std), float(eps), int(bool(scrub)),
         -1 if emitter_channel is None else emitter_channel, ptr(em), ptr(out), ptr(part),
         ptr(report), stream())
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

    With `recipe=` (a features.FeatureRecipe) the example is the RAW [B,Cin,H,W]
    batch and compose_features takes prepare_frames's place in the graph:
    `static_in` is [B,Cout,Hp,Wp], `stats` are those of the composed channels and
    report columns 0-2 count the composed values. `emitter_channel=` (a composed
    channel; it needs a recipe, FeatureRecipe.identity(C) for raw channels) adds
    the emitter size to that channel: `pipe.emitter` is the static [B] fp32
    device tensor the graph reads (zeros at capture) and `pipe.set_emitter(v)`
    copies a number or B numbers into it, so the softness control of the paper's
    §3.1.1 needs no new capture. A new recipe is a new pipeline.

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

    def __init__(self, model, example, *, recipe=None, emitter_channel=None, pad_multiple=16,
                 stats=None, scrub=True, crop=False, static_weights=True, warmup=2):
        if not torch.is_tensor(example) or example.dim() != 4:
            got = tuple(example.shape) if torch.is_tensor(example) else type(example).__name__
            raise ValueError(f"FramePipeline: example must be a raw [B,C,H,W] batch, got {got}")
        example = _frames_4d(example, "FramePipeline: example")
        B, C, H, W = example.shape
        self.recipe, self.emitter_channel, self.emitter = recipe, emitter_channel, None
        Cnet = C                                  # the channels the network sees
        if recipe is not None:
            if not isinstance(recipe, FeatureRecipe):
                raise ValueError(f"FramePipeline: recipe must be a FeatureRecipe, got "
                                 f"{type(recipe).__name__}")
            recipe.check_input(C, "FramePipeline")
            Cnet = recipe.out_channels
            if emitter_channel is not None and (isinstance(emitter_channel, bool)
                                                or not isinstance(emitter_channel, int)
                                                or not 0 <= emitter_channel < Cnet):
                raise ValueError(f"FramePipeline: emitter_channel must be in [0, {Cnet}), got "
                                 f"{emitter_channel!r}")
        elif emitter_channel is not None:
            raise ValueError("FramePipeline: emitter_channel needs a recipe (it indexes the "
                             "composed channels); FeatureRecipe.identity(C) is the raw case")
        Hp, Wp = padded_size(H, W, pad_multiple)
        dev = example.device
        self.shape, self.dtype = (B, C, H, W), example.dtype
        self.size = (H, W) if crop else (Hp, Wp)
        self._prep = dict(pad_multiple=pad_multiple, stats=_norm_of(stats, Cnet, dev), scrub=scrub)
        self.raw = example.detach().clone(memory_format=torch.contiguous_format)
        self.static_in = torch.empty((B, Cnet, Hp, Wp), dtype=torch.float32, device=dev)
        if emitter_channel is not None:
            self.emitter = torch.zeros(B, dtype=torch.float32, device=dev)
        self.shadow = self._report = None
        self._capture(model, warmup, static_weights)

    def _body(self):
        B = self.shape[0]
        self._report = torch.empty((B, 6), dtype=torch.int32, device=self.raw.device)
        if self.recipe is None:
            prepare_frames(self.raw, out=self.static_in, report=self._report, **self._prep)
        else:
            compose_features(self.raw, self.recipe, out=self.static_in, report=self._report,
                             emitter_channel=self.emitter_channel, emitter=self.emitter,
                             **self._prep)
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

    def set_emitter(self, values):
        """Copy the emitter size (a number, or one per image) into `pipe.emitter` on
        the current stream; the next replay adds it to the emitter channel."""
        if self.emitter is None:
            raise ValueError("FramePipeline: set_emitter needs emitter_channel= at construction")
        B = self.shape[0]
        try:
            v = torch.as_tensor(values, dtype=torch.float32).reshape(-1)
        except (TypeError, ValueError, RuntimeError):
            v = None
        if v is None or v.numel() not in (1, B):
            raise ValueError(f"FramePipeline: set_emitter takes a number or {B} numbers, got "
                             f"{values!r}")
        self.emitter.copy_(v.expand(B))
        return self.emitter

    def report(self):
        """{key: [count per image]} of the last frame (REPORT_KEYS). Waits for it."""
        return report_dict(self._report)
