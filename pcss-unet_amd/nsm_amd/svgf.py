"""Spatiotemporal variance-guided filtering (SVGF, Schied et al. 2017): the
post-process denoiser of the paper's ray-tracing baseline (§4, Figure 9:
"5-SPP raytracing with SVGF"), on three fused libnsm kernels
(csrc/nsm_svgf.hip; include/nsm.h has the definition of every weight).

Per frame:
    accumulate  colour and the luminance moments are blended with the history
                reprojected along the motion vectors (the lookup and the position
                / depth / normal rejection of nsm_amd/taa.py, same device
                functions); N counts the frames a pixel has been seen, capped at
                `max_history`; a = max(alpha, 1/N); var = max(0, m2 - m1^2)
    variance    pixels with N < `min_history` take colour and variance from a
                7x7 edge-aware spatial estimate instead
    a-trous     `iterations` passes of the 5x5 edge-avoiding wavelet filter at
                steps 1, 2, 4, ..., guided by depth, normals and the variance
The colour after `feedback` a-trous passes (1: the paper's choice; 0: the
accumulated colour; clamped to `iterations`) is the next frame's history. With
`iterations = 0` a frame's result is its accumulated colour (the spatial
estimate then only feeds the returned variance), so that with alpha =
moments_alpha = 1 the input comes back bit for bit.

`atrous_filter` alone, without a variance, is a depth-aware post filter, e.g.
for a PCSS image or the network's output. Colour is [B,C,H,W] with C = 1 or 3,
depth [B,1,H,W], normals [B,3,H,W], motion vectors [B,2,H,W] in the convention
of nsm_amd/temporal.py. Inputs may be fp32, fp16 or bf16 (converted to fp32 as
the metric converts them); every output is fp32. Wrong arguments raise
ValueError before any GPU work; nothing synchronises with the host.
"""
import torch

from ._lib import call, lib, ptr, stream
from .temporal import TemporalInstability, _f32, _scale, _seq


def _fail(msg):
    raise ValueError("SVGF: " + msg)


def _expect(t, what, shape, optional=False):
    if t is None:
        if optional:
            return
        _fail(f"{what} is required ({tuple(shape)})")
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        _fail(f"{what} is {got}, expected {tuple(shape)}")


def _color_shape(t, what):
    if not torch.is_tensor(t) or t.dim() != 4:
        _fail(f"{what} must be a [B,C,H,W] tensor")
    if t.shape[1] not in (1, 3):
        _fail(f"{what} has {t.shape[1]} channels, expected 1 (visibility) or 3 (RGB)")
    return tuple(t.shape)


def _device(tensors):
    """The one GPU device every tensor is on (ValueError for a CPU tensor)."""
    dev = None
    for what, t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            _fail(f"{what} must be on a ROCm GPU device (got {t.device}); there is no CPU "
                  "implementation")
        if dev is not None and t.device != dev:
            _fail(f"{what} is on {t.device}, expected {dev}")
        dev = t.device
    return dev


def _supported(shape):
    per = lib.nsm_svgf_blocks(*shape)
    if per <= 0:
        _fail(f"unsupported shape {tuple(shape)} (C*H*W must be below 2^31)")
    return per


def _overlap(a, b):
    return (a.data_ptr() < b.data_ptr() + b.numel() * b.element_size()
            and b.data_ptr() < a.data_ptr() + a.numel() * a.element_size())


def _out(out, what, shape, dev, inputs):
    """A caller's output buffer checked, or a new one."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    _expect(out, what, shape)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        _fail(f"{what} must be a contiguous fp32 tensor on {dev}")
    if any(t is not None and _overlap(out, t) for t in inputs):
        _fail(f"{what} aliases an input (the kernel gathers from its inputs)")
    return out


def _unit(v, what):
    v = float(v)
    if not (0.0 < v <= 1.0):
        _fail(f"{what} must be in (0, 1], got {v!r}")
    return v


def _count(v, what, least):
    if int(v) != v or int(v) < least or int(v) > 1 << 24:
        _fail(f"{what} must be an integer in [{least}, 2^24], got {v!r}")
    return int(v)


def _sigmas(sigma_z, sigma_n, sigma_l=0.0):
    s = tuple(float(v) for v in (sigma_z, sigma_n, sigma_l))
    if not (s[0] > 0.0) or not (s[1] >= 0.0) or not (s[2] >= 0.0):
        _fail(f"sigma_z must be positive, sigma_n and sigma_l non-negative, got {s}")
    return s


# ---- the three launches (checked fp32 contiguous tensors) -------------------------
def _accumulate(cur, z, n, zp, np_, mv, hist, scale, alpha, moments_alpha, max_history,
                depth_tol, normal_cos, oc, om, on, ov, accepted=None):
    B, C, H, W = cur.shape
    hc, hm, hn = hist if hist is not None else (None, None, None)
    call("nsm_svgf_accumulate", ptr(cur), ptr(z), ptr(n), ptr(zp), ptr(np_), ptr(mv), ptr(hc),
         ptr(hm), ptr(hn), B, C, H, W, scale[0], scale[1], alpha, moments_alpha, max_history,
         float(depth_tol), float(normal_cos), ptr(oc), ptr(om), ptr(on), ptr(ov), ptr(accepted),
         stream())


def _variance(c, m, n, v, z, nr, min_history, sigma_z, sigma_n, oc, ov):
    B, C, H, W = c.shape
    call("nsm_svgf_variance", ptr(c), ptr(m), ptr(n), ptr(v), ptr(z), ptr(nr), B, C, H, W,
         min_history, sigma_z, sigma_n, ptr(oc), ptr(ov), stream())


def _atrous(c, v, z, nr, step, sigma_z, sigma_n, sigma_l, oc, ov):
    B, C, H, W = c.shape
    call("nsm_svgf_atrous", ptr(c), ptr(v), ptr(z), ptr(nr), B, C, H, W, step, sigma_z, sigma_n,
         sigma_l, ptr(oc), ptr(ov), stream())


# ---- the passes as ops ------------------------------------------------------------
def atrous_filter(color, depth, normals, variance=None, *, step=1, sigma_z=1.0, sigma_n=128.0,
                  sigma_l=4.0, out=None):
    """One iteration of the edge-avoiding a-trous filter at `step` (2^i in
    iteration i): taps p + step * (dx, dy), dx, dy in [-2, 2], weighted by the
    B3 spline, the depth weight exp(-|dz| / (sigma_z |grad z . (q - p)| + 1e-8)),
    the normal weight max(0, n_p . n_q)^sigma_n and, with `variance` [B,1,H,W] and
    sigma_l > 0, the luminance weight exp(-|dl| / (sigma_l sqrt(g3x3(var) + 1e-10))).
    Returns color', or (color', variance') with a variance. `out` (fp32,
    contiguous, colour's shape, no input's memory) receives color'."""
    B, C, H, W = shape = _color_shape(color, "color")
    _expect(depth, "depth", (B, 1, H, W))
    _expect(normals, "normals", (B, 3, H, W))
    _expect(variance, "variance", (B, 1, H, W), optional=True)
    if int(step) != step or not (1 <= int(step) <= 1 << 20):
        _fail(f"step must be an integer in [1, 2^20], got {step!r}")
    sz, sn, sl = _sigmas(sigma_z, sigma_n, sigma_l)
    dev = _device((("color", color), ("depth", depth), ("normals", normals),
                   ("variance", variance)) + ((("out", out),) if torch.is_tensor(out) else ()))
    _supported(shape)
    c, z, n = _f32(color), _f32(depth), _f32(normals)
    v = _f32(variance) if variance is not None and sl != 0.0 else None
    out = _out(out, "out", shape, dev, (c, z, n, v))
    ov = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if v is not None else None
    _atrous(c, v, z, n, int(step), sz, sn, sl, out, ov)
    return (out, ov) if v is not None else out


def svgf_accumulate(cur, motion_vectors=None, *, depth=None, normals=None, prev_depth=None,
                    prev_normals=None, history=None, alpha=0.2, moments_alpha=0.2, max_history=32,
                    depth_tol=0.1, normal_cos=0.9, mv_scale=(1.0, 1.0), return_mask=False):
    """The temporal accumulation of one frame. `history`: None for a first
    frame, else (colour [B,C,H,W], moments [B,2,H,W], length [B,1,H,W]) as a
    previous call returned them (the colour possibly filtered since). With
    `motion_vectors` and a history, this frame's and the previous frame's depth
    and normals are required. Returns (colour, moments, length, variance), with
    `return_mask` also accepted [B,1,H,W] bool: where the history was used."""
    B, C, H, W = shape = _color_shape(cur, "cur")
    alpha, moments_alpha = _unit(alpha, "alpha"), _unit(moments_alpha, "moments_alpha")
    max_history, scale = _count(max_history, "max_history", 1), _scale(mv_scale)
    _expect(motion_vectors, "motion_vectors", (B, 2, H, W), optional=True)
    guides = (("depth", depth, 1), ("normals", normals, 3), ("prev_depth", prev_depth, 1),
              ("prev_normals", prev_normals, 3))
    needed = motion_vectors is not None and history is not None
    for what, t, ch in guides:
        _expect(t, what, (B, ch, H, W), optional=not needed)
    if history is not None:
        if not isinstance(history, (tuple, list)) or len(history) != 3:
            _fail("history must be (colour, moments, length) or None")
        for what, t, ch in zip(("history colour", "history moments", "history length"), history,
                               (C, 2, 1)):
            _expect(t, what, (B, ch, H, W))
    dev = _device([("cur", cur), ("motion_vectors", motion_vectors)]
                  + [(w, t) for w, t, _ in guides]
                  + [("history", t) for t in (history or ())])
    _supported(shape)
    hist = tuple(_f32(t) for t in history) if history is not None else None
    mv = _f32(motion_vectors) if motion_vectors is not None else None
    z, n, zp, np_ = (_f32(t) if t is not None and needed else None for _, t, _ in guides)
    oc = torch.empty(shape, dtype=torch.float32, device=dev)
    om = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
    on, ov = (torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) for _ in range(2))
    acc = torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev) if return_mask else None
    _accumulate(_f32(cur), z, n, zp, np_, mv, hist, scale, alpha, moments_alpha, max_history,
                depth_tol, normal_cos, oc, om, on, ov, acc)
    return (oc, om, on, ov) + ((acc.view(torch.bool),) if return_mask else ())


def svgf_variance(color, moments, length, variance, depth, normals, *, min_history=4,
                  sigma_z=1.0, sigma_n=128.0):
    """The spatial fallback for short histories: where `length` < `min_history`,
    colour and variance come from the 7x7 depth- and normal-weighted means of
    colour and moments, the variance scaled by min_history / length; every other
    pixel passes through. Returns (color', variance')."""
    B, C, H, W = shape = _color_shape(color, "color")
    for what, t, ch in (("moments", moments, 2), ("length", length, 1), ("variance", variance, 1),
                        ("depth", depth, 1), ("normals", normals, 3)):
        _expect(t, what, (B, ch, H, W))
    min_history = _count(min_history, "min_history", 0)
    sz, sn, _ = _sigmas(sigma_z, sigma_n)
    dev = _device((("color", color), ("moments", moments), ("length", length),
                   ("variance", variance), ("depth", depth), ("normals", normals)))
    _supported(shape)
    oc = torch.empty(shape, dtype=torch.float32, device=dev)
    ov = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    _variance(_f32(color), _f32(moments), _f32(length), _f32(variance), _f32(depth), _f32(normals),
              min_history, sz, sn, oc, ov)
    return oc, ov


# ---- the recurrence ---------------------------------------------------------------
class _Engine:
    """The parameters of the recurrence, its history (two sets of colour,
    moments and length, one read and one written per frame) and its work
    buffers. `static`: the history is always read from set 0 (a frame ends with
    three copies from set 1), so every address is fixed."""

    def __init__(self, iterations, alpha, moments_alpha, max_history, min_history, feedback,
                 sigma_z, sigma_n, sigma_l, depth_tol, normal_cos, mv_scale, static=False):
        if int(iterations) != iterations or int(iterations) < 0 or int(iterations) > 20:
            _fail(f"iterations must be an integer in [0, 20], got {iterations!r}")
        self.iterations = int(iterations)
        self.alpha, self.moments_alpha = _unit(alpha, "alpha"), _unit(moments_alpha, "moments_alpha")
        self.max_history = _count(max_history, "max_history", 1)
        self.min_history = _count(min_history, "min_history", 0)
        if int(feedback) != feedback or int(feedback) < 0:
            _fail(f"feedback must be a non-negative integer, got {feedback!r}")
        self.feedback = min(int(feedback), self.iterations)
        self.sigmas = _sigmas(sigma_z, sigma_n, sigma_l)
        self.depth_tol, self.normal_cos = float(depth_tol), float(normal_cos)
        self.scale, self.static = _scale(mv_scale), bool(static)
        self.shape = self.dev = None
        self.read = 0       # the history set that holds the latest frame

    def prepare(self, shape, dev):
        if self.shape == tuple(shape) and self.dev == dev:
            return
        B, C, H, W = self.shape = tuple(shape)
        self.dev = dev

        def new(ch):
            return torch.empty((B, ch, H, W), dtype=torch.float32, device=dev)

        self.hist = [(new(C), new(2), new(1)) for _ in range(2)]
        self.work_c, self.work_v = [new(C), new(C)], [new(1), new(1)]

    def frame(self, cur, z, n, zp, np_, mv, first, out, var_out=None, accepted=None):
        """One frame into `out` (and `var_out`); first: no history is read."""
        sz, sn, sl = self.sigmas
        src = None if first else self.hist[0 if self.static else self.read]
        dst = self.hist[1 if self.static else 1 - self.read]
        its, fb = self.iterations, self.feedback
        wc, wv = self.work_c, self.work_v
        c = out if its == 0 else dst[0] if fb == 0 else wc[0]
        _accumulate(cur, z, n, zp, np_, mv if not first else None, src, self.scale, self.alpha,
                    self.moments_alpha, self.max_history, self.depth_tol, self.normal_cos, c,
                    dst[1], dst[2], wv[0], accepted)
        if its == 0:
            dst[0].copy_(out)
            if var_out is not None:
                _variance(c, dst[1], dst[2], wv[0], z, n, self.min_history, sz, sn, wc[0], var_out)
        else:
            _variance(c, dst[1], dst[2], wv[0], z, n, self.min_history, sz, sn, wc[1], wv[1])
            c, v = wc[1], 1
            for k in range(1, its + 1):
                oc = out if k == its else dst[0] if k == fb else wc[0] if c is not wc[0] else wc[1]
                ov = var_out if k == its and var_out is not None else wv[1 - v]
                _atrous(c, wv[v] if sl != 0.0 else None, z, n, 1 << (k - 1), sz, sn, sl, oc,
                        ov if sl != 0.0 else None)
                c, v = oc, 1 - v
            if fb == its:
                dst[0].copy_(out)
            if var_out is not None and sl == 0.0:   # no a-trous pass moves the variance
                var_out.copy_(wv[1])
        if self.static:
            for d, s in zip(self.hist[0], self.hist[1]):
                d.copy_(s)
        else:
            self.read = 1 - self.read


def svgf(frames, motion_vectors=None, *, depth, normals, iterations=5, alpha=0.2,
         moments_alpha=0.2, max_history=32, min_history=4, feedback=1, sigma_z=1.0,
         sigma_n=128.0, sigma_l=4.0, depth_tol=0.1, normal_cos=0.9, mv_scale=(1.0, 1.0),
         return_variance=False):
    """A held sequence denoised into one [T,B,C,H,W] fp32 tensor. frames: T
    tensors [B,C,H,W] or one [T,B,C,H,W] tensor; motion_vectors: T-1 x [B,2,H,W]
    or None (nothing moves, nothing is rejected); depth: T x [B,1,H,W]; normals:
    T x [B,3,H,W]. With `return_variance` also the filtered variance
    [T,B,1,H,W]. The module docstring has the passes and `feedback`."""
    eng = _Engine(iterations, alpha, moments_alpha, max_history, min_history, feedback, sigma_z,
                  sigma_n, sigma_l, depth_tol, normal_cos, mv_scale)
    if not torch.is_tensor(frames) and not isinstance(frames, (list, tuple)):
        _fail("frames must be T tensors [B,C,H,W] or one [T,B,C,H,W] tensor")
    T = len(frames)
    if T == 0:
        _fail("frames must be T tensors [B,C,H,W] or one [T,B,C,H,W] tensor")
    B, C, H, W = shape = _color_shape(frames[0], "frames[0]")
    if depth is None or normals is None:
        _fail("depth and normals guide every pass; both are required")
    fr = _seq(frames, "frames", T, shape, "SVGF")
    mv = _seq(motion_vectors, "motion_vectors", T - 1, (B, 2, H, W), "SVGF")
    dz = _seq(depth, "depth", T, (B, 1, H, W), "SVGF")
    nr = _seq(normals, "normals", T, (B, 3, H, W), "SVGF")
    dev = _device([("frames", t) for t in fr] + [("motion_vectors", t) for t in mv or ()]
                  + [("depth", t) for t in dz] + [("normals", t) for t in nr])
    _supported(shape)
    fr, dz, nr = ([_f32(t) for t in s] for s in (fr, dz, nr))
    mv = [_f32(m) for m in mv] if mv is not None else None
    out = torch.empty((T,) + shape, dtype=torch.float32, device=dev)
    var = torch.empty((T, B, 1, H, W), dtype=torch.float32, device=dev) if return_variance else None
    eng.prepare(shape, dev)
    for t in range(T):
        eng.frame(fr[t], dz[t], nr[t], dz[t - 1] if t else None, nr[t - 1] if t else None,
                  mv[t - 1] if mv and t else None, t == 0, out[t],
                  var[t] if return_variance else None)
    return (out, var) if return_variance else out


class SVGF:
    """The streaming form, e.g. behind FramePipeline.shadow: `svgf(frame,
    motion_vectors, depth, normals)` returns the denoised frame (fp32; with
    `return_variance` also its variance); the first frame of a sequence has no
    history and its motion vectors are ignored; reset() starts a new sequence.
    It keeps its own copies of the previous depth and normals and owns the
    history and every work buffer. Fed the same sequence it returns `svgf`'s
    frames bit for bit.

    The returned tensors are buffers the object owns and alternates between: a
    later call overwrites them, clone them to keep them. With `capturable=True`
    every buffer stays at a fixed address instead (a frame ends with three
    history-sized copy_ on the same stream), so a call captured in
    torch.cuda.graph replays correctly; give the first frame outside the
    capture."""

    def __init__(self, iterations=5, *, alpha=0.2, moments_alpha=0.2, max_history=32,
                 min_history=4, feedback=1, sigma_z=1.0, sigma_n=128.0, sigma_l=4.0, depth_tol=0.1,
                 normal_cos=0.9, mv_scale=(1.0, 1.0), return_variance=False, capturable=False):
        self.capturable, self.return_variance = bool(capturable), bool(return_variance)
        self._eng = _Engine(iterations, alpha, moments_alpha, max_history, min_history, feedback,
                            sigma_z, sigma_n, sigma_l, depth_tol, normal_cos, mv_scale,
                            static=self.capturable)
        self._out = self._var = None
        self._cur = 0
        self._prev_depth = self._prev_normals = None
        self._have = False

    def reset(self):
        self._have = False

    _keep = staticmethod(TemporalInstability._keep)

    def __call__(self, frame, motion_vectors=None, depth=None, normals=None):
        B, C, H, W = shape = _color_shape(frame, "frame")
        _expect(motion_vectors, "motion_vectors", (B, 2, H, W), optional=True)
        _expect(depth, "depth", (B, 1, H, W))
        _expect(normals, "normals", (B, 3, H, W))
        eng = self._eng
        if self._have and eng.shape != shape:
            _fail(f"frame is {shape}, the previous one was {eng.shape}")
        dev = _device((("frame", frame), ("motion_vectors", motion_vectors), ("depth", depth),
                       ("normals", normals)))
        _supported(shape)
        if eng.shape != shape or eng.dev != dev:
            self._have = False
            self._out = [torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(2)]
            self._var = [torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
                         for _ in range(2)]
            eng.prepare(shape, dev)
        cur, z, n = _f32(frame), _f32(depth), _f32(normals)
        mv = _f32(motion_vectors) if motion_vectors is not None and self._have else None
        if not self.capturable:
            self._cur = 1 - self._cur
        out = self._out[self._cur]
        var = self._var[self._cur] if self.return_variance else None
        eng.frame(cur, z, n, self._prev_depth if self._have else None,
                  self._prev_normals if self._have else None, mv, not self._have, out, var)
        self._prev_depth = self._keep(self._prev_depth, z)
        self._prev_normals = self._keep(self._prev_normals, n)
        self._have = True
        return (out, var) if self.return_variance else out
