"""Temporal anti-aliasing resolve (the paper's "TAA (1 last frame)" baseline of
Figure 6, §3.4) as one fused libnsm kernel per frame (nsm_taa_resolve).

    O_0 = I_0
    h   = bilinear sample of O_{t-1} at m(p)          (the previous RESOLVED frame)
    h   = min(max(h, lo), hi)                         (clamp: lo / hi = min / max of I_t
                                                       over the 3x3 neighbourhood of p,
                                                       edge replicate)
    O_t = accepted(p) ? fma(1 - blend, h - I_t, I_t) : I_t

`blend` in (0, 1] is the weight of the current frame. The motion-vector
convention, `mv_scale`, the lookup and the rejection tests (position, depth,
normals) are those of nsm_amd/temporal.py, from the same device functions:
`motion_vectors` maps the pixels of frame t into frame t-1, and depth and
normals are compared with the previous INPUT frame's, so a verdict does not
depend on the recurrence. Without motion vectors nothing moves and nothing is
rejected. Inputs may be fp32, fp16 or bf16 (converted to fp32 as the metric
does); the output is fp32. No host synchronisation anywhere.
"""
import torch

from ._lib import call, ptr, require_gpu, stream
from .temporal import TemporalInstability, _blocks, _f32, _scale, _seq


def _blend(blend):
    b = float(blend)
    if not (0.0 < b <= 1.0):
        raise ValueError(f"temporal AA: blend must be in (0, 1], got {blend!r}")
    return b


def _frame_shape(frame, what):
    if not torch.is_tensor(frame) or frame.dim() != 4:
        raise ValueError(f"temporal AA: {what} must be a [B,C,H,W] tensor")
    return tuple(frame.shape)


def _expect(t, what, shape):
    if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != tuple(shape)):
        got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"temporal AA: {what} is {got}, expected {tuple(shape)}")


def _needs_mv(motion_vectors, *rejecters):
    if motion_vectors is None and any(r is not None for r in rejecters):
        raise ValueError("temporal AA: depth and normals reject reprojected pixels; they need "
                         "motion_vectors")


def _launch(cur, hist, mv, zc, zp, nc, np_, scale, blend, clamp, depth_tol, normal_cos, out,
            accepted=None):
    B, C, H, W = cur.shape
    call("nsm_taa_resolve", ptr(cur), ptr(hist), ptr(mv), ptr(zc), ptr(zp), ptr(nc), ptr(np_),
         B, C, H, W, scale[0], scale[1], blend, int(clamp), float(depth_tol), float(normal_cos),
         ptr(out), ptr(accepted), stream())


def taa_resolve(cur, history, motion_vectors=None, *, depth=None, prev_depth=None, normals=None,
                prev_normals=None, blend=0.1, clamp=True, depth_tol=0.1, normal_cos=0.9,
                mv_scale=(1.0, 1.0), out=None, return_mask=False):
    """One step: `cur` [B,C,H,W] resolved against `history` (the previous
    resolved frame). `depth` / `prev_depth` [B,1,H,W] and `normals` /
    `prev_normals` [B,3,H,W] come in pairs (this frame's and the previous input
    frame's) and need `motion_vectors` [B,2,H,W]. `out` (fp32, contiguous, the
    frame's shape, neither `cur` nor `history`) receives the result. Returns the
    resolved frame, with `return_mask` also `accepted` [B,1,H,W] bool: where the
    history was used. Wrong shapes raise ValueError before any GPU work."""
    blend, scale = _blend(blend), _scale(mv_scale)
    B, C, H, W = shape = _frame_shape(cur, "cur")
    _expect(history, "history", shape)
    if history is None:
        raise ValueError("temporal AA: history must be a [B,C,H,W] tensor")
    _expect(motion_vectors, "motion_vectors", (B, 2, H, W))
    for what, a, b, ch in (("depth", depth, prev_depth, 1), ("normals", normals, prev_normals, 3)):
        if (a is None) != (b is None):
            raise ValueError(f"temporal AA: {what} and prev_{what} come together or not at all")
        _expect(a, what, (B, ch, H, W))
        _expect(b, f"prev_{what}", (B, ch, H, W))
    _needs_mv(motion_vectors, depth, normals)
    if out is not None:
        _expect(out, "out", shape)
        if out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("temporal AA: out must be a contiguous fp32 tensor")
    dev = require_gpu(cur, "temporal-AA frame").device
    _blocks(shape)
    c, h = _f32(cur), _f32(history, dev)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif out.device != dev or out.data_ptr() in (c.data_ptr(), h.data_ptr()):
        raise ValueError("temporal AA: out must be on the frame's device and be neither cur nor "
                         "history (the kernel gathers from both)")
    mv, zc, zp, nc, np_ = (_f32(t, dev) if t is not None else None
                           for t in (motion_vectors, depth, prev_depth, normals, prev_normals))
    acc = torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev) if return_mask else None
    _launch(c, h, mv, zc, zp, nc, np_, scale, blend, clamp, depth_tol, normal_cos, out, acc)
    return (out, acc.view(torch.bool)) if return_mask else out


def temporal_aa(frames, motion_vectors=None, *, depth=None, normals=None, blend=0.1, clamp=True,
                depth_tol=0.1, normal_cos=0.9, mv_scale=(1.0, 1.0), return_mask=False):
    """A whole sequence resolved into one [T,B,C,H,W] fp32 tensor (slice t-1 is
    the history of slice t: nothing is copied but the first frame). frames: T
    tensors [B,C,H,W] or one [T,B,C,H,W] tensor; motion_vectors: T-1 x
    [B,2,H,W]; depth: T x [B,1,H,W]; normals: T x [B,3,H,W]. With `return_mask`
    also `accepted` [T,B,1,H,W] bool (all False for the first frame, which has no
    history). Wrong lengths and shapes raise ValueError before any GPU work."""
    blend, scale = _blend(blend), _scale(mv_scale)
    _needs_mv(motion_vectors, depth, normals)
    T = len(frames)
    if T == 0:
        raise ValueError("temporal AA: frames must be T tensors [B,C,H,W] or one [T,B,C,H,W] "
                         "tensor")
    B, C, H, W = shape = _frame_shape(frames[0], "frames[0]")
    fr = _seq(frames, "frames", T, shape, "temporal AA")
    mv = _seq(motion_vectors, "motion_vectors", T - 1, (B, 2, H, W), "temporal AA")
    dz = _seq(depth, "depth", T, (B, 1, H, W), "temporal AA")
    nr = _seq(normals, "normals", T, (B, 3, H, W), "temporal AA")
    dev = require_gpu(fr[0], "temporal-AA frames").device
    _blocks(shape)
    fr = [_f32(f) for f in fr]
    mv = [_f32(m, dev) for m in mv] if mv is not None else None
    dz = [_f32(z, dev) for z in dz] if dz is not None else None
    nr = [_f32(n, dev) for n in nr] if nr is not None else None
    out = torch.empty((T,) + shape, dtype=torch.float32, device=dev)
    acc = torch.zeros((T, B, 1, H, W), dtype=torch.uint8, device=dev) if return_mask else None
    out[0].copy_(fr[0])
    for t in range(1, T):
        _launch(fr[t], out[t - 1], mv[t - 1] if mv else None,
                dz[t] if dz else None, dz[t - 1] if dz else None,
                nr[t] if nr else None, nr[t - 1] if nr else None,
                scale, blend, clamp, depth_tol, normal_cos, out[t],
                acc[t] if return_mask else None)
    return (out, acc.view(torch.bool)) if return_mask else out


class TemporalAA:
    """The streaming form, e.g. behind GraphedUnet: `taa(frame, motion_vectors,
    depth, normals)` returns the resolved frame (fp32); the first frame of a
    sequence passes through and its motion vectors are ignored; reset() starts a
    new sequence. It keeps its own copies of the previous depth and normals,
    and the history is its own previous output. Fed the same sequence it
    returns temporal_aa's frames bit for bit.

    The returned tensor is one of two buffers the object owns and alternates
    between: a later call overwrites it, clone it to keep it. With
    `capturable=True` every buffer stays at a fixed address instead (the kernel
    writes one static output, then one frame-sized copy_ refreshes the history
    on the same stream), so a call captured in torch.cuda.graph replays
    correctly; give the first frame outside the capture."""

    def __init__(self, blend=0.1, clamp=True, *, depth_tol=0.1, normal_cos=0.9,
                 mv_scale=(1.0, 1.0), capturable=False):
        self.blend, self.clamp = _blend(blend), bool(clamp)
        self.depth_tol, self.normal_cos = float(depth_tol), float(normal_cos)
        self.mv_scale, self.capturable = _scale(mv_scale), bool(capturable)
        self._bufs = [None, None]   # capturable: [static output, history]
        self._cur = 0               # the buffer that holds the latest resolved frame
        self._prev_depth = self._prev_normals = None
        self._have = (False, False, False)   # a history / previous depth / normals is held

    def reset(self):
        self._have = (False, False, False)

    _keep = staticmethod(TemporalInstability._keep)

    def __call__(self, frame, motion_vectors=None, depth=None, normals=None):
        B, C, H, W = shape = _frame_shape(frame, "frame")
        _expect(motion_vectors, "motion_vectors", (B, 2, H, W))
        _expect(depth, "depth", (B, 1, H, W))
        _expect(normals, "normals", (B, 3, H, W))
        have, have_z, have_n = self._have
        if have:
            if tuple(self._bufs[0].shape) != shape:
                raise ValueError(f"temporal AA: frame is {shape}, the previous one was "
                                 f"{tuple(self._bufs[0].shape)}")
            _needs_mv(motion_vectors, depth, normals)
            if (depth is not None and not have_z) or (normals is not None and not have_n):
                raise ValueError("temporal AA: depth / normals must come with every frame of a "
                                 "sequence, the previous frame had none")
        dev = require_gpu(frame, "temporal-AA frame").device
        _blocks(shape)
        cur = _f32(frame)
        z = _f32(depth, dev) if depth is not None else None
        nr = _f32(normals, dev) if normals is not None else None
        for i in (0, 1):
            b = self._bufs[i]
            if b is None or tuple(b.shape) != shape or b.device != dev:
                self._bufs[i] = torch.empty(shape, dtype=torch.float32, device=dev)
        if self.capturable:
            dst, hist = self._bufs
        else:
            hist = self._bufs[self._cur]
            dst = self._bufs[1 - self._cur] if have else hist
        if have:
            mv = _f32(motion_vectors, dev) if motion_vectors is not None else None
            _launch(cur, hist, mv, z, self._prev_depth if z is not None else None,
                    nr, self._prev_normals if nr is not None else None, self.mv_scale,
                    self.blend, self.clamp, self.depth_tol, self.normal_cos, dst)
            self._cur = 1 - self._cur
        else:
            dst.copy_(cur)
        if self.capturable:
            hist.copy_(dst)
        if z is not None:
            self._prev_depth = self._keep(self._prev_depth, z)
        if nr is not None:
            self._prev_normals = self._keep(self._prev_normals, nr)
        self._have = (True, z is not None, nr is not None)
        return dst
