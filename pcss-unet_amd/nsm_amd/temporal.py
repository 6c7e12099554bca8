"""The temporal-instability metric (pert_loss.py:166-199; the paper's Eq. 3) on
the libnsm kernels, with motion-vector reprojection.

    D_t(p) = |I_t(p) - I_{t-1}(m(p))|,   E = mean(exp(alpha * D) - 1)

Motion-vector convention: `motion_vectors[t-1]` is a [B,2,H,W] tensor in pixels
that maps the pixels of frame t into frame t-1: pixel (x, y) of image b looks
up the previous frame at (x + mv[b,0,y,x] * mv_scale[0], y + mv[b,1,y,x] *
mv_scale[1]); channel 0 runs along the width; integer coordinates are pixel
centres (`align_corners=True` in F.grid_sample's terms); the lookup is
bilinear. `mv_scale` converts other units (e.g. (W, H) for motion in fractions
of the image, negative to flip the direction).

Rejection: a pixel whose lookup position is not finite or lies outside
[0, W-1] x [0, H-1] (bounds inclusive) does not count; with `depth`
(T x [B,1,H,W]) neither does one with |z_t - z~| > depth_tol * |z_t|, with
`normals` (T x [B,3,H,W]) one with dot(n_t, n~) < normal_cos, z~ and n~ being
the previous frame's values interpolated at the lookup position (n~ is not
renormalised; a NaN in either comparison rejects).

The reference's `measure_temporal_instability(frames, motion_vectors, alpha)`
accepts the motion vectors and leaves their branch as `pass`: with motion
vectors it raises UnboundLocalError on the first pair. Without them this
module's function is the reference's, on `nsm_expdiff_mean` as before.
"""
import torch

from ._lib import call, lib, ptr, require_gpu, stream

_NORMALIZE = ("valid", "all")


def _f32(t, device=None):
    """fp32 contiguous, as measure_temporal_instability has always converted."""
    t = t.detach().contiguous()
    return t.to(device=device, dtype=torch.float32) if device is not None else t.to(torch.float32)


def _seq(x, what, n, shape, who="temporal instability"):
    """A list of n tensors of `shape` from a list or a stacked tensor (ValueError otherwise)."""
    if x is None:
        return None
    if len(x) != n:
        raise ValueError(f"{who}: {what} has {len(x)} entries, expected {n}")
    out = [x[i] for i in range(n)]
    for i, t in enumerate(out):
        if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
            got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"{who}: {what}[{i}] is {got}, expected {tuple(shape)}")
    return out


def _scale(mv_scale):
    try:
        sx, sy = (float(v) for v in mv_scale)
    except (TypeError, ValueError):
        raise ValueError(f"temporal instability: mv_scale must be (scale_x, scale_y), got "
                         f"{mv_scale!r}") from None
    return sx, sy


def _check_normalize(normalize):
    if normalize not in _NORMALIZE:
        raise ValueError(f"temporal instability: normalize must be 'valid' or 'all', got "
                         f"{normalize!r}")


def _check(frames, motion_vectors, depth, normals, mv_scale, normalize):
    """Host-side argument checks (shapes only: no GPU work, no synchronisation)."""
    _check_normalize(normalize)
    scale = _scale(mv_scale)
    if motion_vectors is None and (depth is not None or normals is not None):
        raise ValueError("temporal instability: depth and normals reject reprojected pixels; "
                         "they need motion_vectors")
    T = len(frames)
    if T == 0 or not torch.is_tensor(frames[0]) or frames[0].dim() != 4:
        raise ValueError("temporal instability: frames must be T tensors [B,C,H,W] or one "
                         "[T,B,C,H,W] tensor")
    B, C, H, W = frames[0].shape
    fr = _seq(frames, "frames", T, (B, C, H, W))
    mv = _seq(motion_vectors, "motion_vectors", T - 1, (B, 2, H, W))
    dz = _seq(depth, "depth", T, (B, 1, H, W))
    nr = _seq(normals, "normals", T, (B, 3, H, W))
    return fr, mv, dz, nr, scale


def _launch_pair(cur, prev, mv, zc, zp, nc, np_, scale, alpha, depth_tol, normal_cos, psum, pcnt):
    B, C, H, W = cur.shape
    call("nsm_temporal_pair", ptr(cur), ptr(prev), ptr(mv), ptr(zc), ptr(zp), ptr(nc), ptr(np_),
         B, C, H, W, scale[0], scale[1], float(alpha), float(depth_tol), float(normal_cos),
         ptr(psum), ptr(pcnt), stream())


def _blocks(shape):
    per = lib.nsm_temporal_blocks(*shape)
    if per <= 0:
        raise ValueError(f"temporal instability: unsupported shape {tuple(shape)} (C*H*W must be "
                         "below 2^31)")
    return per


def _finalize(psum, pcnt, npairs, shape, per, normalize, acc=None):
    B = shape[0]
    dev = psum.device
    sums = torch.empty((npairs, B), dtype=torch.float32, device=dev)
    counts = torch.empty((npairs, B), dtype=torch.int64, device=dev)
    out = torch.empty((), dtype=torch.float32, device=dev)
    n_all = shape[0] * shape[1] * shape[2] * shape[3] if normalize == "all" else 0
    call("nsm_temporal_finalize", ptr(psum), ptr(pcnt), npairs, B, per, n_all, ptr(sums),
         ptr(counts), ptr(out), ptr(acc), stream())
    return out, sums, counts


def _run(frames, motion_vectors, alpha, depth, normals, depth_tol, normal_cos, mv_scale,
         normalize):
    """(value, sums [T-1,B], counts [T-1,B]) of a checked sequence of T >= 2 frames."""
    fr, mv, dz, nr, scale = _check(frames, motion_vectors, depth, normals, mv_scale, normalize)
    dev = require_gpu(fr[0], "temporal-instability frames").device
    shape = tuple(fr[0].shape)
    per = _blocks(shape)
    npairs = len(fr) - 1
    fr = [_f32(f) for f in fr]
    mv = [_f32(m, dev) for m in mv] if mv is not None else None
    dz = [_f32(z, dev) for z in dz] if dz is not None else None
    nr = [_f32(n, dev) for n in nr] if nr is not None else None
    psum = torch.empty((npairs, shape[0], per), dtype=torch.float32, device=dev)
    pcnt = torch.empty((npairs, shape[0], per), dtype=torch.int32, device=dev)
    for t in range(1, len(fr)):
        _launch_pair(fr[t], fr[t - 1], mv[t - 1] if mv else None,
                     dz[t] if dz else None, dz[t - 1] if dz else None,
                     nr[t] if nr else None, nr[t - 1] if nr else None,
                     scale, alpha, depth_tol, normal_cos, psum[t - 1], pcnt[t - 1])
    return _finalize(psum, pcnt, npairs, shape, per, normalize)


def measure_temporal_instability(frames, motion_vectors=None, alpha=5.0, *, depth=None,
                                 normals=None, depth_tol=0.1, normal_cos=0.9,
                                 mv_scale=(1.0, 1.0), normalize="valid"):
    """Mean over consecutive frame pairs of mean(exp(alpha * D) - 1), as a
    device scalar without a host synchronisation (pert_loss.py:166-199).

    frames: T same-shape tensors [B,C,H,W] on the GPU (fp32, fp16 or bf16), or
    one [T,B,C,H,W] tensor. Without `motion_vectors`, D = |f_t - f_{t-1}| and
    the result is the reference's (`nsm_expdiff_mean`, unchanged). With them
    (T-1 tensors [B,2,H,W]; convention and rejection tests in the module
    docstring), D compares each pixel with its reprojected position in the
    previous frame, the paper's Eq. 3, which the reference leaves as a stub that
    raises. `alpha` defaults to the reference's 5.0; the paper uses 3.

    `normalize` is what a pair's sum over the batch is divided by: "valid" (the
    default) by the number of surviving elements over the batch (0 for a pair in
    which nothing survives), "all" by B*C*H*W, the paper's literal P. "valid" is
    the default because with "all" every rejected pixel counts as a perfectly
    stable one: a sequence with more disocclusion, or a faster camera, reads as
    MORE stable, and figures of sequences with different motion cannot be
    compared. `temporal_instability_terms` returns what any other normalisation
    needs.

    depth / normals without motion_vectors, wrong lengths and wrong shapes raise
    ValueError before any GPU work."""
    _check_normalize(normalize)
    if motion_vectors is None:
        if depth is not None or normals is not None:
            raise ValueError("temporal instability: depth and normals reject reprojected pixels; "
                             "they need motion_vectors")
        if len(frames) < 2:
            return torch.tensor(0.0)
        dev = frames[0].device
        require_gpu(frames[0], "temporal-instability frames")
        n = frames[0].numel()
        partial = torch.empty(lib.nsm_loss_blocks(n), dtype=torch.float32, device=dev)
        total = torch.zeros((), dtype=torch.float32, device=dev)
        for t in range(1, len(frames)):
            a = frames[t].detach().contiguous().to(torch.float32)
            b = frames[t - 1].detach().contiguous().to(torch.float32)
            out = torch.empty((), dtype=torch.float32, device=dev)
            call("nsm_expdiff_mean", ptr(a), ptr(b), n, float(alpha), ptr(partial), ptr(out),
                 stream())
            total = total + out
        return total / (len(frames) - 1)
    if len(frames) < 2:
        _check(frames, motion_vectors, depth, normals, mv_scale, normalize)
        return torch.tensor(0.0)
    return _run(frames, motion_vectors, alpha, depth, normals, depth_tol, normal_cos, mv_scale,
                normalize)[0]


def temporal_instability_terms(frames, motion_vectors=None, alpha=5.0, *, depth=None,
                               normals=None, depth_tol=0.1, normal_cos=0.9,
                               mv_scale=(1.0, 1.0), normalize="valid"):
    """(sums [T-1,B] fp32, valid [T-1,B] int64) on the device: per frame pair and
    image the sum of exp(alpha * D) - 1 over the surviving elements and their
    number (pixels times C), so that any normalisation can be formed without a
    second pass. Same arguments as measure_temporal_instability (`normalize`
    does not change the terms); without motion_vectors nothing moves and
    nothing is rejected. No host synchronisation."""
    if len(frames) < 2:
        fr = _check(frames, motion_vectors, depth, normals, mv_scale, normalize)[0]
        dev, B = fr[0].device, fr[0].shape[0]
        return (torch.zeros((0, B), dtype=torch.float32, device=dev),
                torch.zeros((0, B), dtype=torch.int64, device=dev))
    _, sums, counts = _run(frames, motion_vectors, alpha, depth, normals, depth_tol, normal_cos,
                           mv_scale, normalize)
    return sums, counts


def reproject(prev, motion_vectors, mv_scale=(1.0, 1.0)):
    """(warped [B,C,H,W] fp32, valid [B,1,H,W] bool): `prev` sampled bilinearly at
    each pixel's motion-vector adjusted position (the lookup of
    measure_temporal_instability, from the same device function), 0 where the
    position is not finite or outside the image, and whether it was inside.
    No host synchronisation."""
    scale = _scale(mv_scale)
    if not torch.is_tensor(prev) or prev.dim() != 4:
        raise ValueError("reproject: prev must be a [B,C,H,W] tensor")
    B, C, H, W = prev.shape
    if not torch.is_tensor(motion_vectors) or tuple(motion_vectors.shape) != (B, 2, H, W):
        got = tuple(motion_vectors.shape) if torch.is_tensor(motion_vectors) else None
        raise ValueError(f"reproject: motion_vectors is {got}, expected {(B, 2, H, W)}")
    dev = require_gpu(prev, "reproject input").device
    _blocks((B, C, H, W))
    p, m = _f32(prev), _f32(motion_vectors, dev)
    out = torch.empty_like(p)
    valid = torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev)
    call("nsm_reproject", ptr(p), ptr(m), B, C, H, W, scale[0], scale[1], ptr(out), ptr(valid),
         stream())
    return out, valid.view(torch.bool)


class TemporalInstability:
    """measure_temporal_instability for sequences too long to hold: feed the
    frames one by one.

    update(frame, motion_vectors=None, depth=None, normals=None) compares `frame`
    with the previous one (`motion_vectors` maps this frame into the previous
    one; the first frame's are ignored), adds the pair's value to a device
    accumulator in double and keeps its own copy of the frame (and of its depth
    and normals): no host synchronisation. compute() reads the accumulator (one
    synchronisation) and returns the mean of the pair values so far as a float,
    0.0 before the second frame; reset() starts a new sequence. Fed the same
    sequence with motion vectors it returns measure_temporal_instability's value
    bit for bit. Without motion vectors a pair goes through the same kernel with
    no motion (the list form keeps the reference's `nsm_expdiff_mean` path there,
    which rounds each pair to fp32: equal to rounding, not bitwise).
    `device=` allocates the accumulator at construction, which an update()
    captured in a graph needs (the first frame is given outside the capture)."""

    def __init__(self, alpha=5.0, *, depth_tol=0.1, normal_cos=0.9, mv_scale=(1.0, 1.0),
                 normalize="valid", device=None):
        _check_normalize(normalize)
        self.alpha, self.depth_tol, self.normal_cos = float(alpha), float(depth_tol), float(normal_cos)
        self.mv_scale, self.normalize = _scale(mv_scale), normalize
        self._acc = torch.zeros(2, dtype=torch.float64, device=device) if device is not None else None
        self._prev = self._prev_depth = self._prev_normals = None
        self._have = (False, False, False)   # a previous frame / depth / normals is held

    def reset(self):
        if self._acc is not None:
            self._acc.zero_()
        self._have = (False, False, False)

    @staticmethod
    def _keep(buf, t):
        if buf is None or buf.shape != t.shape or buf.device != t.device:
            return t.clone()
        return buf.copy_(t)

    def update(self, frame, motion_vectors=None, depth=None, normals=None):
        if not torch.is_tensor(frame) or frame.dim() != 4:
            raise ValueError("TemporalInstability: frame must be a [B,C,H,W] tensor")
        B, C, H, W = frame.shape
        for what, t, ch in (("motion_vectors", motion_vectors, 2), ("depth", depth, 1),
                            ("normals", normals, 3)):
            if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != (B, ch, H, W)):
                got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
                raise ValueError(f"TemporalInstability: {what} is {got}, expected {(B, ch, H, W)}")
        have, have_z, have_n = self._have
        if have:
            if tuple(self._prev.shape) != (B, C, H, W):
                raise ValueError(f"TemporalInstability: frame is {(B, C, H, W)}, the previous one "
                                 f"was {tuple(self._prev.shape)}")
            if motion_vectors is None and (depth is not None or normals is not None):
                raise ValueError("TemporalInstability: depth and normals reject reprojected "
                                 "pixels; they need motion_vectors")
            if (depth is not None and not have_z) or (normals is not None and not have_n):
                raise ValueError("TemporalInstability: depth / normals must come with every "
                                 "frame of a sequence, the previous frame had none")
        dev = require_gpu(frame, "temporal-instability frame").device
        per = _blocks((B, C, H, W))
        cur = _f32(frame)
        z = _f32(depth, dev) if depth is not None else None
        nr = _f32(normals, dev) if normals is not None else None
        if self._acc is None or self._acc.device != dev:
            self._acc = torch.zeros(2, dtype=torch.float64, device=dev)
        if have:
            mv = _f32(motion_vectors, dev) if motion_vectors is not None else None
            psum = torch.empty((1, B, per), dtype=torch.float32, device=dev)
            pcnt = torch.empty((1, B, per), dtype=torch.int32, device=dev)
            _launch_pair(cur, self._prev, mv, z, self._prev_depth if z is not None else None,
                         nr, self._prev_normals if nr is not None else None, self.mv_scale,
                         self.alpha, self.depth_tol, self.normal_cos, psum, pcnt)
            _finalize(psum, pcnt, 1, (B, C, H, W), per, self.normalize, acc=self._acc)
        self._prev = self._keep(self._prev, cur)
        if z is not None:
            self._prev_depth = self._keep(self._prev_depth, z)
        if nr is not None:
            self._prev_normals = self._keep(self._prev_normals, nr)
        self._have = (True, z is not None, nr is not None)

    def compute(self):
        if self._acc is None:
            return 0.0
        total, n = self._acc.cpu().tolist()
        if n == 0:
            return 0.0
        return torch.tensor(total / n, dtype=torch.float64).to(torch.float32).item()
