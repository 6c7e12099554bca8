"""The temporal anti-aliasing resolve (nsm_taa_resolve, nsm_amd/taa.py)
restated with plain torch indexing on temporal_util's lookup: the comparator of
test_taa_ref.py and test_gpu_taa.py. Evaluated in float64 on inputs first
rounded to float32; `dtype=torch.float32` is the same arithmetic on ATen ops,
and its own error against float64 is the yardstick of the GPU tests.

    O_0 = I_0
    h   = bilinear sample of O_{t-1} at m(p)   (temporal_util.lookup / sample)
    h   = min(max(h, lo), hi), lo / hi = min / max of I_t over the 3x3
          neighbourhood with replicated edges               (clamp)
    O_t = accepted ? I_t + (1 - blend) (h - I_t) : I_t
accepted: the position, depth and normal tests of temporal_util, depth and
normals of the previous INPUT frame. No reference implementation exists (the
reference repository has no TAA), so nothing here comes from a fixture."""
import torch
import torch.nn.functional as F

from temporal_util import (DEPTH_TOL, FAMILIES, NORMAL_COS, SHAPES, T, inputs, lookup,  # noqa: F401
                           sample, translation_case)

BLENDS = (0.1, 0.5)
CASES = [(s, f, r, c, b) for f in FAMILIES for r in (False, True) for s in SHAPES
         for c in (True, False) for b in BLENDS]
IDS = [f"{f}-{'reject' if r else 'position'}-{'clamp' if c else 'noclamp'}-b{b}-"
       + "x".join(map(str, s)) for s, f, r, c, b in CASES]


def bounds(img):
    """(lo, hi) of img [B,C,H,W] over each pixel's 3x3 neighbourhood, edges replicated."""
    p = F.pad(img, (1, 1, 1, 1), mode="replicate")
    return -F.max_pool2d(-p, 3, stride=1), F.max_pool2d(p, 3, stride=1)


def resolve(frames, mvs=None, depth=None, normals=None, blend=0.1, clamp=True,
            depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS, scale=(1.0, 1.0), dtype=torch.float64):
    """(resolved frames: T x [B,C,H,W] in dtype, accepted: T x [B,1,H,W] bool,
    clamped: T x share of the pixels whose history the clamp changed)."""
    # blend reaches the kernel as a float32; 1 - blend is formed in the working type
    keep = 1 - torch.tensor(blend, dtype=torch.float32).to(dtype)
    B, C, H, W = frames[0].shape
    out = [frames[0].to(dtype)]
    acc = [torch.zeros(B, 1, H, W, dtype=torch.bool)]
    changed = [0.0]
    for t in range(1, len(frames)):
        cur = frames[t].to(dtype)
        mv = mvs[t - 1] if mvs is not None else torch.zeros(B, 2, H, W)
        ok, taps, _ = lookup(mv, scale, dtype)
        if depth is not None:
            z = depth[t].to(dtype)[:, 0]
            ok = ok & ((z - sample(depth[t - 1].to(dtype), taps)[:, 0]).abs() <= depth_tol * z.abs())
        if normals is not None:
            ok = ok & ((normals[t].to(dtype) * sample(normals[t - 1].to(dtype), taps)).sum(1)
                       >= normal_cos)
        h = sample(out[t - 1], taps)
        if clamp:
            lo, hi = bounds(cur)
            hc = torch.minimum(torch.maximum(h, lo), hi)
            changed.append((hc != h).float().mean().item())
            h = hc
        else:
            changed.append(0.0)
        ok = ok.unsqueeze(1)
        out.append(torch.where(ok, cur + keep * (h - cur), cur))
        acc.append(ok)
    return out, acc, changed


_REF = {}


def reference(shape, family, reject, clamp, blend):
    """A case computed once, shared, read-only: (inputs, float64 (frames,
    accepted, clamped), float32 restatement (frames, accepted, clamped))."""
    key = (shape, family, reject, clamp, blend)
    if key not in _REF:
        frames, mvs, depth, normals = data = inputs(shape, family)
        kw = dict(depth=depth, normals=normals) if reject else {}
        _REF[key] = (data, resolve(frames, mvs, blend=blend, clamp=clamp, **kw),
                     resolve(frames, mvs, blend=blend, clamp=clamp, dtype=torch.float32, **kw))
    return _REF[key]


def floor_abs(shape, family, mvs, blend, t):
    """The derived absolute floor of frame t's error:
        (2^-21 + 2 delta) * sum_{k<t} (1 - blend)^k.
    2^-21: the handful of roundings of a bilinear sample and one fma on values
    in [0, 1]; delta = 2^-23 (W - 1 + max|mv|) for Gaussian motion vectors (the
    coordinate rounding of temporal_util.floor_rel, times the largest slope of a
    bilinear surface over values in [0, 1]; 0 on the 1/8-pixel grid, where
    coordinates and weights are exact in float32), max|mv| over the pairs up to
    t; the geometric sum: an earlier frame's error passes through a convex
    sample and a 1-Lipschitz clamp and is scaled by 1 - blend."""
    delta = 0.0
    if t and family == "gauss" and mvs is not None:
        delta = 2.0 ** -23 * (shape[3] - 1 + max(m.abs().max().item() for m in mvs[:t]))
    return (2.0 ** -21 + 2 * delta) * sum((1 - blend) ** k for k in range(t))


def bound(ref64, ref32, shape, family, mvs, blend, t):
    """What frame t may be off by: max(2 x the float32 restatement's worst error
    on that frame, the floor); and that worst error."""
    e32 = (ref32[t].double() - ref64[t]).abs().max().item()
    return max(2 * e32, floor_abs(shape, family, mvs, blend, t)), e32


def constant_case(shape=(1, 2, 9, 11)):
    """A 0/1 checkerboard followed by a constant 0.5 frame, no motion."""
    B, C, H, W = shape
    y, x = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    board = ((x + y) % 2).float().expand(B, C, H, W).contiguous()
    return [board, torch.full(shape, 0.5)]


NOISE_T = 8


def noise_case(seed=3, shape=(1, 1, 67, 129), sigma=0.05):
    """Figure 6's axis in the small: a smooth seeded image plus iid N(0, sigma)
    noise per frame, NOISE_T frames, no motion."""
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    ph = 6.28 * torch.rand(4, generator=gen)
    y = torch.arange(H, dtype=torch.float32).view(H, 1)
    x = torch.arange(W, dtype=torch.float32).view(1, W)
    img = 0.5 + 0.2 * torch.sin(x / 17 + ph[0]) * torch.cos(y / 11 + ph[1]) \
        + 0.1 * torch.sin(x / 5 + y / 7 + ph[2])
    img = img.expand(B, C, H, W)
    return [(img + sigma * torch.randn(shape, generator=gen)).contiguous() for _ in range(NOISE_T)]
