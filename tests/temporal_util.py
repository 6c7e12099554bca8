"""The temporal-instability metric with motion-vector reprojection (the paper's
Eq. 3) restated with plain torch indexing: the comparator of
test_temporal_ref.py and test_gpu_temporal.py. Evaluated in float64 on inputs
first rounded to float32; `dtype=torch.float32` is the same arithmetic a user
would otherwise run on ATen ops, and its own error against float64 is the
yardstick of the GPU tests.

Convention (include/nsm.h): pixel (x, y) of image b looks up the previous frame
at (x + mv[b,0,y,x] * sx, y + mv[b,1,y,x] * sy), pixel units, channel 0 along
the width, integer coordinates = pixel centres (align_corners=True), bilinear.
Rejected: a position that is not finite or outside [0, W-1] x [0, H-1]
(inclusive); with depth, !(|z_t - z~| <= depth_tol |z_t|); with normals,
!(dot(n_t, n~) >= normal_cos), n~ not renormalised."""
import torch

T = 4
# ragged width and partial waves; several channels and a width under one
# vector; several blocks per image with odd sizes
SHAPES = [(2, 1, 19, 37), (1, 3, 8, 5), (2, 1, 67, 129)]
FAMILIES = ("grid", "gauss")     # motion vectors on a 1/8-pixel grid, |mv| <= 5; N(0, 2.5 px)
DEPTH_TOL, NORMAL_COS = 0.3, 0.2
MARGIN = 1e-4          # no decision margin of a seeded case may be smaller
REPAIR = 10 * MARGIN   # inputs() moves a closer draw to a clear verdict (_repair)
# one seed per case (default 5); test_temporal_ref.test_decision_margins holds
# every case to MARGIN: a seed under it is replaced here, the cap stays
SEEDS = {}


def seed_of(shape, family):
    return SEEDS.get((shape, family), 5)


def inputs(shape, family, seed=None):
    """float32 frames (T x [B,C,H,W] in [0, 1]), motion vectors (T-1 x [B,2,H,W]),
    depth (T x [B,1,H,W] in [1, 2]) and unit normals (T x [B,3,H,W])."""
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(seed_of(shape, family) if seed is None else seed)
    frames = [torch.rand(shape, generator=gen) for _ in range(T)]
    if family == "grid":
        mvs = [torch.randint(-40, 41, (B, 2, H, W), generator=gen).float() / 8 for _ in range(T - 1)]
    else:
        mvs = [2.5 * torch.randn((B, 2, H, W), generator=gen) for _ in range(T - 1)]
    depth = [1 + torch.rand((B, 1, H, W), generator=gen) for _ in range(T)]
    normals = []
    for _ in range(T):
        n = 0.6 * torch.randn((B, 3, H, W), generator=gen)
        n[:, 2] += 1
        normals.append(n / n.norm(dim=1, keepdim=True))
    _repair(mvs, depth, normals)
    return frames, mvs, depth, normals


def _repair(mvs, depth, normals):
    """Move the few near-ties of a drawn case (in place) away from their verdict.
    With tens of thousands of pixels and three tests each, some draw always
    lands within MARGIN of a threshold, whatever the seed: every pixel closer
    than REPAIR = 10 x MARGIN (judged in float64) is moved to a clear verdict.
      border: a position within REPAIR of x = 0 / W-1 (y = 0 / H-1), exactly on
        it for the 1/8-pixel grid, moves 1/8 pixel inside (it stays on the grid;
        the inclusive bounds themselves are what the translation test pins);
      depth: z_t(p) becomes the interpolated previous depth (accepted, margin
        depth_tol |z|);
      normal: n_t(p) is negated (margin -> -margin - 2 normal_cos).
    z_t and n_t are also pair t+1's previous frame, so the pairs are repaired
    in order, each after the frames it reads as `previous` are final."""
    B, _, H, W = mvs[0].shape
    x = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    y = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    for t in range(1, T):
        m = mvs[t - 1]
        for ch, pos, hi in ((0, x, W - 1), (1, y, H - 1)):
            p = pos + m[:, ch].double()
            m[:, ch] += 0.125 * (p.abs() < REPAIR).float() - 0.125 * ((p - hi).abs() < REPAIR).float()
        _, taps, _ = lookup(m)
        zs = sample(depth[t - 1].double(), taps)
        z = depth[t].double()
        tie = (DEPTH_TOL * z.abs() - (z - zs).abs()).abs() < REPAIR
        depth[t][tie] = zs.float()[tie]
        dot = (normals[t].double() * sample(normals[t - 1].double(), taps)).sum(1, keepdim=True)
        tie = ((dot - NORMAL_COS).abs() < REPAIR).expand_as(normals[t])
        normals[t][tie] = -normals[t][tie]


def translation_case(shape=(2, 1, 19, 37), dx=3, dy=-2, seed=0):
    """Frame t is frame t-1 rolled by (dx, dy); the motion vectors are (-dx, -dy)."""
    gen = torch.Generator().manual_seed(seed)
    frames = [torch.rand(shape, generator=gen)]
    for _ in range(T - 1):
        frames.append(torch.roll(frames[-1], shifts=(dy, dx), dims=(2, 3)))
    mv = torch.empty(shape[0], 2, *shape[2:])
    mv[:, 0], mv[:, 1] = -dx, -dy
    return frames, [mv.clone() for _ in range(T - 1)]


def lookup(mv, scale=(1.0, 1.0), dtype=torch.float64):
    """Positions and taps of mv [B,2,H,W]: (ok [B,H,W] bool, taps, border margin
    [B,H,W]: distance to the nearest image border, negative outside)."""
    B, _, H, W = mv.shape
    m = mv.to(dtype)
    px = torch.arange(W, dtype=dtype).view(1, 1, W) + m[:, 0] * scale[0]
    py = torch.arange(H, dtype=dtype).view(1, H, 1) + m[:, 1] * scale[1]
    ok = torch.isfinite(px) & torch.isfinite(py) & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    margin = torch.minimum(torch.minimum(px, (W - 1) - px), torch.minimum(py, (H - 1) - py))
    cx, cy = torch.where(ok, px, torch.zeros_like(px)), torch.where(ok, py, torch.zeros_like(py))
    x0 = cx.floor().clamp(0, max(W - 2, 0)).long()
    y0 = cy.floor().clamp(0, max(H - 2, 0)).long()
    fx, fy = cx - x0.to(dtype), cy - y0.to(dtype)
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    return ok, (x0, x1, y0, y1, fx, fy), margin


def sample(img, taps):
    """Bilinear sample of img [B,C,H,W] (already in the working dtype) at taps."""
    x0, x1, y0, y1, fx, fy = taps
    B, C = img.shape[:2]
    b = torch.arange(B).view(B, 1, 1, 1)
    c = torch.arange(C).view(1, C, 1, 1)
    x0, x1, y0, y1, fx, fy = (t.unsqueeze(1) for t in (x0, x1, y0, y1, fx, fy))
    return ((1 - fy) * (1 - fx) * img[b, c, y0, x0] + (1 - fy) * fx * img[b, c, y0, x1]
            + fy * (1 - fx) * img[b, c, y1, x0] + fy * fx * img[b, c, y1, x1])


def pair(cur, prev, mv, alpha, zc=None, zp=None, nc=None, np_=None, depth_tol=DEPTH_TOL,
         normal_cos=NORMAL_COS, scale=(1.0, 1.0), dtype=torch.float64):
    """One frame pair: dict of per-image sums [B] (dtype), surviving element
    counts [B] (int64), sum of exp(alpha D) over the survivors [B], the final
    mask [B,H,W] and the decision margins (border, depth, normal; the latter two
    over the pixels whose position is inside)."""
    C = cur.shape[1]
    ok, taps, border = lookup(mv, scale, dtype)
    margins = {"border": border[torch.isfinite(border)].abs().min().item()}
    keep = ok.clone()
    if zc is not None:
        z = zc.to(dtype)[:, 0]
        m = depth_tol * z.abs() - (z - sample(zp.to(dtype), taps)[:, 0]).abs()
        keep &= m >= 0
        margins["depth"] = m[ok].abs().min().item() if ok.any() else float("inf")
    if nc is not None:
        m = (nc.to(dtype) * sample(np_.to(dtype), taps)).sum(1) - normal_cos
        keep &= m >= 0
        margins["normal"] = m[ok].abs().min().item() if ok.any() else float("inf")
    d = (cur.to(dtype) - sample(prev.to(dtype), taps)).abs()
    e = torch.exp(alpha * d) * keep.unsqueeze(1)
    return dict(sums=(e - keep.unsqueeze(1).to(dtype)).flatten(1).sum(1), exps=e.flatten(1).sum(1),
                counts=keep.flatten(1).sum(1) * C, keep=keep, margins=margins)


def sequence(frames, mvs, alpha, depth=None, normals=None, dtype=torch.float64, **kw):
    """(sums [T-1,B], counts [T-1,B], exps [T-1,B], margins of every pair)."""
    ps = [pair(frames[t], frames[t - 1], mvs[t - 1], alpha,
               *((depth[t], depth[t - 1]) if depth is not None else (None, None)),
               *((normals[t], normals[t - 1]) if normals is not None else (None, None)),
               dtype=dtype, **kw) for t in range(1, len(frames))]
    return (torch.stack([p["sums"] for p in ps]), torch.stack([p["counts"] for p in ps]),
            torch.stack([p["exps"] for p in ps]), [p["margins"] for p in ps])


def value(sums, counts, normalize, n_all):
    """Mean over the pairs of sum over the batch / divisor (0 when it is 0), in float64."""
    s = sums.double().sum(1)
    den = counts.sum(1).double() if normalize == "valid" else torch.full_like(s, float(n_all))
    return torch.where(den > 0, s / den.clamp_min(1), torch.zeros_like(s)).mean().item()


_REF = {}


def reference(shape, family, reject, alpha):
    """A case computed once, shared, read-only: (inputs, float64 (sums, counts,
    exps, margins), float32 restatement (sums, counts, exps, margins))."""
    key = (shape, family, reject, alpha)
    if key not in _REF:
        frames, mvs, depth, normals = data = inputs(shape, family)
        kw = dict(depth=depth, normals=normals) if reject else {}
        _REF[key] = (data, sequence(frames, mvs, alpha, **kw),
                     sequence(frames, mvs, alpha, dtype=torch.float32, **kw))
    return _REF[key]


def floor_rel(shape, family, mvs, sums, exps, alpha):
    """The derived relative floor of a per-(pair, image) sum [T-1,B]: 1e-6, the
    rtol of test_l1_loss (on the 1/8-pixel grid with |mv| <= 5 the coordinates
    and weights are exact in float32 and the arithmetic is that test's); for
    Gaussian motion vectors plus alpha * 2 delta * sum(exp(alpha D)) / sum, delta
    = 2^-23 (W - 1 + max|mv|): the coordinate rounding times the largest slope
    of a bilinear surface over values in [0, 1]."""
    f = torch.full_like(sums, 1e-6)
    if family == "gauss":
        W = shape[3]
        for p, m in enumerate(mvs):
            delta = 2.0 ** -23 * (W - 1 + m.abs().max().item())
            f[p] += alpha * 2 * delta * exps[p] / sums[p].clamp_min(1e-300)
    return f
