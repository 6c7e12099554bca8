"""The SVGF denoiser (nsm_svgf_accumulate / _variance / _atrous, nsm_amd/svgf.py)
restated with plain torch indexing on temporal_util's lookup: the comparator of
test_svgf_ref.py and test_gpu_svgf.py. Evaluated in float64 on inputs first
rounded to float32; `dtype=torch.float32` is the same arithmetic on ATen ops,
and its own error against float64 is the yardstick of the GPU tests. No
reference implementation exists (the reference repository has no SVGF), so
nothing here comes from a fixture. The definition is in include/nsm.h:

    grad z(p)   central differences, edges replicated, 0 along an axis of length 1
    e_z(p, q) = |z_p - z_q| / (sigma_z |grad z(p) . (q - p)| + 1e-8)
    w_n(p, q) = max(0, n_p . n_q)^sigma_n
    accumulate  N = min(hN + 1, max_history) at the nearest tap, a = max(alpha, 1/N),
                c' = c + (1 - a)(h_c - c), likewise m1, m2 with a_m; rejected or
                first frame: N = 1, c' = c, m1 = l, m2 = l^2; var = max(0, m2 - m1^2)
    variance    N < min_history: 7x7 means weighted by exp(-e_z) w_n (centre 1),
                var = max(0, M2 - M1^2) min_history / N
    a-trous     taps p + s (dx, dy), h = (1/16, 1/4, 3/8, 1/4, 1/16), centre h(0)^2,
                w = h h exp(-e_z - |l_p - l_q| / phi_l) w_n,
                phi_l = sigma_l sqrt(max(g3x3(var), 0) + 1e-10),
                c' = sum w c / sum w, var' = sum w^2 var / (sum w)^2
Every scalar parameter reaches the kernels as a float32 and is rounded so here.

Floors (what a result may be off by whatever the float32 restatement happens
to err by), u = 2^-24. All seeded motion vectors lie on the 1/8-pixel grid with
|mv| <= 5, where positions, bilinear weights and the nearest-tap rounding are
exact in float32: the coordinate rounding contributes nothing, the floors come
from the operation count alone.
  a spatial pass, colour: the result is a convex combination of values in
    [0, 1], so a relative error rho on every weight moves it by at most rho.
    A weight is exp(E), E = sigma_n log(dot) - e_z - dl / phi: the dot product
    of unit normals carries 3 roundings that matter (3 u sigma_n on E where the
    weight is not negligible, dot ~ 1); the other terms are about 16 roundings
    relative to their own size x, and x exp(-x) <= 0.37, plus an exponential
    good to 2 ulp: 8 u. The sum of up to 49 non-negative terms and the division:
    27 u on numerator and denominator.  floor_color = u (3 sigma_n + 35).
  accumulate: 2^-21, the handful of roundings of a bilinear sample and one fma
    on values in [0, 1] (taa_util.floor_abs); the variance m2 - m1^2 likewise.
  variance pass, variance: M1 and M2 are such means (floor_color each), M1^2
    doubles M1's, and min_history / N is at most min_history: 3 min_history
    floor_color.
  a-trous, variance: sum w^2 var / (sum w)^2 carries twice a weight's relative
    error: 2 floor_color max(var).
  the recurrence: the errors of a frame's passes add (each pass is a convex
    combination of its colour input for fixed weights), and what the history
    carries over is scaled by 1 - alpha per frame: the geometric sum of
    taa_util.floor_abs. The dependence of the weights on the colour through
    the luminance term is of second order and left to the 2 x float32 rule."""
import functools

import torch

import temporal_util as U
from temporal_util import DEPTH_TOL, MARGIN, NORMAL_COS, REPAIR, SHAPES, lookup, sample  # noqa: F401

T = 6
FAMILIES = ("planes", "random")
H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
SIGMA_NOISE = 0.15


def velocity(shape):
    """Pixels per frame by which the "planes" scene moves (on the 1/8-pixel
    grid, off the nearest-tap tie); slower on an image a few pixels wide, so
    that a history can outgrow min_history there too."""
    return (1.25, -0.75) if shape[3] >= 16 else (0.25, -0.125)


# the issue's defaults; "cap" has max_history = min_history = 4, so the cap binds
# from the fourth frame on (CAP_CASE is the one case that runs with it)
CAP_CASE = ((2, 1, 19, 37), "planes")
PARAMS = dict(iterations=5, alpha=0.2, moments_alpha=0.2, max_history=32, min_history=4,
              feedback=1, sigma_z=1.0, sigma_n=128.0, sigma_l=4.0)
CAP = dict(PARAMS, max_history=4)
U24 = 2.0 ** -24


def single_thread(fn):
    """Run fn on one CPU thread: the restatement is thousands of small tensor
    operations, which a thread pool slows down several times."""
    @functools.wraps(fn)
    def run(*a, **kw):
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            return fn(*a, **kw)
        finally:
            torch.set_num_threads(n)
    return run


def c32(v, dtype):
    """A scalar as the kernel receives it: rounded to float32, then widened."""
    return torch.tensor(float(v), dtype=torch.float32).to(dtype)


# ---- seeded inputs ------------------------------------------------------------
def _repair(mvs, depth, normals):
    """temporal_util._repair for any number of frames, plus the nearest-tap
    rounding: a position whose fraction is within REPAIR of 0.5 (exactly on it
    for the 1/8-pixel grid) moves 1/8 pixel on, which keeps it on the grid, on
    the same side of every border and off the border itself."""
    B, _, H, W = mvs[0].shape
    x = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    y = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    for t in range(1, len(mvs) + 1):
        m = mvs[t - 1]
        for ch, pos, hi in ((0, x, W - 1), (1, y, H - 1)):
            p = pos + m[:, ch].double()
            m[:, ch] += 0.125 * (((p - p.floor()) - 0.5).abs() < REPAIR).float()
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


def random_inputs(shape, seed=5):
    """temporal_util.inputs on the 1/8-pixel grid, two draws joined into T frames."""
    a, b = U.inputs(shape, "grid", seed), U.inputs(shape, "grid", seed + 1)
    frames, mvs, depth, normals = ([t.clone() for t in (x + y)] for x, y in zip(a, b))
    frames, depth, normals = frames[:T], depth[:T], normals[:T]
    mvs = mvs[:T - 1]
    _repair(mvs, depth, normals)
    return frames, mvs, depth, normals, None


def planes_inputs(shape, seed=7):
    """Two planar depth regions meeting at a slanted edge, one normal per region
    plus noise of sigma 0.02 (renormalised), a smooth penumbra signal plus
    Gaussian noise of SIGMA_NOISE clipped to [0, 1]; the scene moves by velocity()
    pixels per frame and the motion vectors say so. Returns (frames, mvs, depth,
    normals, clean)."""
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    L = float(max(H, W))
    vel = velocity(shape)
    tint = torch.tensor([1.0, 0.9, 0.8][:C]).view(1, C, 1, 1)
    n0 = torch.tensor([0.2, 0.1, 1.0])
    n1 = torch.tensor([-0.5, 0.3, 0.8])
    frames, depth, normals, clean = [], [], [], []
    for t in range(T):
        u = (torch.arange(W, dtype=torch.float64) - t * vel[0]).view(1, 1, 1, W)
        v = (torch.arange(H, dtype=torch.float64) - t * vel[1]).view(1, 1, H, 1)
        side = ((u - W / 2) * 0.94 + (v - H / 2) * 0.34) > 0.05
        z = torch.where(side, 3.5 - 0.009 * u + 0.0172 * v, 1.2 + 0.013 * u + 0.0071 * v)
        depth.append(z.expand(B, 1, H, W).float().contiguous())
        n = torch.where(side.expand(1, 3, H, W), n1.view(1, 3, 1, 1), n0.view(1, 3, 1, 1))
        n = n.expand(B, 3, H, W) + 0.02 * torch.randn((B, 3, H, W), generator=gen)
        normals.append((n / n.norm(dim=1, keepdim=True)).contiguous())
        s = 0.5 + 0.2 * torch.tanh((0.8 * (u - 0.45 * W) + 0.6 * (v - 0.5 * H)) / (0.3 * L))
        s = (s.float() * tint).expand(B, C, H, W).contiguous()
        clean.append(s)
        frames.append((s + SIGMA_NOISE * torch.randn(shape, generator=gen)).clamp(0, 1))
    mv = torch.empty(B, 2, H, W)
    mv[:, 0], mv[:, 1] = -vel[0], -vel[1]
    mvs = [mv.clone() for _ in range(T - 1)]
    _repair(mvs, depth, normals)
    return frames, mvs, depth, normals, clean


def edge_side(shape):
    """The region of every pixel of frame 0 of planes_inputs: [H,W] bool."""
    _, _, H, W = shape
    u = torch.arange(W, dtype=torch.float64).view(1, W)
    v = torch.arange(H, dtype=torch.float64).view(H, 1)
    return ((u - W / 2) * 0.94 + (v - H / 2) * 0.34) > 0.05


def inputs(shape, family):
    return planes_inputs(shape) if family == "planes" else random_inputs(shape)


# ---- the definition -----------------------------------------------------------
def luminance(c):
    """[B,C,H,W] -> [B,H,W]"""
    if c.shape[1] == 1:
        return c[:, 0]
    k = [c32(v, c.dtype) for v in (0.2126, 0.7152, 0.0722)]
    return k[0] * c[:, 0] + k[1] * c[:, 1] + k[2] * c[:, 2]


def gradient(z):
    """z [B,H,W] -> (gx, gy)"""
    H, W = z.shape[-2:]
    xp, xm = torch.arange(W).add(1).clamp(max=W - 1), torch.arange(W).sub(1).clamp(min=0)
    yp, ym = torch.arange(H).add(1).clamp(max=H - 1), torch.arange(H).sub(1).clamp(min=0)
    dx, dy = (xp - xm).to(z.dtype), (yp - ym).to(z.dtype).view(H, 1)
    gx = (z[:, :, xp] - z[:, :, xm]) / dx.clamp(min=1) if W > 1 else torch.zeros_like(z)
    gy = (z[:, yp] - z[:, ym]) / dy.clamp(min=1) if H > 1 else torch.zeros_like(z)
    return gx, gy


def shifted(img, ox, oy):
    """img [B,K,H,W] read at p + (ox, oy) (0 where that is outside: such a tap
    has weight 0), and which taps are inside the image [H,W]."""
    H, W = img.shape[-2:]
    ys, xs = torch.arange(H) + oy, torch.arange(W) + ox
    inside = ((ys >= 0) & (ys < H)).view(H, 1) & ((xs >= 0) & (xs < W)).view(1, W)
    out = torch.zeros_like(img)
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 < y1 and x0 < x1:
        out[:, :, y0:y1, x0:x1] = img[:, :, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out, inside


def edge_weight_terms(z, n, grad, ox, oy, sigma_z, sigma_n):
    """(e_z [B,H,W], w_n [B,H,W], inside [H,W]) of the tap at offset (ox, oy)."""
    dt = z.dtype
    zq, inside = shifted(z, ox, oy)
    nq, _ = shifted(n, ox, oy)
    gx, gy = grad
    ez = (z[:, 0] - zq[:, 0]).abs() / (c32(sigma_z, dt) * (gx * ox + gy * oy).abs() + c32(1e-8, dt))
    dot = n[:, 0] * nq[:, 0] + n[:, 1] * nq[:, 1] + n[:, 2] * nq[:, 2]
    return ez, dot.clamp(min=0) ** c32(sigma_n, dt), inside


def gauss3(v):
    p = torch.nn.functional.pad(v, (1, 1, 1, 1), mode="replicate")
    H, W = v.shape[-2:]
    k = ((1 / 16, 1 / 8, 1 / 16), (1 / 8, 1 / 4, 1 / 8), (1 / 16, 1 / 8, 1 / 16))
    return sum(k[j][i] * p[:, :, j:j + H, i:i + W] for j in range(3) for i in range(3))


@single_thread
def atrous(color, var, depth, normals, step=1, sigma_z=1.0, sigma_n=128.0, sigma_l=4.0,
           dtype=torch.float64):
    """One iteration: (color', var' or None, share of the in-image non-centre
    taps whose weight exceeds 1e-3 h(dx) h(dy))."""
    c, z, n = color.to(dtype), depth.to(dtype), normals.to(dtype)
    lum = var is not None and sigma_l != 0
    v = var.to(dtype) if lum else None
    grad, l = gradient(z[:, 0]), luminance(c)
    if lum:
        phi = c32(sigma_l, dtype) * torch.sqrt(gauss3(v)[:, 0].clamp(min=0) + c32(1e-10, dtype))
    w0 = H5[2] * H5[2]
    sw = torch.full_like(l, w0)
    sc = w0 * c
    sv = (w0 * w0) * v if lum else None
    taps = big = 0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dx == 0 and dy == 0:
                continue
            ox, oy = dx * step, dy * step
            ez, wn, inside = edge_weight_terms(z, n, grad, ox, oy, sigma_z, sigma_n)
            cq, _ = shifted(c, ox, oy)
            e = ez + (l - luminance(cq)).abs() / phi if lum else ez
            hh = H5[dx + 2] * H5[dy + 2]
            w = hh * torch.exp(-e) * wn * inside
            sw = sw + w
            sc = sc + w.unsqueeze(1) * cq
            if lum:
                sv = sv + (w * w).unsqueeze(1) * shifted(v, ox, oy)[0]
            taps += inside.sum().item() * c.shape[0]
            big += ((w > 1e-3 * hh) & inside).sum().item()
    return (sc / sw.unsqueeze(1), sv / (sw * sw).unsqueeze(1) if lum else None,
            big / max(taps, 1))


@single_thread
def variance_pass(color, moments, length, var, depth, normals, min_history=4, sigma_z=1.0,
                  sigma_n=128.0, dtype=torch.float64):
    """(color', var')"""
    c, m, z, n = color.to(dtype), moments.to(dtype), depth.to(dtype), normals.to(dtype)
    N, v = length.to(dtype), var.to(dtype)
    grad = gradient(z[:, 0])
    sw = torch.ones_like(z[:, 0])
    sc, sm = c.clone(), m.clone()
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            if dx == 0 and dy == 0:
                continue
            ez, wn, inside = edge_weight_terms(z, n, grad, dx, dy, sigma_z, sigma_n)
            w = torch.exp(-ez) * wn * inside
            sw = sw + w
            sc = sc + w.unsqueeze(1) * shifted(c, dx, dy)[0]
            sm = sm + w.unsqueeze(1) * shifted(m, dx, dy)[0]
    M = sm / sw.unsqueeze(1)
    est = (M[:, 1:2] - M[:, 0:1] * M[:, 0:1]).clamp(min=0) * (c32(min_history, dtype) / N)
    short = N < min_history
    return torch.where(short, sc / sw.unsqueeze(1), c), torch.where(short, est, v)


@single_thread
def accumulate(cur, depth, normals, prev_depth, prev_normals, mv, hist, alpha=0.2,
               moments_alpha=0.2, max_history=32, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS,
               scale=(1.0, 1.0), dtype=torch.float64):
    """dict(color, moments, length, var, accepted [B,1,H,W] bool, margins). hist:
    None (a first frame) or (colour, moments, length); mv None: no motion and
    nothing rejected."""
    c = cur.to(dtype)
    B, C, H, W = c.shape
    l = luminance(c).unsqueeze(1)
    margins = {}
    if hist is None:
        ok = torch.zeros(B, H, W, dtype=torch.bool)
        cc, m1, m2, N = c, l, l * l, torch.ones(B, 1, H, W, dtype=dtype)
    else:
        hc, hm, hn = (t.to(dtype) for t in hist)
        m = mv if mv is not None else torch.zeros(B, 2, H, W)
        ok, taps, border = lookup(m, scale, dtype)
        inside = ok.clone()
        margins["border"] = border[torch.isfinite(border)].abs().min().item()
        if mv is not None:
            z = depth.to(dtype)[:, 0]
            d = depth_tol * z.abs() - (z - sample(prev_depth.to(dtype), taps)[:, 0]).abs()
            ok = ok & (d >= 0)
            d2 = (normals.to(dtype) * sample(prev_normals.to(dtype), taps)).sum(1) - normal_cos
            ok = ok & (d2 >= 0)
            if inside.any():
                margins["depth"] = d[inside].abs().min().item()
                margins["normal"] = d2[inside].abs().min().item()
        px = torch.arange(W, dtype=dtype).view(1, 1, W) + m[:, 0].to(dtype) * scale[0]
        py = torch.arange(H, dtype=dtype).view(1, H, 1) + m[:, 1].to(dtype) * scale[1]
        px, py = torch.where(inside, px, torch.zeros_like(px)), torch.where(inside, py, torch.zeros_like(py))
        if inside.any():
            margins["nearest"] = min(((p - p.floor()) - 0.5).abs()[inside].min().item()
                                     for p in (px, py))
        ix = (px + 0.5).floor().clamp(0, W - 1).long()
        iy = (py + 0.5).floor().clamp(0, H - 1).long()
        b = torch.arange(B).view(B, 1, 1)
        okc = ok.unsqueeze(1)
        N = torch.where(okc, (hn[b, 0, iy, ix].unsqueeze(1) + 1).clamp(max=max_history),
                        torch.ones(B, 1, H, W, dtype=dtype))
        a = torch.maximum(c32(alpha, dtype), 1 / N)
        am = torch.maximum(c32(moments_alpha, dtype), 1 / N)
        hm_s = sample(hm, taps)
        cc = torch.where(okc, c + (1 - a) * (sample(hc, taps) - c), c)
        m1 = torch.where(okc, l + (1 - am) * (hm_s[:, 0:1] - l), l)
        m2 = torch.where(okc, l * l + (1 - am) * (hm_s[:, 1:2] - l * l), l * l)
    return dict(color=cc, moments=torch.cat([m1, m2], 1), length=N,
                var=(m2 - m1 * m1).clamp(min=0), accepted=ok.unsqueeze(1), margins=margins)


@single_thread
def sequence(frames, mvs, depth, normals, iterations=5, alpha=0.2, moments_alpha=0.2,
             max_history=32, min_history=4, feedback=1, sigma_z=1.0, sigma_n=128.0, sigma_l=4.0,
             depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS, scale=(1.0, 1.0), dtype=torch.float64):
    """The whole recurrence: dict of lists over the frames (out, var, accepted,
    length, margins)."""
    res = dict(out=[], var=[], accepted=[], length=[], margins=[])
    fb = min(feedback, iterations)
    hist = None
    for t in range(len(frames)):
        a = accumulate(frames[t], depth[t], normals[t], depth[t - 1] if t else None,
                       normals[t - 1] if t else None, mvs[t - 1] if mvs is not None and t else None,
                       hist, alpha, moments_alpha, max_history, depth_tol, normal_cos, scale, dtype)
        c, v = variance_pass(a["color"], a["moments"], a["length"], a["var"], depth[t], normals[t],
                             min_history, sigma_z, sigma_n, dtype)
        keep = a["color"]
        if iterations == 0:
            c = a["color"]
        for k in range(1, iterations + 1):
            c, v2, _ = atrous(c, v, depth[t], normals[t], 1 << (k - 1), sigma_z, sigma_n, sigma_l,
                              dtype)
            v = v2 if v2 is not None else v
            if k == fb:
                keep = c
        hist = (keep, a["moments"], a["length"])
        res["out"].append(c)
        res["var"].append(v)
        res["accepted"].append(a["accepted"])
        res["length"].append(a["length"])
        res["margins"].append(a["margins"])
    return res


# ---- floors and the bound -----------------------------------------------------
def floor_color(sigma_n):
    """A spatial pass's colour (module docstring)."""
    return U24 * (3 * sigma_n + 35)


FLOOR_ACC = 2.0 ** -21


def floor_var_fallback(sigma_n, min_history):
    return 3 * min_history * floor_color(sigma_n)


def floor_var_atrous(sigma_n, vmax):
    return 2 * floor_color(sigma_n) * vmax


def floor_sequence(t, vmax, iterations=5, alpha=0.2, min_history=4, sigma_n=128.0, **_):
    """(colour, variance) floors of frame t of the recurrence."""
    geo = sum((1 - alpha) ** k for k in range(t + 1))
    fc = FLOOR_ACC + (iterations + 1) * floor_color(sigma_n)
    fv = FLOOR_ACC + floor_var_fallback(sigma_n, min_history) \
        + iterations * floor_var_atrous(sigma_n, vmax)
    return fc * geo, fv * geo


def bound(got64, got32, floor):
    """max(2 x the float32 restatement's worst error, the floor), and that error."""
    e32 = (got32.double() - got64).abs().max().item()
    return max(2 * e32, floor), e32


_REF = {}


def reference(shape, family, motion=True, params="default"):
    """A case computed once, shared, read-only: (inputs, float64 sequence,
    float32 sequence)."""
    key = (shape, family, motion, params)
    if key not in _REF:
        data = inputs(shape, family)
        frames, mvs, depth, normals, _ = data
        kw = CAP if params == "cap" else PARAMS
        m = mvs if motion else None
        _REF[key] = (data, sequence(frames, m, depth, normals, **kw),
                     sequence(frames, m, depth, normals, dtype=torch.float32, **kw))
    return _REF[key]
