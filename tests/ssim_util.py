"""`pytorch_msssim.ssim` with its defaults (win_size 11, sigma 1.5, K = (0.01,
0.03), nonnegative_ssim=False) restated from its published algorithm with
F.conv2d and torch autograd: the comparator of test_ssim_ref.py and
test_gpu_ssim.py. Evaluated in float64 on inputs first rounded to float32;
`dtype=torch.float32` is what a user would otherwise run on ATen ops, and its
own error against float64 is the yardstick of the GPU tests."""
import torch
import torch.nn.functional as F

WIN, SIGMA = 11, 1.5
# one window per image; a single row of windows; one 16 x 64 tile of windows
# plus one window each way (B = 3, distinct images); >= 2 tiles both ways and no
# power-of-two multiple
SHAPES = [(2, 1, 11, 11), (1, 1, 12, 13), (2, 1, 11, 75), (3, 1, 27, 75), (2, 1, 40, 90)]
FAMILIES = ("random", "smooth")
RANGES = (1.0, 255.0)


def inputs(shape, family="random", seed=0):
    """float32 (o, t), every image of the batch distinct.
    random: o = sigmoid(2 randn), t = rand (detail_util.inputs);
    smooth: t a sigmoid edge ramp whose phase differs per image,
            o = clamp(t + 0.02 randn, 0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    if family == "random":
        o = torch.sigmoid(2 * torch.randn(shape, generator=gen))
        t = torch.rand(shape, generator=gen)
        return o, t
    B, _, H, W = shape
    y = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1)
    x = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
    phase = torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1)
    t = torch.sigmoid((x + 0.5 * y - 0.45 * (W + 0.5 * H) - 3.0 * phase) / 4.0)
    o = (t + 0.02 * torch.randn(shape, generator=gen)).clamp(0, 1)
    return o, t


def window(dtype):
    """The 1-D Gaussian: exp(-(i-5)^2 / (2 sigma^2)), normalised to sum 1."""
    c = torch.arange(WIN, dtype=dtype) - WIN // 2
    g = torch.exp(-(c ** 2) / (2 * SIGMA ** 2))
    return g / g.sum()


def blur(x, g):
    """g along H, then g along W; a valid correlation (no padding)."""
    x = F.conv2d(x, g.view(1, 1, WIN, 1))
    return F.conv2d(x, g.view(1, 1, 1, WIN))


def ssim_map(o, t, data_range=1.0):
    g = window(o.dtype)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    a, b = blur(o, g), blur(t, g)
    p, q, r = blur(o * o, g), blur(t * t, g), blur(o * t, g)
    sx, sy, sxy = p - a * a, q - b * b, r - a * b
    return (2 * a * b + c1) / (a * a + b * b + c1) * ((2 * sxy + c2) / (sx + sy + c2))


def ssim_per_image(o, t, data_range=1.0):
    return ssim_map(o, t, data_range).flatten(1).mean(1)


def evaluate(o32, t32, data_range=1.0, dtype=torch.float64):
    """(per-image values [B], batch mean (float), d(mean)/do [B,1,H,W]) in `dtype`."""
    o = o32.detach().clone().to(dtype).requires_grad_(True)   # never the shared input itself
    per = ssim_per_image(o, t32.to(dtype), data_range)
    val = per.mean()
    grad, = torch.autograd.grad(val, o)
    return per.detach(), val.item(), grad


def closed_form_grad(o32, t32, data_range=1.0, dtype=torch.float64):
    """d(mean S)/dX_i = (g*A)_i + 2 X_i (g*Bc)_i + Y_i (g*Cc)_i with A = dS/da,
    Bc = dS/dp, Cc = dS/dr per window over the window count, `*` the full
    (transposed) separable correlation."""
    X, Y = o32.to(dtype), t32.to(dtype)
    g = window(dtype)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    a, b = blur(X, g), blur(Y, g)
    p, q, r = blur(X * X, g), blur(Y * Y, g), blur(X * Y, g)
    d1, d2 = a * a + b * b + c1, (p - a * a) + (q - b * b) + c2
    lum, cs = (2 * a * b + c1) / d1, (2 * (r - a * b) + c2) / d2
    n = a.numel()
    A = (cs * 2 * (b - lum * a) / d1 + lum * 2 * (a * cs - b) / d2) / n
    Bc = -lum * cs / d2 / n
    Cc = 2 * lum / d2 / n

    def full(m):
        m = F.conv2d(m, g.flip(0).view(1, 1, WIN, 1), padding=(WIN - 1, 0))
        return F.conv2d(m, g.flip(0).view(1, 1, 1, WIN), padding=(0, WIN - 1))

    return full(A) + 2 * X * full(Bc) + Y * full(Cc)


_REF = {}


def reference(shape, family, data_range=1.0):
    """A case computed once, shared, read-only: (o, t, float64 (per, val, grad),
    float32 restatement (per, val, grad))."""
    key = (shape, family, data_range)
    if key not in _REF:
        o, t = inputs(shape, family)
        _REF[key] = (o, t, evaluate(o, t, data_range), evaluate(o, t, data_range, torch.float32))
    return _REF[key]


def grad_errors(got, ref):
    """(rel-L2, worst per-pixel error / max|ref|); every pixel counts."""
    d = got.double() - ref
    return ((d.norm() / ref.norm().clamp_min(1e-300)).item(),
            (d.abs().max() / ref.abs().max().clamp_min(1e-300)).item())


def f32_errors(shape, family, data_range=1.0):
    """The float32 restatement's own error against float64 for a case:
    (gradient rel-L2, worst pixel / max|g|, |value error|, worst per-image |value error|)."""
    _, _, (per, val, grad), (per32, val32, grad32) = reference(shape, family, data_range)
    rel, worst = grad_errors(grad32, grad)
    return rel, worst, abs(val32 - val), (per32.double() - per).abs().max().item()
