"""The detail terms of CustomLoss (customLoss.py:139-185) restated with
F.conv2d and torch autograd: the comparator of test_detail_ref.py and
test_gpu_detail.py. Evaluated in float64 on inputs first rounded to float32,
with the penumbra mask built in float32 (as the reference builds it on fp32
tensors); `dtype=torch.float32` gives the reference's own arithmetic."""
import torch
import torch.nn.functional as F

# smaller than the halo; >= 2 tiles both ways and no multiple of a power-of-two
# tile; one 16 x 64 tile plus one pixel
SHAPES = [(2, 1, 2, 2), (2, 1, 4, 6), (3, 1, 33, 65), (2, 1, 40, 72), (2, 1, 17, 65)]
TERMS = ("hf", "pen", "sob")

VALUE_REL = 1e-5        # ~40 fp32 roundings per pixel at 2^-24 each = 2.4e-6, times 4
GRAD_REL_L2 = 1e-5
GRAD_PIXEL = 1e-4       # times max|g|
TIE_SHARE = 0.01        # excluded near-tie pixels per case
TIE = {"hf": 1e-5, "sob": 1e-5, "pen": 1e-7}


def inputs(shape, seed=0):
    """o = sigmoid(2 randn), t = rand: float32, every image of the batch distinct."""
    gen = torch.Generator().manual_seed(seed)
    o = torch.sigmoid(2 * torch.randn(shape, generator=gen))
    t = torch.rand(shape, generator=gen)
    return o, t


def gaussian(dtype):
    """customLoss.py:106-114."""
    x = (torch.arange(5) - 2).expand(5, -1)
    y = x.transpose(0, 1)
    k = torch.exp(-(x.pow(2) + y.pow(2)).to(dtype) / 2.0)
    return (k / k.sum()).view(1, 1, 5, 5)


def sobel_kernels(dtype):
    """customLoss.py:168-169."""
    kx = torch.tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=dtype).view(1, 1, 3, 3)
    ky = torch.tensor([[-1, -2, -1], [0, 0, 0], [1, 2, 1]], dtype=dtype).view(1, 1, 3, 3)
    return kx, ky


def penumbra_mask(t):
    t32 = t.to(torch.float32)
    return (t32 > torch.tensor(0.1, dtype=torch.float32)) & (t32 < torch.tensor(0.9, dtype=torch.float32))


def high_freq(x):
    return x - F.conv2d(x, gaussian(x.dtype), padding=2)


def sobel_mag(x):
    kx, ky = sobel_kernels(x.dtype)
    gx, gy = F.conv2d(x, kx, padding=1), F.conv2d(x, ky, padding=1)
    return torch.sqrt(gx ** 2 + gy ** 2 + 1e-6)


def terms(o, t):
    """{'hf', 'pen', 'sob'} in o's dtype, differentiable wrt o."""
    m = penumbra_mask(t).to(o.dtype)
    return {
        "hf": (high_freq(o) - high_freq(t)).abs().mean(),
        "pen": (m * (o - t).abs()).sum() / (m.sum() + 1e-8),
        "sob": (sobel_mag(o) - sobel_mag(t)).abs().mean(),
    }


def evaluate(o32, t32, dtype=torch.float64):
    """Values and per-term gradients: ({term: float}, {term: [B,1,H,W] tensor})."""
    o = o32.detach().clone().to(dtype).requires_grad_(True)   # never the shared input itself
    tt = terms(o, t32.to(dtype))
    grads = {k: torch.autograd.grad(v, o, retain_graph=True)[0] for k, v in tt.items()}
    return {k: v.item() for k, v in tt.items()}, grads


def near_ties(o32, t32):
    """Pixels whose gradient hangs on a decision that is a near tie in float64:
    {term: bool [B,1,H,W]}."""
    o, t = o32.double(), t32.double()
    r = (high_freq(o) - high_freq(t)).abs()
    dm = (sobel_mag(o) - sobel_mag(t)).abs()
    return {
        "hf": F.max_pool2d((r < TIE["hf"]).double(), 5, 1, 2) > 0,
        "sob": F.max_pool2d((dm < TIE["sob"]).double(), 3, 1, 1) > 0,
        "pen": (o - t).abs() < TIE["pen"],
    }


_REF = {}


def reference(shape):
    """The float64 reference of a SHAPES case (computed once, shared, read-only)."""
    if shape not in _REF:
        o, t = inputs(shape)
        vals, grads = evaluate(o, t)
        _REF[shape] = (o, t, vals, grads, near_ties(o, t))
    return _REF[shape]


def grad_errors(got, ref, excluded):
    """(rel-L2, worst per-pixel error / max|ref|, excluded share) outside `excluded`."""
    keep = ~excluded
    d = (got.double() - ref)[keep]
    r = ref[keep]
    rel = (d.norm() / r.norm().clamp_min(1e-300)).item()
    worst = (d.abs().max() / ref.abs().max().clamp_min(1e-300)).item() if d.numel() else 0.0
    return rel, worst, excluded.double().mean().item()
