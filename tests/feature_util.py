"""The oracle of the feature-recipe tests (test_feature_ref.py,
test_gpu_features.py): `compose_ref`, a numpy fp32 restatement of what
nsm_feature_compose does per output sample, every step a separate np.float32
operation in the order of csrc/nsm_features.hip:

    1. the term over the raw values at the reflected source pixel
       (raw / sub / ratio with its floor / dot3, left to right)
    2. the census: NaN, +Inf, -Inf among an image's own H x W composed values
    3. the scrub: NaN -> 0, +Inf -> 1, -Inf -> 0, selects only
    4. v + emitter[b] on the emitter channel only
    5. (v - mean[c]) / (std[c] + eps)

and the seeded inputs with the special values planted where frame_util's
prep_spots puts them. numpy's float32 ufuncs round once per operation and never
contract, so on finite and infinite values the result is the kernel's bit for
bit. What IEEE 754 leaves open is the sign and payload of a NaN that an
operation produces or passes on: x86 and gfx950 differ there, so `same_bits`
compares NaNs by position, and bit for bit only in the channels named `exact`
(raw terms nothing was added to, where the kernel moves the bits).
"""
import numpy as np
import torch

import frame_util as F

FLT_MAX = np.float32(np.finfo(np.float32).max)
PAYLOAD_NAN = np.array([0xffc12345], dtype=np.uint32).view(np.float32)[0]   # quiet, negative
EPS = 1e-8
LAYOUT = {"d": 0, "n": 1, "z": 4, "ne": 5, "zf": 8, "ce": 9, "cc": 10}
EXPRS = ["z", "z-zf", "z/zf", "cc/d", "n.ne", "ce"]
CIN = 11


def recipe6():
    from nsm_amd.features import FeatureRecipe
    return FeatureRecipe.parse(EXPRS, layout=LAYOUT)


def reflect(n, p):
    return [i if i < n else 2 * (n - 1) - i for i in range(p)]


def compose_ref(x, recipe, Hp=None, Wp=None, scrub=False, stats=None, eps=EPS,
                emitter_channel=None, emitter=None):
    """x [B,Cin,H,W] float32 numpy -> (out [B,Cout,Hp,Wp] float32, census [B,3] int32)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4 and x.shape[1] == recipe.in_channels
    B, _, H, W = x.shape
    Hp, Wp = Hp or H, Wp or W
    assert H <= Hp < 2 * H and W <= Wp < 2 * W
    src = x[:, :, reflect(H, Hp), :][:, :, :, reflect(W, Wp)]
    floor = np.float32(recipe.ratio_floor)
    out = np.empty((B, recipe.out_channels, Hp, Wp), dtype=np.float32)
    with np.errstate(all="ignore"):
        for c, (op, a, b) in enumerate(recipe.table().tolist()):
            if op == 0:
                v = src[:, a].copy()
            elif op == 1:
                v = src[:, a] - src[:, b]
            elif op == 2:
                q = src[:, a] / src[:, b]
                v = np.where(np.abs(src[:, b]) <= floor, np.float32(0.0), q)
            else:
                p0 = src[:, a] * src[:, b]
                p1 = src[:, a + 1] * src[:, b + 1]
                p2 = src[:, a + 2] * src[:, b + 2]
                v = (p0 + p1) + p2
            assert v.dtype == np.float32
            out[:, c] = v
        own = out[:, :, :H, :W].reshape(B, -1)
        census = np.stack([np.isnan(own).sum(1), (own == np.inf).sum(1), (own == -np.inf).sum(1)],
                          axis=1).astype(np.int32)
        if scrub:
            out = np.where(np.isnan(out), np.float32(0.0),
                           np.where(out == np.inf, np.float32(1.0),
                                    np.where(out == -np.inf, np.float32(0.0), out)))
        if emitter_channel is not None:
            e = np.broadcast_to(np.asarray(emitter, dtype=np.float32).reshape(-1), (B,))
            out[:, emitter_channel] = out[:, emitter_channel] + e.reshape(B, 1, 1)
        if stats is not None:
            mean, std = (np.asarray(v, dtype=np.float32).reshape(1, -1, 1, 1) for v in stats)
            out = (out - mean) / (std + np.float32(eps))
    assert out.dtype == np.float32
    return out, census


def _around(v):
    """v's fp32 neighbour below, v, and the neighbour above."""
    v = np.float32(v)
    return [np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(np.inf))]


def scenarios(floor=1e-6):
    """What is planted at a pixel: {raw channel: value} over LAYOUT. None of them
    makes a subnormal intermediate (no finite value is divided by FLT_MAX)."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    d, n, z, ne, zf, ce, cc = (LAYOUT[k] for k in ("d", "n", "z", "ne", "zf", "ce", "cc"))
    sc = [
        {z: nan}, {zf: nan}, {z: nan, zf: nan},                  # NaN through raw, sub and ratio
        {z: inf, zf: inf}, {z: -inf, zf: 1.0}, {zf: inf}, {zf: -inf}, {z: inf, zf: -inf},
        {z: FLT_MAX, zf: -FLT_MAX}, {z: -FLT_MAX, zf: FLT_MAX},  # sub overflows, the ratio is -1
        {cc: FLT_MAX, d: 0.5}, {cc: -FLT_MAX, d: 0.5},           # the ratio overflows
        {d: 0.0}, {d: -0.0}, {d: nan}, {d: inf, cc: inf},
        {z: -0.0, zf: -0.0}, {ce: -0.0}, {ce: nan}, {ce: inf}, {ce: -inf}, {ce: FLT_MAX},
        {n: inf, n + 1: 0.0, n + 2: 1.0, ne: 0.0, ne + 1: 1.0, ne + 2: 1.0},        # Inf * 0
        {n: FLT_MAX, n + 1: FLT_MAX, n + 2: 0.0, ne: 2.0, ne + 1: 2.0, ne + 2: 0.0},   # Inf + Inf
        {n: FLT_MAX, n + 1: FLT_MAX, n + 2: 1.0, ne: 2.0, ne + 1: -2.0, ne + 2: 1.0},  # Inf - Inf
        {n + 1: nan}, {ne + 2: -inf},
        {ce: PAYLOAD_NAN, z: PAYLOAD_NAN},                       # a raw term keeps sign and payload
    ]
    for v in _around(floor):                                      # denominators around the floor
        sc += [{d: v, cc: 1.0}, {d: -v, cc: 1.0}, {zf: v, z: -1.0}]
    return sc


def spots_for(H, W, pad_multiple, count):
    """frame_util's prep_spots inside H x W, topped up with interior pixels to `count`."""
    spots = [s for s in F.prep_spots(H, W, pad_multiple) if 0 <= s[0] < H and 0 <= s[1] < W]
    spots = list(dict.fromkeys(spots))
    k = 0
    while len(spots) < count and k < H * W:
        s = ((5 + 3 * k) % H, (7 + 5 * k) % W)
        if s not in spots:
            spots.append(s)
        k += 1
    return spots


def feature_input(shape, seed=0, pad_multiple=None, floor=1e-6):
    """Seeded unit normals [B,CIN,H,W] (float32 numpy) with the scenarios planted:
    scenario (i + 11 b) mod S at spot i of image b, so the reflected rows and
    columns and the corners meet different ones in each image."""
    B, C, H, W = shape
    assert C == CIN
    g = torch.Generator().manual_seed(6007 * seed + sum(shape))
    x = torch.randn(*shape, generator=g).numpy().copy()
    sc = scenarios(floor)
    spots = spots_for(H, W, pad_multiple, len(sc))
    for b in range(B):
        for i, (yy, xx) in enumerate(spots):
            for ch, v in sc[(i + 11 * b) % len(sc)].items():
                x[b, ch, yy, xx] = v
    return x


def mild_input(shape, seed=0, floor=1e-6):
    """Seeded unit normals with a few specials per image that compose to NaN, +Inf,
    -Inf, +-0 and guarded ratios but to nothing huge: frames a network, a patch
    pool and a statistics pass can take (no FLT_MAX)."""
    B, C, H, W = shape
    assert C == CIN and H >= 4 and W >= 8
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    d, z, zf, ce, cc = (LAYOUT[k] for k in ("d", "z", "zf", "ce", "cc"))
    g = torch.Generator().manual_seed(7001 * seed + sum(shape))
    x = torch.randn(*shape, generator=g).numpy().copy()
    plan = [{z: nan}, {zf: nan}, {z: inf, zf: inf}, {z: -inf}, {zf: inf}, {d: 0.0}, {d: -0.0},
            {d: np.float32(floor), cc: 1.0}, {ce: -0.0}, {ce: -inf}, {z: -0.0, zf: -0.0}, {ce: inf}]
    for b in range(B):
        for i, sc in enumerate(plan[:len(plan) - b]):             # another count in every image
            yy, xx = ((H - 1 - i) % H, W - 1) if i % 3 == 0 else ((2 * i + b) % H, (3 * i + 1) % W)
            for ch, v in sc.items():
                x[b, ch, yy, xx] = v
    return x


def stats_for(C, seed=1):
    """Per-channel figures with a std of 0 (a division by eps) in channel 0."""
    g = torch.Generator().manual_seed(seed)
    means, stds = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    stds[0] = 0.0
    return means.numpy().copy(), stds.numpy().copy()


def bits(t):
    t = torch.as_tensor(t)
    return t.contiguous().view(torch.int32)


def same_bits(got, ref, exact=None, what=""):
    """got == ref bit for bit (fp32; -0.0 is not +0.0), a NaN matching any NaN at
    the same place; in the channels `exact` (None: none, "all": every one) a
    NaN's sign and payload count too. Prints how many NaNs differ in their bits."""
    got, ref = torch.as_tensor(got).cpu(), torch.as_tensor(ref).cpu()
    if got.shape != ref.shape or got.dtype != torch.float32 or ref.dtype != torch.float32:
        return False
    gb, rb = bits(got), bits(ref)
    nan_g, nan_r = torch.isnan(got), torch.isnan(ref)
    loose = int(((gb != rb) & nan_g & nan_r).sum())
    if loose:
        print(f"{what}: {loose} of {int(nan_r.sum())} NaNs differ in sign or payload")
    canon = torch.tensor(0x7fc00000, dtype=torch.int32)
    ok = torch.equal(torch.where(nan_g, canon, gb), torch.where(nan_r, canon, rb))
    if exact == "all":
        ok = ok and torch.equal(gb, rb)
    elif exact:
        ok = ok and torch.equal(gb[:, list(exact)], rb[:, list(exact)])
    return ok


def raw_channels(recipe):
    """The output channels that are raw terms."""
    return [c for c, t in enumerate(recipe.terms) if t[0] == "raw"]
