"""The oracle of the inference-frame-path tests (test_frame_ref.py,
test_gpu_frames.py): a CPU restatement, in torch and numpy ops, of what the
reference's inference.py does around model(x), and the seeded inputs.

    prep_ref    nn.ReflectionPad2d((0, pad_w, 0, pad_h)) to a multiple of 16
                (inference.py:153-163), torch.nan_to_num(nan=0.0, posinf=1.0,
                neginf=0.0) (inference.py:170-173), then the loader's
                (x - mean) / (std + 1e-8) (setdata.py:316) when stats are given
    finish_ref  the crop, nan_to_num again (inference.py:199-202), np.clip(., 0, 1)
                and (x * 255).astype(np.uint8) with np.transpose(., (1, 2, 0))
                (save_output, inference.py:108-125)
    *_census    the counts the device census reports
"""
import numpy as np
import torch

FLT_MAX = float(np.finfo(np.float32).max)
DENORMAL = float(np.float32(1e-41))
# NaN, +Inf, -Inf and the finite values a scrub must not touch
SPECIALS = [float("nan"), float("inf"), float("-inf"), -0.0, DENORMAL, FLT_MAX, -FLT_MAX]
EPS = 1e-8

# (B, C, H, W) of test 1: pad 15/13 with W % 4 = 3; pad 15/0; none; W % 4 = 2; pad 1/14
PREP_SHAPES = [(1, 4, 17, 19), (2, 7, 33, 48), (1, 4, 16, 16), (2, 1, 20, 66), (1, 3, 31, 18)]
# (Hp, Wp) -> size of test 4
FINISH_CROPS = [((32, 32), (17, 19)), ((32, 80), (20, 66)), ((16, 16), (16, 16)), ((32, 48), None)]


def padded(n, multiple=16):
    return n if multiple in (None, 1) else -(-n // multiple) * multiple


def scrub(t):
    return torch.nan_to_num(t, nan=0.0, posinf=1.0, neginf=0.0)


def prep_ref(x, pad_multiple=16, scrub_on=True, stats=None, eps=EPS):
    """x [B,C,H,W] fp32 CPU -> [B,C,Hp,Wp] fp32."""
    H, W = x.shape[-2:]
    pad_h, pad_w = padded(H, pad_multiple) - H, padded(W, pad_multiple) - W
    y = torch.nn.ReflectionPad2d((0, pad_w, 0, pad_h))(x) if pad_h or pad_w else x.clone()
    if scrub_on:
        y = scrub(y)
    if stats is not None:
        mean, std = (torch.as_tensor(v, dtype=torch.float32).view(1, -1, 1, 1) for v in stats)
        y = (y - mean) / (std + torch.tensor(eps, dtype=torch.float32))
    return y


def pad_by_index(x, Hp, Wp):
    """The pad as the index formula: out[.., y, x] = in[.., ry, rx]."""
    H, W = x.shape[-2:]
    ry = [y if y < H else 2 * (H - 1) - y for y in range(Hp)]
    rx = [c if c < W else 2 * (W - 1) - c for c in range(Wp)]
    return x[..., ry, :][..., rx]


def prep_census(x):
    """[B,3]: NaN, +Inf, -Inf among each image's own samples."""
    f = x.flatten(1)
    return torch.stack([torch.isnan(f).sum(1), (f == float("inf")).sum(1),
                        (f == float("-inf")).sum(1)], dim=1).to(torch.int32)


def finish_ref(o, size=None):
    """o [B,C,Hp,Wp] fp32 CPU -> (uint8 [B,H,W] or [B,H,W,C], fp32 [B,C,H,W])."""
    H, W = size if size is not None else o.shape[-2:]
    v = np.clip(scrub(o[..., :H, :W]).numpy(), 0, 1)
    assert v.dtype == np.float32
    imgs = []
    for frame in v:                       # save_output takes one [C,H,W] frame
        if frame.shape[0] == 1:
            imgs.append((frame.squeeze(0) * 255).astype(np.uint8))
        else:
            imgs.append((np.transpose(frame, (1, 2, 0)) * 255).astype(np.uint8))
    return torch.from_numpy(np.stack(imgs)), torch.from_numpy(v.copy())


def finish_census(o, size=None):
    """[B,3]: non-finite, < 0 and > 1 samples of each image's cropped region."""
    H, W = size if size is not None else o.shape[-2:]
    f = o[..., :H, :W].flatten(1)
    return torch.stack([(~torch.isfinite(f)).sum(1), (f < 0).sum(1), (f > 1).sum(1)],
                       dim=1).to(torch.int32)


def plant(x, spots):
    """Write SPECIALS, in turn, at the (y, x) `spots` of every plane, each
    plane starting at another special so that every value meets every spot
    kind across planes."""
    B, C = x.shape[:2]
    for b in range(B):
        for c in range(C):
            for i, (yy, xx) in enumerate(spots):
                x[b, c, yy, xx] = SPECIALS[(i + b * C + c) % len(SPECIALS)]
    return x


def prep_spots(H, W, pad_multiple=16):
    """Interior, row H-1, column W-1, and the rows / columns a reflection
    copies (those within the pad's reach of the far edge, the edge excluded)."""
    ph, pw = padded(H, pad_multiple) - H, padded(W, pad_multiple) - W
    spots = [(H // 2, W // 2), (H // 3, 1), (1, W // 3), (H // 2, W // 2 + 1), (2, 2), (3, 5),
             (H // 2 + 1, 3),
             (H - 1, 0), (H - 1, W // 2), (H - 1, W - 1), (0, W - 1), (H // 2, W - 1)]
    for k in range(1, ph + 1):            # row H-1-k is copied to row H-1+k
        spots.append((H - 1 - k, (3 * k) % W))
    for k in range(1, pw + 1):
        spots.append(((5 * k) % H, W - 1 - k))
    if ph and pw:
        spots.append((H - 2, W - 2))      # copied three times: right, below, corner
    return list(dict.fromkeys(spots))


def prep_input(shape, seed=0, pad_multiple=16, clean_image=None):
    """Seeded normals with the specials planted; clean_image: an image index left
    without any (the census's 'none' case)."""
    g = torch.Generator().manual_seed(7919 * seed + sum(shape))
    x = torch.randn(*shape, generator=g)
    keep = x[clean_image].clone() if clean_image is not None else None
    plant(x, prep_spots(shape[2], shape[3], pad_multiple))
    if clean_image is not None:
        x[clean_image] = keep
    return x


def finish_values():
    """Every k/255 with both fp32 neighbours, the edges of the clip, and the
    non-finite values."""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    vals = np.concatenate([
        k, np.nextafter(k, np.float32(-np.inf)), np.nextafter(k, np.float32(np.inf)),
        np.array([0.0, -0.0, 1.0, 1 - 2.0 ** -24, 1 + 2.0 ** -23, -1e-30, 2.0,
                  np.nan, np.inf, -np.inf], dtype=np.float32)]).astype(np.float32)
    return torch.from_numpy(vals)


def finish_input(C, Hp, Wp, size=None, seed=0):
    """[B,C,Hp,Wp] uniform on [-0.1, 1.1] with every one of finish_values() at a
    seeded place of the cropped region of some image; B is the smallest batch
    (at least 2) whose cropped regions hold them all."""
    H, W = size if size is not None else (Hp, Wp)
    vals = finish_values()
    B = max(2, -(-vals.numel() // (C * H * W)))
    g = torch.Generator().manual_seed(104729 * seed + 31 * C + Hp + Wp)
    o = torch.rand(B, C, Hp, Wp, generator=g) * 1.2 - 0.1
    crop = o[..., :H, :W].clone()
    where = torch.randperm(crop.numel(), generator=g)[:vals.numel()]
    crop.view(-1)[where] = vals
    o[..., :H, :W] = crop
    return o
