"""A numpy restatement of the training-patch sampler (csrc/nsm_patch.hip), with
no import from nsm_amd: the draws in Python integers and the gather in float32
arithmetic, one rounding per operation, in the kernel's order.

Sample i of step t is n = t * B + i (mod 2^64); field f of it is
r_f = mix64((seed ^ mix64(rank)) ^ mix64(8 n + f)) and draw(m) = (r_f * m) >> 64.
"""
import numpy as np

M64 = (1 << 64) - 1
EPS = 1e-8          # MmapLiverDataset.EPS (setdata.py:316)


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def field(seed, rank, n, f):
    return mix64(((seed & M64) ^ mix64(rank)) ^ mix64((8 * n + f) & M64))


def shard(N, world, rank):
    lo, hi = rank * N // world, (rank + 1) * N // world
    return lo, hi - lo


def draws(seed, rank, step, B, *, frame, patch, lo, count, order="sequential", align=1,
          hflip=False, vflip=False, emitters=1):
    """int32 [B, 8]: frame, oy, ox, hflip, vflip, emitter, 0, 0 of each sample."""
    (H, W), (ph, pw) = frame, patch
    out = np.zeros((B, 8), dtype=np.int32)
    for i in range(B):
        n = (step * B + i) & M64
        if order == "sequential":
            out[i, 0] = lo + n % count
        else:
            out[i, 0] = lo + ((field(seed, rank, n, 0) * count) >> 64)
        out[i, 1] = align * ((field(seed, rank, n, 1) * ((H - ph) // align + 1)) >> 64)
        out[i, 2] = align * ((field(seed, rank, n, 2) * ((W - pw) // align + 1)) >> 64)
        r = field(seed, rank, n, 3)
        out[i, 3] = (r >> 63) if hflip else 0
        out[i, 4] = ((r >> 62) & 1) if vflip else 0
        out[i, 5] = (field(seed, rank, n, 4) * emitters) >> 64
    return out


def gather(inputs, labels, d, patch, *, means=None, stds=None, eps=EPS, hsign=None, vsign=None,
           emitter_channel=None, emitter_values=None):
    """(x [B,C,ph,pw], y [B,1,ph,pw]) float32 of the draws d [B,8]:
    x = ((s * v + o) - mean[c]) / (std[c] + eps); o only on the emitter channel.
    No stats: mean 0, std 1, eps 0."""
    inputs, labels = np.asarray(inputs, np.float32), np.asarray(labels, np.float32)
    C = inputs.shape[1]
    ph, pw = patch
    f32 = np.float32
    if means is None:
        means, stds, eps = np.zeros(C, f32), np.ones(C, f32), 0.0
    means, stds = np.asarray(means, f32), np.asarray(stds, f32)
    div = (stds + f32(eps)).astype(f32).reshape(C, 1, 1)
    one = np.ones(C, f32)
    hsign = one if hsign is None else np.asarray(hsign, f32)
    vsign = one if vsign is None else np.asarray(vsign, f32)
    xs, ys = [], []
    for fr, oy, ox, hf, vf, e, _, _ in np.asarray(d).tolist():
        v = inputs[fr, :, oy:oy + ph, ox:ox + pw]
        y = labels[fr, e:e + 1, oy:oy + ph, ox:ox + pw]
        if hf:
            v, y = v[:, :, ::-1], y[:, :, ::-1]
        if vf:
            v, y = v[:, ::-1], y[:, ::-1]
        s = ((hsign if hf else one) * (vsign if vf else one)).astype(f32).reshape(C, 1, 1)
        a = (s * v).astype(f32)
        if emitter_channel is not None:
            a[emitter_channel] = a[emitter_channel] + f32(emitter_values[e])
        xs.append(((a - means.reshape(C, 1, 1)).astype(f32) / div).astype(f32))
        ys.append(np.ascontiguousarray(y))
    return np.stack(xs), np.stack(ys)


def chi2(counts):
    counts = np.asarray(counts, dtype=np.float64)
    exp = counts.sum() / counts.size
    return float(((counts - exp) ** 2 / exp).sum())
