"""The training-patch sampler: random crops, mirrored G-buffers and the drawn
emitter size (paper §3.1.1), gathered on the device from a pool that was
uploaded once.

The paper trains on up to 400 frames of 2k x 1k per scene and the training step
runs on 512 x 512 crops; `FrameLoader` serves whole frames through the host. A
`PatchSampler` holds the split in device memory (400 x (7 + 1) x 2048 x 1024
fp32 are 26.8 GB) and one launch per step (csrc/nsm_patch.hip,
nsm_patch_gather) writes the batch straight into the step's static buffers:

    sampler = PatchSampler.from_dir(data_dir, patch=(512, 512), batch=8, order="random",
                                    hflip=True, hflip_sign=[1, -1, 1, 1, 1, 1, 1])
    step = GraphedTrainStep(model, loss_fn, opt, *sampler.next())
    for _ in range(steps):
        sampler.next(out=(step.x, step.y))
        step()

What is drawn is a pure function of (seed, rank, step, sample): `patch_draws`
restates it in Python integers, the kernel records it (`record_draws=True`,
`last_draws`), and a resumed sampler (`state_dict`) continues the same stream.
For sample i of step t let n = t * batch + i (mod 2^64); field f of it is

    r_f = mix64((seed ^ mix64(rank)) ^ mix64(8 n + f)),   draw(m) = (r_f * m) >> 64

    f = 0  frame   sequential: lo + n mod count; random: lo + draw(count)
    f = 1  oy      align * draw((H - ph) // align + 1)
    f = 2  ox      align * draw((W - pw) // align + 1)
    f = 3  flips   hflip = top bit, vflip = next bit (a disabled flip is 0)
    f = 4  e       draw(E), the label plane (emitter size) of the pair

with [lo, lo + count) = shard_range(N, world, rank), this rank's frames.

A mirrored G-buffer is not a mirrored tensor: a channel that holds the x
(y) component of a normal changes sign under a horizontal (vertical) flip.
`hflip_sign` / `vflip_sign` are per-channel factors applied to flipped samples.
`emitter_channel` / `emitter_values`: labels [N,E,H,W] hold one target per
emitter size; the drawn index e selects the plane and `emitter_values[e]` is
added to the raw value of that input channel (the dc offset of §3.1.1) before
the normalisation:

    x = ((s * v + o) - mean[c]) / (std[c] + eps)
"""
import os

import numpy as np
import torch

from ._lib import call, ptr, stream
from .data import FrameLoader, MmapLiverDataset, _given_stats, load_stats, shard_range

ORDERS = ("sequential", "random")
UPLOAD_BYTES = 256 << 20    # from_dir: input bytes per batch of the one-time upload
_M64 = (1 << 64) - 1


def mix64(z):
    """nsm::mix64 (csrc/nsm_common.h) on Python integers."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def patch_draws(seed, rank, step, batch, *, frame, patch, lo, count, order="sequential", align=1,
                hflip=False, vflip=False, emitters=1):
    """What nsm_patch_gather draws for the `batch` samples of `step`: an int32
    [batch, 8] tensor of (frame, oy, ox, hflip, vflip, emitter, 0, 0). frame =
    (H, W), patch = (ph, pw); [lo, lo + count) the shard. Host integers only."""
    (H, W), (ph, pw) = frame, patch
    key = (seed & _M64) ^ mix64(rank)
    ny, nx = (H - ph) // align + 1, (W - pw) // align + 1
    rows = []
    for i in range(batch):
        n = (step * batch + i) & _M64
        r = [mix64(key ^ mix64((8 * n + f) & _M64)) for f in range(5)]
        fr = lo + (n % count if order == "sequential" else (r[0] * count) >> 64)
        rows.append([fr, align * ((r[1] * ny) >> 64), align * ((r[2] * nx) >> 64),
                     (r[3] >> 63) if hflip else 0, ((r[3] >> 62) & 1) if vflip else 0,
                     (r[4] * emitters) >> 64, 0, 0])
    return torch.tensor(rows, dtype=torch.int32)


def _as_i64(u):
    """A uint64 as the int64 word holding its bits."""
    return u - (1 << 64) if u >= (1 << 63) else u


def _int_arg(v, name, lo):
    if isinstance(v, bool) or not isinstance(v, int) or v < lo:
        raise ValueError(f"patch sampler: {name} must be an integer >= {lo}, got {v!r}")
    return v


class PatchSampler:
    """Batches of training patches out of a device-resident pool.

    inputs [N,C,H,W] and labels [N,E,H,W] (E = 1: the reference's format) are
    fp32 tensors, normally on the GPU (`from_dir` uploads a split once); with
    CPU tensors everything but `next` works (`draws`, the state).
    stats: a StatsResult or a (means, stds) pair as FrameLoader takes them;
    None: no normalisation, the raw values bit for bit. order: "sequential" is
    the reference's in-order walk over the rank's shard, "random" draws frames
    uniformly with replacement. capturable=True keeps seed and step in device
    words, so `next(out=...)` may be captured into a graph and every replay
    draws the next batch; otherwise they are kernel arguments and the step is
    counted on the host."""

    def __init__(self, inputs, labels, patch=(512, 512), batch=8, stats=None, seed=0,
                 order="sequential", align=1, hflip=False, vflip=False, hflip_sign=None,
                 vflip_sign=None, emitter_channel=None, emitter_values=None, world=1, rank=0,
                 capturable=False, record_draws=False):
        for t, name, shape in ((inputs, "inputs", "[N,C,H,W]"), (labels, "labels", "[N,E,H,W]")):
            if not torch.is_tensor(t) or t.dim() != 4 or min(t.shape) < 1:
                got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
                raise ValueError(f"patch sampler: {name} must be a non-empty {shape} tensor, got {got}")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"patch sampler: {name} must be contiguous float32, got {t.dtype}")
        N, C, H, W = inputs.shape
        if labels.shape[0] != N or tuple(labels.shape[2:]) != (H, W) or labels.device != inputs.device:
            raise ValueError(f"patch sampler: labels {tuple(labels.shape)} on {labels.device} do not "
                             f"match inputs {tuple(inputs.shape)} on {inputs.device}")
        E = labels.shape[1]
        try:
            ph, pw = (int(v) for v in patch)
        except (TypeError, ValueError):
            raise ValueError(f"patch sampler: patch must be (height, width), got {patch!r}") from None
        if ph < 1 or pw < 1 or ph > H or pw > W:
            raise ValueError(f"patch sampler: patch {ph} x {pw} does not fit the {H} x {W} frame")
        _int_arg(batch, "batch", 1)
        _int_arg(align, "align", 1)
        _int_arg(world, "world", 1)
        _int_arg(rank, "rank", 0)
        if rank >= world:
            raise ValueError(f"patch sampler: rank {rank} of world {world}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed <= _M64:
            raise ValueError(f"patch sampler: seed must be an integer in [0, 2^64), got {seed!r}")
        if order not in ORDERS:
            raise ValueError(f"patch sampler: order must be one of {ORDERS}, got {order!r}")
        lo, hi = shard_range(N, world, rank)
        if hi <= lo:
            raise ValueError(f"patch sampler: rank {rank} of {world} owns no frame of {N}")
        if C * H * W >= 1 << 31 or E * H * W >= 1 << 31 or C > 256:
            raise ValueError(f"patch sampler: unsupported frame size {C} x {H} x {W} with {E} label "
                             "planes (a frame holds fewer than 2^31 samples, at most 256 channels)")
        dev = inputs.device
        if stats is None:
            means, stds, self.eps = torch.zeros(C), torch.ones(C), 0.0
        else:
            means, stds = _given_stats(stats, C)
            self.eps = MmapLiverDataset.EPS
        signs = []
        for v, name in ((hflip_sign, "hflip_sign"), (vflip_sign, "vflip_sign")):
            if v is None:
                signs.append(None)
                continue
            v = torch.as_tensor(v).detach().to(torch.float32).reshape(-1)
            if v.numel() != C:
                raise ValueError(f"patch sampler: {name} has {v.numel()} entries, the frames have "
                                 f"{C} channels")
            signs.append(v.to(dev).contiguous())
        if (emitter_channel is None) != (emitter_values is None):
            raise ValueError("patch sampler: emitter_channel and emitter_values go together, got "
                             f"{emitter_channel!r} and {emitter_values!r}")
        if emitter_channel is None:
            self.emitter_channel, self.emitter_values = -1, None
        else:
            if isinstance(emitter_channel, bool) or not isinstance(emitter_channel, int) \
                    or not 0 <= emitter_channel < C:
                raise ValueError(f"patch sampler: emitter_channel must be in [0, {C}), got "
                                 f"{emitter_channel!r}")
            ev = torch.as_tensor(emitter_values).detach().to(torch.float32).reshape(-1)
            if ev.numel() != E:
                raise ValueError(f"patch sampler: emitter_values has {ev.numel()} entries, the labels "
                                 f"hold {E} planes per frame")
            self.emitter_channel, self.emitter_values = emitter_channel, ev.to(dev).contiguous()
        self.inputs, self.labels = inputs, labels
        self.N, self.C, self.E, self.H, self.W = N, C, E, H, W
        self.patch, self.batch, self.align = (ph, pw), batch, align
        self.hflip, self.vflip = bool(hflip), bool(vflip)
        self.hflip_sign, self.vflip_sign = signs
        self.means, self.stds = means.to(dev).contiguous(), stds.to(dev).contiguous()
        self.seed, self.order, self.world, self.rank = seed, order, world, rank
        self.lo, self.count = lo, hi - lo
        self.capturable, self.record_draws = bool(capturable), bool(record_draws)
        self.last_draws = None
        self._step = 0
        self._words = None      # capturable: int64 [2] on the device, (seed, step)
        if self.capturable:
            self._words = torch.tensor([_as_i64(seed), 0], dtype=torch.int64).to(dev)

    @classmethod
    def from_dir(cls, data_dir, split="train", device="cuda", stats_dir=None, recipe=None, **kw):
        """Upload {split}_inputs.npy / {split}_labels.npy once (through the native
        loader, which converts f64 labels on the way) and sample from them.
        Stats as FrameLoader takes them: `stats=`, else train_stats.json under
        stats_dir or data_dir; neither: no normalisation. recipe (a
        features.FeatureRecipe): each uploaded chunk is composed on the device
        (frames.compose_features, no scrub) and the pool holds the recipe's
        channels; stats, hflip_sign, vflip_sign and emitter_channel then index
        the composed channels."""
        dev = torch.device(device)
        shape = np.load(os.path.join(data_dir, f"{split}_inputs.npy"), mmap_mode="r").shape
        N, Craw, H, W = (int(v) for v in shape)
        C = Craw
        if recipe is not None:
            from .frames import compose_features
            recipe.check_input(Craw, "patch sampler")
            C = recipe.out_channels
        chunk = max(1, min(N, UPLOAD_BYTES // (4 * Craw * H * W)))
        loader = FrameLoader(data_dir, split, batch=chunk, device=dev, apply_normalization=False)
        inputs = torch.empty((N, C, H, W), dtype=torch.float32, device=dev)
        labels = torch.empty((N, 1, H, W), dtype=torch.float32, device=dev)
        at = 0
        try:
            for _ in range(len(loader)):
                x, y = loader.next()
                if recipe is None:
                    inputs[at:at + x.shape[0]].copy_(x.detach())
                else:
                    compose_features(x.detach(), recipe, out=inputs[at:at + x.shape[0]])
                labels[at:at + x.shape[0]].copy_(y)
                at += x.shape[0]
        finally:
            loader.close()
        if at != N:
            raise ValueError(f"patch sampler: {data_dir} gave {at} frames of {N}")
        if kw.get("stats") is None:
            kw["stats"] = load_stats(stats_dir or data_dir, C)
        return cls(inputs, labels, **kw)

    # ---- the stream ---------------------------------------------------------------
    @property
    def step(self):
        """The step the next batch is drawn for (capturable: reads the device)."""
        return int(self._words[1].item()) if self.capturable else self._step

    def draws(self, step):
        """The draws of `step` as the kernel makes them: int32 [batch, 8] on the
        host, no GPU involved (see patch_draws)."""
        return patch_draws(self.seed, self.rank, step, self.batch, frame=(self.H, self.W),
                           patch=self.patch, lo=self.lo, count=self.count, order=self.order,
                           align=self.align, hflip=self.hflip, vflip=self.vflip, emitters=self.E)

    def state_dict(self):
        return {"seed": self.seed, "step": self.step, "order": self.order, "rank": self.rank}

    def load_state_dict(self, state):
        """Continue the stream of `state`: its seed and step are taken over
        (capturable: one upload into the device words, no re-capture); its order
        and rank must be this sampler's."""
        if state["order"] != self.order or state["rank"] != self.rank:
            raise ValueError(f"patch sampler: the state is of order {state['order']!r}, rank "
                             f"{state['rank']}; this sampler is {self.order!r}, rank {self.rank}")
        seed, step = state["seed"], _int_arg(state["step"], "step", 0)
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed <= _M64:
            raise ValueError(f"patch sampler: seed must be an integer in [0, 2^64), got {seed!r}")
        self.seed, self._step = seed, step
        if self.capturable:
            self._words.copy_(torch.tensor([_as_i64(seed), step], dtype=torch.int64))

    def next(self, out=None):
        """(x [B,C,ph,pw] normalised, y [B,1,ph,pw]) of the next step, fp32. out =
        (x, y): written in place (the static buffers of a GraphedTrainStep),
        nothing is copied; without it both are allocated and x requires grad,
        as the loaders' batches do. One launch (capturable: two), no host
        synchronisation."""
        dev = self.inputs.device
        if dev.type != "cuda":
            raise ValueError(f"patch sampler: the pool must be on a ROCm GPU device (got {dev}); "
                             "the gather has no CPU implementation")
        B, C, (ph, pw) = self.batch, self.C, self.patch
        if out is None:
            x = torch.empty((B, C, ph, pw), dtype=torch.float32, device=dev)
            y = torch.empty((B, 1, ph, pw), dtype=torch.float32, device=dev)
        else:
            try:
                x, y = out
            except (TypeError, ValueError):
                raise ValueError("patch sampler: out must be an (x, y) pair of tensors") from None
            for t, shape, name in ((x, (B, C, ph, pw), "x"), (y, (B, 1, ph, pw), "y")):
                if (not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.float32
                        or t.device != dev or not t.is_contiguous()):
                    got = (tuple(t.shape), t.dtype, str(t.device)) if torch.is_tensor(t) else \
                        type(t).__name__
                    raise ValueError(f"patch sampler: out {name} must be a contiguous {shape} "
                                     f"torch.float32 tensor on {dev}, got {got}")
        if self.record_draws and (self.last_draws is None or not self.capturable):
            self.last_draws = torch.empty((B, 8), dtype=torch.int32, device=dev)
        seed_dev = step_dev = None
        if self.capturable:
            seed_dev, step_dev = self._words.data_ptr(), self._words.data_ptr() + 8
        call("nsm_patch_gather", ptr(self.inputs), ptr(self.labels), self.N, C, self.E, self.H,
             self.W, B, ph, pw, ptr(self.means), ptr(self.stds), float(self.eps),
             ptr(self.hflip_sign), ptr(self.vflip_sign), self.emitter_channel,
             ptr(self.emitter_values), ORDERS.index(self.order), self.align, int(self.hflip),
             int(self.vflip), self.lo, self.count, self.rank, self.seed, seed_dev, self._step,
             step_dev, ptr(x), ptr(y), ptr(self.last_draws) if self.record_draws else None, stream())
        if self.capturable:
            call("nsm_patch_advance", step_dev, stream())
        else:
            self._step += 1
        return (x.requires_grad_(True), y) if out is None else (x, y)
