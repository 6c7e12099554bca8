"""Per-channel dataset statistics on the device: the `train_stats.json` that
FrameLoader and MmapLiverDataset normalise with (the reference's
calculate_dataset_stats.py), the per-frame min / max / mean / std table of its
check_channel_stats.py, and the dataset sigma_i of the paper's Eq. 1
(nsm_amd/sensitivity.py), from one read of the raw frames as the native loader
delivers them.

Two launches per batch (csrc/nsm_stats.hip): nsm_stats_partial writes one fp64
record {count, mean, M2, min, max, nonfinite} per block of every (frame,
channel) plane, nsm_stats_merge folds them in a fixed order into the optional
per-frame table [B,C,6] and the running state [C,6], which stays on the device
across batches. Records merge by Chan's pairwise rule, so a channel far from
zero (a depth of 1000 with a spread of 0.01) loses nothing to cancellation, and
the fixed order makes the same call sequence give the same bits. Non-finite
samples are counted per channel and left out of the other figures. Nothing
synchronises with the host: the results are device tensors, and reading them is
the only wait (dataset_stats reads them: it writes a file).
"""
import json
import os
from collections import namedtuple

import torch

from ._lib import NsmError, call, lib, ptr, require_gpu, stream

REC = 6   # doubles of a record: count, mean, M2, min, max, nonfinite
_NONFINITE = ("raise", "skip")


class StatsResult(namedtuple("StatsResult", "count means stds mins maxs nonfinite")):
    """Per channel: `count` finite samples (int64), `means` and population
    `stds` (fp64, ddof = 0, as the reference's dataset figure), `mins` and
    `maxs` (fp32, the samples' own type; +inf / -inf without a finite sample)
    and the number of `nonfinite` samples (int64)."""
    __slots__ = ()

    def std(self, unbiased=True):
        """The n - 1 form (NaN below two samples, as torch.std); unbiased=False: `stds`."""
        if not unbiased:
            return self.stds
        n = self.count.to(torch.float64)
        return self.stds * torch.sqrt(n / (n - 1))


def _empty_state(channels, device):
    st = torch.zeros((channels, REC), dtype=torch.float64, device=device)
    st[:, 3] = float("inf")
    st[:, 4] = float("-inf")
    return st


def _check_channels(channels):
    if isinstance(channels, bool) or not isinstance(channels, int) or channels < 1:
        raise ValueError(f"channel stats: channels must be an integer >= 1, got {channels!r}")
    return channels


def _check_input(x, channels=None):
    """Host-side argument checks (no GPU work)."""
    if not torch.is_tensor(x) or x.dim() != 4:
        got = tuple(x.shape) if torch.is_tensor(x) else type(x).__name__
        raise ValueError(f"channel stats: x must be a [B,C,H,W] tensor, got {got}")
    if x.dtype != torch.float32:
        raise ValueError(f"channel stats: x must be float32 (the raw frames), got {x.dtype}")
    if min(x.shape) < 1:
        raise ValueError(f"channel stats: empty input {tuple(x.shape)}")
    if channels is not None and x.shape[1] != channels:
        raise ValueError(f"channel stats: x has {x.shape[1]} channels, expected {channels}")
    if lib.nsm_stats_blocks(x.shape[2] * x.shape[3]) <= 0:
        raise ValueError(f"channel stats: unsupported plane size {x.shape[2]} x {x.shape[3]}")


class ChannelStats:
    """Running statistics of `channels` channels: update(x) per batch, compute()
    for the result so far, merge(other) for another accumulator's share (a
    second rank's shard), reset() to start over. The state is a [C,6] fp64
    device tensor; compute() returns device tensors without a host
    synchronisation."""

    def __init__(self, channels):
        self.channels = _check_channels(channels)
        self._state = None
        self._ws = None

    def reset(self):
        if self._state is not None:   # in place: a captured update keeps its pointer
            self._state.copy_(_empty_state(self.channels, self._state.device))

    def _on(self, device):
        if self._state is None:
            self._state = _empty_state(self.channels, device)
        elif self._state.device != device:
            raise ValueError(f"channel stats: the state lives on {self._state.device}, "
                             f"got a tensor on {device}")
        return self._state

    def update(self, x, per_frame=False):
        """Fold x [B,C,H,W] (fp32, on the GPU) in. per_frame=True returns the
        batch's own [B,C,6] fp64 records {count, mean, M2, min, max, nonfinite}."""
        _check_input(x, self.channels)
        dev = require_gpu(x, "channel-stats input").device
        x = x.detach().contiguous()
        B, C, H, W = x.shape
        per = lib.nsm_stats_blocks(H * W)
        state = self._on(dev)
        need = B * C * per * REC
        if self._ws is None or self._ws.device != dev or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.float64, device=dev)
        frames = torch.empty((B, C, REC), dtype=torch.float64, device=dev) if per_frame else None
        call("nsm_stats_partial", ptr(x), B, C, H * W, ptr(self._ws), stream())
        call("nsm_stats_merge", ptr(self._ws), B, C, per, ptr(frames), ptr(state), stream())
        return frames

    def merge(self, other):
        """Chan-merge another accumulator's state, or a StatsResult, into this one."""
        if isinstance(other, StatsResult):
            n = other.count.to(torch.float64)
            rec = torch.stack([n, other.means, other.stds * other.stds * n,
                               other.mins.to(torch.float64), other.maxs.to(torch.float64),
                               other.nonfinite.to(torch.float64)], dim=1).contiguous()
        elif isinstance(other, ChannelStats):
            rec = other._state
        else:
            raise ValueError(f"channel stats: cannot merge a {type(other).__name__}")
        if rec is None:
            return self
        if rec.shape[0] != self.channels:
            raise ValueError(f"channel stats: merging {rec.shape[0]} channels into {self.channels}")
        dev = require_gpu(rec, "channel-stats state").device
        call("nsm_stats_merge", ptr(rec), 1, self.channels, 1, None, ptr(self._on(dev)), stream())
        return self

    def compute(self):
        if self._state is None:
            raise RuntimeError("ChannelStats.compute() before the first update()")
        return result_of(self._state)


def result_of(records):
    """StatsResult of records [..., 6] (the state, or a per-frame table)."""
    n, mean, m2, mn, mx, bad = records.unbind(-1)
    var = torch.where(n > 0, m2 / n.clamp_min(1.0), torch.zeros_like(m2))
    return StatsResult(n.to(torch.int64), mean, torch.sqrt(var), mn.to(torch.float32),
                       mx.to(torch.float32), bad.to(torch.int64))


def channel_stats(x):
    """StatsResult of one tensor x [B,C,H,W] (fp32, on the GPU)."""
    _check_input(x)
    acc = ChannelStats(x.shape[1])
    acc.update(x)
    return acc.compute()


def stats_json(means, stds):
    """The text of train_stats.json as the reference's calculate_dataset_stats.py
    writes it: the keys `means` and `stds`, lists of Python floats, indent 4."""
    def floats(v):
        if torch.is_tensor(v):
            v = v.detach().to("cpu", torch.float64)
        return [float(t) for t in v]

    means, stds = floats(means), floats(stds)
    if len(means) != len(stds) or not means:
        raise ValueError(f"stats json: {len(means)} means and {len(stds)} stds")
    return json.dumps({"means": means, "stds": stds}, indent=4)


def save_stats(stats_dir, means, stds):
    """Write train_stats.json (never the pickled .npy) into stats_dir; returns the path."""
    path = os.path.join(stats_dir, "train_stats.json")
    text = stats_json(means, stds)
    with open(path, "w", encoding="utf-8") as f:
        f.write(text)
    return path


def dataset_stats(data_dir, split="train", batch=8, device="cuda", world=1, rank=0, save=True,
                  nonfinite="raise", per_frame=False, recipe=None):
    """Statistics of `{split}_inputs.npy` under data_dir, streamed raw through
    FrameLoader (this rank's shard, the short last batch included). Returns the
    StatsResult, and with per_frame=True also the [N,C,6] fp64 table of every
    frame's record {count, mean, M2, min, max, nonfinite}.

    save=True writes `train_stats.json` into data_dir in the reference's shape;
    it needs the whole split (world == 1): merge shards with ChannelStats.merge
    and write with save_stats. nonfinite="raise" raises ValueError naming the
    channels that hold NaN or Inf and how many; "skip" accepts them (they are
    left out of the figures either way). recipe (a features.FeatureRecipe): every
    uploaded batch is composed on the device (frames.compose_features, no scrub)
    before it is folded in, so the figures, and the file, are those of the
    recipe's channels: what a model trained on them normalises with."""
    from .data import FrameLoader
    from .frames import compose_features
    if nonfinite not in _NONFINITE:
        raise ValueError(f"dataset stats: nonfinite must be one of {_NONFINITE}, got {nonfinite!r}")
    if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
        raise ValueError(f"dataset stats: batch must be an integer >= 1, got {batch!r}")
    if save and world != 1:
        raise ValueError("dataset stats: save=True needs the whole split (world=1); merge the "
                         "shards with ChannelStats.merge and write with save_stats")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise NsmError(f"dataset stats run on a ROCm GPU device (got {dev}); "
                       "the nsm_amd path has no CPU implementation")
    loader = FrameLoader(data_dir, split=split, batch=batch, device=dev, world=world, rank=rank,
                         apply_normalization=False)
    try:
        if recipe is not None:
            recipe.check_input(loader.C, "dataset stats")
        acc = ChannelStats(loader.C if recipe is None else recipe.out_channels)
        tables = []
        for _ in range(len(loader)):
            x, _ = loader.next()
            x = x.detach()
            if recipe is not None:
                x = compose_features(x, recipe)
            t = acc.update(x, per_frame=per_frame)
            if per_frame:
                tables.append(t)
        res = acc.compute()
    finally:
        loader.close()
    bad = res.nonfinite.tolist()
    if nonfinite == "raise" and any(bad):
        raise ValueError("dataset stats: non-finite samples in " + ", ".join(
            f"channel {c} ({k})" for c, k in enumerate(bad) if k))
    if save:
        save_stats(data_dir, res.means, res.stds)
    return (res, torch.cat(tables)) if per_frame else res
