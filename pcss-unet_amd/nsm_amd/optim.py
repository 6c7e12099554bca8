"""Train-step tail on libnsm kernels over ONE flat parameter buffer, and the
data-parallel gradient all-reduce.

Reference step tail (main.py:281-423, optimizer/scheduler main.py:952-969):

    backward -> [sanitise: NaN/Inf census, skip if >20 % of a tensor is bad,
    else repair NaN->mean+noise, Inf->+-10*max (:287-354)] -> per-parameter
    pre-unscale clip to 1000*scale (:361-365) -> unscale_ -> per-parameter
    NaN/Inf skip, norm > 1e5 skip, norm > 1e3 rescale to 1e3 (:368-402) ->
    clip_grad_norm_(max_norm) with max_norm = 1.0, or max(0.1, 1-epoch/E)
    after half the epochs (:357-358,405) -> skip if a clipped norm > 10
    (:408-418) -> AdamW step (:421) ; LambdaLR warmup + cosine (:959-969).

`FlatAdamW(..., sanitize=True)` runs all of that on the device as a fixed
sequence of five kernels (include/nsm.h `nsm_grad_tail` + `nsm_adamw_tail`):
every decision the reference takes on the host becomes a device flag that the
next kernel reads, the AdamW step count lives on the device (a skipped step
does not advance it, exactly like a `continue` before `optimizer.step()`), and
nothing synchronises with the host. `sanitize=False` is the plain
clip_grad_norm_ + AdamW tail.

`FlatAdamW` re-homes the parameters into a single contiguous fp32 buffer
(views keep the module's parameter objects, so state_dict / LambdaLR /
named_parameters are unchanged). The Unet backward writes all 66 gradients
into one flat buffer too, so the DP exchange is one all-reduce of 60 MiB.
`state_dict()` / `load_state_dict()` use torch.optim.AdamW's format, so
main.py's `optimizer_state_dict` checkpoints interchange.

main.py:952-957 builds Adam, AdamW or (for any other `optimizer_type`) SGD with
momentum. `FlatAdam` and `FlatSGD` are the other two on the same flat buffer
and the same device tail: everything up to the update (`nsm_grad_tail`) is
shared, only the last kernel differs (`nsm_adam_tail` / `nsm_sgd_tail`), and
their checkpoints are torch.optim.Adam's / torch.optim.SGD's.
`make_optimizer(params, optimizer_type, lr)` is that three-way block.

The loss scale of the fp16 mode is either a constant (`grad_scale=`, a kernel
argument of `nsm_grad_tail`) or an `nsm_amd.GradScaler` (`grad_scaler=`): then
the tail is `nsm_grad_tail_scaled`, which reads the scale from the scaler's
device state and applies torch.amp.GradScaler's update rule to it in the same
finalize kernel (grad_scaler.py).

lr and max_norm are kernel arguments too, unless the optimizer is built with
`device_hyper=True` (sanitize=True only): then they live in a 16-byte device
block (a double lr, a float max_norm) that the `*_dev` entries of the same
kernels read, and `sync_hyper()` uploads the host group's lr and the current
max_norm whenever they differ from the pair last uploaded (`nsm_hyper_set`, the
values as arguments of a one-thread launch). `step()` calls it unless the
stream is capturing; GraphedTrainStep calls it before each replay. So a
LambdaLR / ReduceLROnPlateau / `set_epoch` / `load_state_dict` change reaches a
captured step with no new capture. The host group's lr stays the truth:
`state_dict()` is unchanged.
"""
import math
import os

import torch
import torch.distributed as dist

from ._lib import call, lib, ptr, stream


def flat_grad(params):
    """The flat tensor backing all .grad views (in parameter order), or None."""
    gs = [p.grad for p in params]
    if any(g is None for g in gs):
        return None
    base = gs[0]
    st = base.untyped_storage()
    off = base.storage_offset()
    for g in gs:
        if g.untyped_storage().data_ptr() != st.data_ptr() or g.storage_offset() != off \
                or not g.is_contiguous():
            return None
        off += g.numel()
    total = off - base.storage_offset()
    return torch.empty(0, dtype=base.dtype, device=base.device).set_(
        st, base.storage_offset(), (total,), (1,))


# Gradient all-reduces already in flight for a flat gradient buffer, issued by
# the Unet backward as soon as a contiguous bucket of it is final:
# {storage ptr: (flat tensor kept alive, [async work handles])}. Only one
# step's buffer is ever outstanding.
_PENDING = {}


def allreduce_async(flat, lo, hi, group=None):
    """Start the (sum) all-reduce of flat[lo:hi] on RCCL's stream, ordered after
    the work already queued on the current stream; allreduce_grads() waits."""
    key = flat.untyped_storage().data_ptr()
    ent = _PENDING.get(key)
    if ent is None or ent[0] is not flat:
        _PENDING.clear()
        ent = _PENDING[key] = (flat, [])
    ent[1].append(dist.all_reduce(flat[lo:hi], group=group, async_op=True))
    spans = getattr(flat, "_nsm_spans", None)
    if spans is None:
        spans = flat._nsm_spans = []
    spans.append((lo, hi))


def allreduce_grads(params, group=None):
    """Sum grads over ranks (RCCL over xGMI); averaging is folded into the
    optimizer (inv_world). If the backward already put the buckets of this flat
    buffer in flight (Unet.overlap_grad_allreduce), this only makes the current
    stream wait for them."""
    params = list(params)
    g = flat_grad(params)
    if g is not None:
        ent = _PENDING.pop(g.untyped_storage().data_ptr(), None)
        if ent is not None:
            flat, works = ent
            covered = sum(w_hi - w_lo for w_lo, w_hi in getattr(flat, "_nsm_spans", []))
            for w in works:
                w.wait()
            if covered == g.numel():
                return
            raise RuntimeError("pending gradient buckets do not cover the flat buffer")
    if g is None:
        for p in params:
            if p.grad is not None:
                dist.all_reduce(p.grad, group=group)
    else:
        dist.all_reduce(g, group=group)


# ---- schedules of main.py ---------------------------------------------------
def lr_lambda(warmup_epochs=5, num_epochs=200):
    """main.py:959-967 `get_lr_lambda`: linear warmup from 0 (epoch 0 -> lr 0),
    then cosine to a floor of 1 % — pass to torch.optim.lr_scheduler.LambdaLR."""
    def f(epoch):
        if epoch < warmup_epochs:
            return float(epoch) / float(max(1, warmup_epochs))
        decay = 0.5 * (1.0 + math.cos(math.pi * (epoch - warmup_epochs)
                                      / (num_epochs - warmup_epochs)))
        return max(0.01, decay)
    return f


def make_lambda_lr(optimizer, warmup_epochs=5, num_epochs=200):
    """The reference's scheduler (main.py:969) on any optimizer (FlatAdamW included)."""
    return torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=lr_lambda(warmup_epochs,
                                                                            num_epochs))


def max_norm_for(epoch, num_epochs):
    """main.py:357-358: clip_grad_norm_ threshold of an epoch."""
    r = epoch / num_epochs
    return 1.0 if r < 0.5 else max(0.1, 1.0 - r)


FLAG_NAMES = ("skip", "repaired", "severe", "nonfinite", "huge", "postclip", "n_rescaled",
              "n_zeroed")


def _bump(params):
    """The parameters were rewritten in place by HIP kernels, invisibly to
    autograd's version counters: bump them, so caches keyed on the versions
    (infer.GraphedUnet's frozen weight layouts) see the change."""
    with torch.no_grad():
        for p in params:
            torch.autograd.graph.increment_version(p)


class _FlatOptimizer(torch.optim.Optimizer):
    """What FlatAdamW, FlatAdam and FlatSGD share: the parameters re-homed into
    one flat fp32 buffer, the block plan and workspace of the device tail, the
    DP averaging (inv_world) and the rank-0 repair seed, the max_norm schedule,
    the `nsm_grad_tail` call and the inspection helpers. A subclass allocates
    its state (`_alloc_state`), launches its update kernel (`_tail_update` after
    nsm_grad_tail, `_plain_update` for sanitize=False) and names the torch
    optimizer whose checkpoint format it reads and writes (`_TORCH`)."""
    _TORCH = None
    # group options the kernels do not implement: {key: the only value accepted}
    _REFUSED = {}

    def __init__(self, params, defaults, max_grad_norm=None, world_size=1, sanitize=False,
                 grad_scale=1.0, seed=None, grad_scaler=None, device_hyper=False):
        params = list(params)
        if device_hyper and not sanitize:
            raise ValueError(f"{type(self).__name__}: device_hyper needs sanitize=True (the "
                             "device tail is what reads lr and max_norm from the hyper block)")
        if grad_scaler is not None:
            if float(grad_scale) != 1.0:
                raise ValueError(f"{type(self).__name__}: grad_scale is the static loss scale; "
                                 "with grad_scaler= the scale is the scaler's")
            if grad_scaler.is_enabled() and not sanitize:
                raise ValueError(f"{type(self).__name__}: grad_scaler needs sanitize=True (the "
                                 "device tail is what unscales and updates the scale)")
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError(f"{type(self).__name__} supports one param group")
        params = self.param_groups[0]["params"]
        dev = params[0].device
        total = sum(p.numel() for p in params)
        self.flat = torch.empty(total, dtype=torch.float32, device=dev)
        off = 0
        offs = [0]
        with torch.no_grad():
            for p in params:
                n = p.numel()
                self.flat[off:off + n].copy_(p.detach().reshape(-1))
                p.data = self.flat[off:off + n].view_as(p)
                off += n
                offs.append(off)
        self._alloc_state()
        self.max_grad_norm = max_grad_norm
        self.world_size = world_size
        self.inv_world = 1.0 / world_size
        self.sanitize = sanitize
        self.grad_scale = float(grad_scale)
        # nsm_amd.GradScaler: the loss scale is device state the tail reads and
        # updates (a disabled one is kept for scaler.step(), and changes nothing)
        self.grad_scaler = grad_scaler
        self._scaler = grad_scaler if grad_scaler is not None and grad_scaler.is_enabled() \
            else None
        self.step_count = 0          # host count (sanitize=False: no step is ever skipped)
        nb = lib.nsm_loss_blocks(total)
        self._partial = torch.empty(nb, dtype=torch.float32, device=dev)
        self._sumsq = torch.empty((), dtype=torch.float32, device=dev)
        self._coef = torch.empty((), dtype=torch.float32, device=dev)
        # device state of the reference tail: [optimizer steps taken, tail calls]
        self._step_dev = torch.zeros(2, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(8, dtype=torch.int32, device=dev)
        self.stat = torch.zeros(4, dtype=torch.float32, device=dev)
        if sanitize:
            self._plan(offs, dev)
        # device_hyper: lr and max_norm live in a device block the tail reads
        # (include/nsm.h, nsm_hyper_set), so a captured step follows a schedule
        self.device_hyper = bool(device_hyper)
        self._hyper_dev = None
        self._hyper_sent = None      # the (lr, max_norm) pair last uploaded
        if self.device_hyper:
            self._hyper_dev = torch.zeros(int(lib.nsm_hyper_bytes()), dtype=torch.uint8,
                                          device=dev)
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little") >> 1
            # data parallel: every rank must draw the same repair noise, or the
            # replicas diverge at the first NaN repair (all ranks hold the same
            # averaged gradient) -> rank 0's seed everywhere
            if world_size > 1 and dist.is_available() and dist.is_initialized():
                bdev = dev if dist.get_backend() == "nccl" else torch.device("cpu")
                t = torch.tensor([seed], dtype=torch.int64, device=bdev)
                dist.broadcast(t, 0)
                seed = int(t.item())
        self.seed = seed

    def _plan(self, offs, dev):
        import ctypes
        nseg = len(offs) - 1
        seg_off = (ctypes.c_int64 * (nseg + 1))(*offs)
        nblk = lib.nsm_tail_plan(seg_off, nseg, None, None, None, None, 0)
        blk_seg = (ctypes.c_int * nblk)()
        blk_lo = (ctypes.c_int64 * nblk)()
        blk_hi = (ctypes.c_int64 * nblk)()
        seg_blk = (ctypes.c_int * (nseg + 1))()
        if lib.nsm_tail_plan(seg_off, nseg, blk_seg, blk_lo, blk_hi, seg_blk, nblk) != nblk:
            raise RuntimeError("nsm_tail_plan failed")
        t = lambda a, dt: torch.tensor(list(a), dtype=dt).to(dev)  # noqa: E731
        self._nseg, self._nblk = nseg, nblk
        self._seg_off = t(seg_off, torch.int64)
        self._seg_blk = t(seg_blk, torch.int32)
        self._blk_seg = t(blk_seg, torch.int32)
        self._blk_lo = t(blk_lo, torch.int64)
        self._blk_hi = t(blk_hi, torch.int64)
        nbytes = int(lib.nsm_tail_ws_bytes(nseg, nblk))
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._seg_coef = torch.zeros(4 * nseg, dtype=torch.float32, device=dev)

    # ---- what a subclass provides --------------------------------------------
    def _alloc_state(self):
        raise NotImplementedError

    def _tail_update(self, g, grp, st):
        """The update kernel after nsm_grad_tail (reads flags / seg_coef / the
        device step count)."""
        raise NotImplementedError

    def _plain_update(self, g, n, grp, coef, st):
        """The sanitize=False update (host step count self.step_count)."""
        raise NotImplementedError

    def _moments(self):
        """The flat state tensors the update kernel writes."""
        raise NotImplementedError

    def _hyper_keys(self):
        raise NotImplementedError

    # ---- what GraphedTrainStep needs -----------------------------------------
    def step_state(self):
        """Every tensor a step writes besides its scratch: the flat parameters,
        the optimizer's flat state, the tail's device counters and flags (and
        the grad scaler's device state)."""
        st = [self.flat] + self._moments() + [self._step_dev, self.flags, self.stat]
        if self._scaler is not None:
            st.append(self._scaler.state_tensor())
        return st

    def step_hyper(self):
        """The hyper-parameters a step passes as kernel arguments (a captured
        graph freezes them: a change needs a new capture). With device_hyper,
        lr and max_norm are not among them: the tail reads them from the hyper
        block, a constant of the step that sync_hyper() rewrites between steps
        (so it is no part of step_state() either)."""
        g = self.param_groups[0]
        keys = [k for k in self._hyper_keys() if not (self.device_hyper and k == "lr")]
        vals = tuple(tuple(g[k]) if isinstance(g[k], (tuple, list)) else float(g[k])
                     for k in keys)
        if not self.device_hyper:
            vals += (self.max_grad_norm,)
        if self._scaler is not None:
            # the scale itself is device state: its changes need no new capture
            return vals + (self._scaler.tail_args(),)
        return vals + (self.grad_scale,)

    def _hyper_pair(self):
        mx = float(self.max_grad_norm) if self.max_grad_norm is not None else float("inf")
        return (float(self.param_groups[0]["lr"]), mx)

    def sync_hyper(self):
        """device_hyper: upload (lr, max_norm) to the hyper block if they differ
        from the pair last uploaded (the first call always uploads): one
        one-thread launch on the current stream, no host wait. The values are
        arguments of that launch, so uploads and replays may be queued back to
        back. On a capturing stream it raises: a recorded upload would write
        the captured values back on every replay."""
        if not self.device_hyper:
            return
        pair = self._hyper_pair()
        if pair == self._hyper_sent:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{type(self).__name__}.sync_hyper: the stream is capturing; call "
                               "it before the capture and before each replay")
        with torch.cuda.device(self._hyper_dev.device):
            call("nsm_hyper_set", ptr(self._hyper_dev), pair[0], pair[1], stream())
        self._hyper_sent = pair

    def hyper_values(self):
        """device_hyper: {"lr", "max_norm"} as the hyper block holds them (host
        sync; for inspection, like last_flags())."""
        if not self.device_hyper:
            raise RuntimeError(f"{type(self).__name__}: built without device_hyper=True")
        raw = self._hyper_dev.cpu()
        return {"lr": float(raw[:8].view(torch.float64)[0].item()),
                "max_norm": float(raw[8:12].view(torch.float32)[0].item())}

    # main.py:357-358
    def set_epoch(self, epoch, num_epochs):
        """Apply the reference's max_norm schedule for `epoch` of `num_epochs`."""
        self.max_grad_norm = max_norm_for(epoch, num_epochs)

    @torch.no_grad()
    def step(self, closure=None, noise=None):
        """One tail step. `noise` (flat like the gradient, sanitize=True only)
        supplies the randn values of the NaN repair (main.py:336) for parity
        tests; otherwise a counter-based device generator draws them."""
        params = self.param_groups[0]["params"]
        g = flat_grad(params)
        if g is None:
            g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1)
                           for p in params])
        grp = self.param_groups[0]
        n = self.flat.numel()
        st = stream()
        if self.sanitize:
            if self.device_hyper:
                # the *_dev entries read max_norm (and lr) from the hyper block. A
                # captured upload would write the frozen values back on every
                # replay: under capture the block is the caller's to keep current
                # (GraphedTrainStep, or sync_hyper() before graph.replay())
                if not torch.cuda.is_current_stream_capturing():
                    self.sync_hyper()
                sfx, mx = "_dev", ptr(self._hyper_dev)
            else:
                sfx = ""
                mx = float(self.max_grad_norm) if self.max_grad_norm is not None else float("inf")
            if self._scaler is not None:
                call("nsm_grad_tail_scaled" + sfx, ptr(g), self._nseg, ptr(self._seg_off),
                     ptr(self._seg_blk), ptr(self._blk_seg), ptr(self._blk_lo), ptr(self._blk_hi),
                     self._nblk, self.inv_world, ptr(self._scaler.state_tensor()), mx, ptr(noise),
                     self.seed, ptr(self._ws), self._ws.numel(), ptr(self._seg_coef),
                     ptr(self.stat), ptr(self.flags), ptr(self._step_dev),
                     *self._scaler.tail_args(), st)
            else:
                call("nsm_grad_tail" + sfx, ptr(g), self._nseg, ptr(self._seg_off),
                     ptr(self._seg_blk), ptr(self._blk_seg), ptr(self._blk_lo), ptr(self._blk_hi),
                     self._nblk, self.inv_world, self.grad_scale, mx, ptr(noise), self.seed,
                     ptr(self._ws), self._ws.numel(), ptr(self._seg_coef), ptr(self.stat),
                     ptr(self.flags), ptr(self._step_dev), st)
            self._tail_update(g, grp, st)
            _bump(params)
            return None
        self.step_count += 1
        coef = None
        if self.max_grad_norm is not None or self.inv_world != 1.0:
            call("nsm_sumsq", ptr(g), n, ptr(self._partial), ptr(self._sumsq), st)
            mx = float(self.max_grad_norm) if self.max_grad_norm is not None else float("inf")
            call("nsm_clip_coef", ptr(self._sumsq), self.inv_world, mx, ptr(self._coef), st)
            coef = self._coef
        self._plain_update(g, n, grp, coef, st)
        _bump(params)
        return None

    def zero_grad(self, set_to_none=True):
        for p in self.param_groups[0]["params"]:
            p.grad = None

    # ---- inspection (these synchronise; not for the hot loop) ----------------
    def steps_taken(self):
        return int(self._step_dev[0].item()) if self.sanitize else self.step_count

    def last_flags(self):
        """{name: value} of the last sanitised step's decisions (host sync)."""
        f = self.flags.tolist()
        d = dict(zip(FLAG_NAMES, f))
        s = self.stat.tolist()
        d.update(total_norm=s[0], clip_coef=s[1], max_norm=s[2], max_clipped_norm=s[3])
        return d

    # ---- the torch twin's checkpoint format -----------------------------------
    def _torch_group_defaults(self):
        ref = self._TORCH([torch.zeros(1)], lr=1e-3)
        d = dict(ref.defaults)
        d.update({k: v for k, v in self.param_groups[0].items() if k != "params"})
        return d

    def _check_refused(self, opts):
        for k, ok in self._REFUSED.items():
            if k in opts and opts[k] != ok:
                raise ValueError(f"{type(self).__name__} does not implement {k}={opts[k]!r}")

    def _load_group(self, sd, keys):
        """Check a torch state_dict's single group against ours and take its
        hyper-parameters; returns the group."""
        params = self.param_groups[0]["params"]
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(params):
            raise ValueError(f"state_dict does not match {type(self).__name__}'s single "
                             "parameter group")
        grp = groups[0]
        self._check_refused(grp)
        for k in keys + ("initial_lr",):
            if k in grp:
                self.param_groups[0][k] = grp[k]
        return grp

    def _set_steps(self, s):
        self.step_count = s
        self._step_dev[0] = s


class _FlatAdamFamily(_FlatOptimizer):
    """Adam-type state: two flat moments and one step count, checkpointed as
    torch's `step` / `exp_avg` / `exp_avg_sq` per parameter."""
    _TAIL = _STEP = None

    def _alloc_state(self):
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)

    def _moments(self):
        return [self.exp_avg, self.exp_avg_sq]

    def _hyper_keys(self):
        return ("lr", "betas", "eps", "weight_decay")

    def _tail_update(self, g, grp, st):
        b1, b2 = grp["betas"]
        # device_hyper: the entry that reads lr from the hyper block
        name, lr = (self._TAIL + "_dev", ptr(self._hyper_dev)) if self.device_hyper \
            else (self._TAIL, float(grp["lr"]))
        call(name, ptr(self.flat), ptr(g), ptr(self.exp_avg), ptr(self.exp_avg_sq),
             ptr(self._blk_seg), ptr(self._blk_lo), ptr(self._blk_hi), self._nblk,
             ptr(self._seg_coef), ptr(self.flags), ptr(self._step_dev), lr,
             float(b1), float(b2), float(grp["eps"]), float(grp["weight_decay"]), st)

    def _plain_update(self, g, n, grp, coef, st):
        b1, b2 = grp["betas"]
        call(self._STEP, ptr(self.flat), ptr(g), ptr(self.exp_avg), ptr(self.exp_avg_sq), n,
             float(grp["lr"]), float(b1), float(b2), float(grp["eps"]), float(grp["weight_decay"]),
             self.step_count, ptr(coef), st)

    def state_dict(self):
        params = self.param_groups[0]["params"]
        step = float(self.steps_taken())
        state, off = {}, 0
        for i, p in enumerate(params):
            n = p.numel()
            if step > 0:
                state[i] = {"step": torch.tensor(step),
                            "exp_avg": self.exp_avg[off:off + n].view_as(p).clone(),
                            "exp_avg_sq": self.exp_avg_sq[off:off + n].view_as(p).clone()}
            off += n
        grp = self._torch_group_defaults()
        grp["params"] = list(range(len(params)))
        return {"state": state, "param_groups": [grp]}

    def load_state_dict(self, sd):
        params = self.param_groups[0]["params"]
        grp = self._load_group(sd, ("lr", "betas", "eps", "weight_decay"))
        steps = set()
        off = 0
        with torch.no_grad():
            for i, p in enumerate(params):
                n = p.numel()
                st = sd["state"].get(i, sd["state"].get(grp["params"][i]))
                if st is not None:
                    self.exp_avg[off:off + n].copy_(st["exp_avg"].reshape(-1))
                    self.exp_avg_sq[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
                    steps.add(int(float(st["step"])))
                else:
                    self.exp_avg[off:off + n].zero_()
                    self.exp_avg_sq[off:off + n].zero_()
                    steps.add(0)
                off += n
        if len(steps) != 1:
            raise ValueError(f"{type(self).__name__} keeps one step count; checkpoint has "
                             f"{sorted(steps)}")
        self._set_steps(steps.pop())


class FlatAdamW(_FlatAdamFamily):
    """main.py:955 `optim.AdamW(lr, weight_decay=1e-3)` (decoupled weight decay)."""
    _TORCH = torch.optim.AdamW
    _TAIL, _STEP = "nsm_adamw_tail", "nsm_adamw_step"

    def __init__(self, params, lr=7e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3,
                 max_grad_norm=None, world_size=1, sanitize=False, grad_scale=1.0, seed=None,
                 grad_scaler=None, device_hyper=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay),
                         max_grad_norm, world_size, sanitize, grad_scale, seed, grad_scaler,
                         device_hyper)


class FlatAdam(_FlatAdamFamily):
    """main.py:953 `optim.Adam(lr, weight_decay=1e-4)`: L2 weight decay added to
    the gradient before the moments (torch.optim.Adam's single-tensor path)."""
    _TORCH = torch.optim.Adam
    _TAIL, _STEP = "nsm_adam_tail", "nsm_adam_step"
    _REFUSED = {"amsgrad": False, "maximize": False}

    def __init__(self, params, lr=7e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4,
                 max_grad_norm=None, world_size=1, sanitize=False, grad_scale=1.0, seed=None,
                 amsgrad=False, maximize=False, grad_scaler=None, device_hyper=False):
        self._check_refused(dict(amsgrad=amsgrad, maximize=maximize))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay),
                         max_grad_norm, world_size, sanitize, grad_scale, seed, grad_scaler,
                         device_hyper)


class FlatSGD(_FlatOptimizer):
    """main.py:957 `optim.SGD(lr, momentum=0.9, weight_decay=1e-4)`: dampening
    0, no Nesterov. One flat momentum buffer (none at momentum=0). As in torch,
    the buffer starts as the first gradient that is actually stepped: the
    kernels take `buf = g` while the step count is 1 (the device count under
    sanitize=True, so a skipped first step leaves the next one to initialise),
    `buf = momentum*buf + g` afterwards.

    Checkpoints are torch.optim.SGD's: `momentum_buffer` per parameter and no
    step count. A state_dict with buffers resumes with `buf = momentum*buf + g`
    (steps_taken() then counts from 1); one without them, or with None entries,
    resumes with `buf = g`."""
    _TORCH = torch.optim.SGD
    _REFUSED = {"nesterov": False, "maximize": False, "dampening": 0}

    def __init__(self, params, lr=7e-4, momentum=0.9, weight_decay=1e-4, max_grad_norm=None,
                 world_size=1, sanitize=False, grad_scale=1.0, seed=None, dampening=0,
                 nesterov=False, maximize=False, grad_scaler=None, device_hyper=False):
        self._check_refused(dict(dampening=dampening, nesterov=nesterov, maximize=maximize))
        if momentum < 0:
            raise ValueError(f"FlatSGD: invalid momentum {momentum}")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay),
                         max_grad_norm, world_size, sanitize, grad_scale, seed, grad_scaler,
                         device_hyper)

    def _alloc_state(self):
        mu = self.param_groups[0]["momentum"]
        self.momentum_buffer = torch.zeros_like(self.flat) if mu != 0 else None

    def _moments(self):
        return [] if self.momentum_buffer is None else [self.momentum_buffer]

    def _hyper_keys(self):
        return ("lr", "momentum", "weight_decay")

    def _buf(self, grp):
        if grp["momentum"] != 0 and self.momentum_buffer is None:
            # torch would start the buffer at this step's gradient; the kernels
            # decide "first step" from the step count, which has moved on
            raise ValueError("FlatSGD was built with momentum=0 and holds no momentum buffer; "
                             "build a new FlatSGD to train with momentum")
        return self.momentum_buffer if grp["momentum"] != 0 else None

    def _tail_update(self, g, grp, st):
        name, lr = ("nsm_sgd_tail_dev", ptr(self._hyper_dev)) if self.device_hyper \
            else ("nsm_sgd_tail", float(grp["lr"]))
        call(name, ptr(self.flat), ptr(g), ptr(self._buf(grp)), ptr(self._blk_seg),
             ptr(self._blk_lo), ptr(self._blk_hi), self._nblk, ptr(self._seg_coef),
             ptr(self.flags), ptr(self._step_dev), lr, float(grp["momentum"]),
             float(grp["weight_decay"]), st)

    def _plain_update(self, g, n, grp, coef, st):
        call("nsm_sgd_step", ptr(self.flat), ptr(g), ptr(self._buf(grp)), n, float(grp["lr"]),
             float(grp["momentum"]), float(grp["weight_decay"]), self.step_count, ptr(coef), st)

    def state_dict(self):
        params = self.param_groups[0]["params"]
        # torch keeps a buffer once a step was taken with momentum, else no state
        stepped = self.param_groups[0]["momentum"] != 0 and self.steps_taken() > 0
        state, off = {}, 0
        for i, p in enumerate(params):
            n = p.numel()
            if stepped:
                state[i] = {"momentum_buffer": self.momentum_buffer[off:off + n].view_as(p).clone()}
            off += n
        grp = self._torch_group_defaults()
        grp["params"] = list(range(len(params)))
        return {"state": state, "param_groups": [grp]}

    def load_state_dict(self, sd):
        params = self.param_groups[0]["params"]
        grp = self._load_group(sd, ("lr", "momentum", "weight_decay"))
        bufs = []
        for i in range(len(params)):
            st = sd["state"].get(i, sd["state"].get(grp["params"][i]))
            bufs.append(None if st is None else st.get("momentum_buffer"))
        have = [b is not None for b in bufs]
        if any(have) and not all(have):
            raise ValueError("FlatSGD keeps one first-step state; checkpoint has momentum buffers "
                             "for some parameters only")
        mu = self.param_groups[0]["momentum"]
        if mu != 0 and self.momentum_buffer is None:
            self.momentum_buffer = torch.zeros_like(self.flat)
        if all(have) and mu != 0:
            off = 0
            with torch.no_grad():
                for p, b in zip(params, bufs):
                    n = p.numel()
                    self.momentum_buffer[off:off + n].copy_(b.reshape(-1))
                    off += n
            self._set_steps(1)    # buffers present: the next step is buf = mu*buf + g
        else:
            if self.momentum_buffer is not None:
                self.momentum_buffer.zero_()
            self._set_steps(0)    # the next step taken initialises buf = g


def make_optimizer(params, optimizer_type, lr, **kw):
    """main.py:952-957 in one call: 'adam' -> Adam(weight_decay=1e-4), 'adamw' ->
    AdamW(weight_decay=1e-3), anything else -> SGD(momentum=0.9,
    weight_decay=1e-4), on the flat-buffer optimizers. The comparison is the
    reference's (exact, case-sensitive); `kw` takes max_grad_norm, world_size,
    sanitize, grad_scale, seed, grad_scaler and device_hyper."""
    if optimizer_type == 'adam':
        return FlatAdam(params, lr=lr, weight_decay=1e-4, **kw)
    elif optimizer_type == 'adamw':
        return FlatAdamW(params, lr=lr, weight_decay=1e-3, **kw)
    else:
        return FlatSGD(params, lr=lr, momentum=0.9, weight_decay=1e-4, **kw)
