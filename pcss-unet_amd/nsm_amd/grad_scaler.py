"""Dynamic loss scaling for the fp16 training step, kept on the device.

The reference trains under `torch.amp.autocast(float16)` with a
`torch.amp.GradScaler` (main.py:175, 257-259, 281, 361-368, 421-422).
`nsm_amd.GradScaler` has that surface, but the work is the device tail's:

  * the scale, the growth tracker and three counters live in one device buffer
    of NSM_SCALER_WORDS words (include/nsm.h);
  * the loss backward is seeded from the scale word itself (`scaler.seed`, or
    `scaler.scale(loss)` which multiplies by it), so nothing reads the scale on
    the host and a captured graph follows a moving scale;
  * `nsm_grad_tail_scaled` (an optimizer built with `grad_scaler=`) unscales by
    that word and, in its finalize kernel, applies torch.amp.GradScaler's update
    rule (`torch._amp_update_scale_`) to it. `found_inf` is the tail's own
    census: a NaN or Inf anywhere in the (rank-averaged) scaled gradient, or a
    non-finite norm after the repair.

`on_overflow` says what a step with `found_inf` does: "skip" (torch's
behaviour: no optimizer step) or "repair" (the reference's: the tail repairs
the gradient and steps, main.py:320-354; the scale still backs off).

The reference's loop becomes

    scaler = nsm_amd.GradScaler()
    opt = nsm_amd.make_optimizer(params, 'adamw', lr, sanitize=True, grad_scaler=scaler)
    scaler.scale(loss).backward()
    scaler.step(opt); scaler.update()

`unscale_` has no place in it: the tail unscales (and replaces main.py:287-418).
"""
import torch

from ._lib import call, ptr, stream

SCALER_WORDS = 8            # NSM_SCALER_WORDS
STATE_NAMES = ("scale", "growth_tracker", "found_inf", "overflows", "growths")
_POLICIES = {"repair": 0, "skip": 1}


class GradScaler:
    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5,
                 growth_interval=2000, enabled=True, on_overflow="skip", device=None):
        # what torch.amp.GradScaler refuses
        if growth_factor <= 1.0:
            raise ValueError("The growth factor must be > 1.0.")
        if backoff_factor >= 1.0:
            raise ValueError("The backoff factor must be < 1.0.")
        if backoff_factor <= 0.0:
            raise ValueError("The backoff factor must be > 0.0.")
        if int(growth_interval) < 1:
            raise ValueError("The growth interval must be >= 1.")
        if on_overflow not in _POLICIES:
            raise ValueError(f"on_overflow must be 'skip' or 'repair', got {on_overflow!r}")
        self._enabled = bool(enabled)
        self.growth_factor = float(growth_factor)
        self.backoff_factor = float(backoff_factor)
        self.growth_interval = int(growth_interval)
        self.on_overflow = on_overflow
        self._state = None
        self.seed = None       # disabled: loss.backward(None) is loss.backward()
        if not self._enabled:
            return
        self._check_scale(init_scale)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None \
            else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"GradScaler: the scale lives on a ROCm GPU device (got {dev}); pass "
                             "enabled=False elsewhere, as main.py:175 does")
        self._state = torch.zeros(SCALER_WORDS, dtype=torch.int32, device=dev)
        # 0-dim fp32 view of the scale word: its address never changes
        self.seed = self._state.view(torch.float32)[0]
        self._set(float(init_scale), 0)

    @staticmethod
    def _check_scale(s):
        s = float(s)
        if not (s > 0.0 and s <= 3.4028234663852886e38):
            raise ValueError(f"GradScaler: the scale must be a positive finite fp32, got {s}")

    def _set(self, scale, tracker):
        with torch.cuda.device(self._state.device):
            call("nsm_scaler_set", ptr(self._state), float(scale), int(tracker), stream())

    def is_enabled(self):
        return self._enabled

    # ---- what the tail is called with ----------------------------------------
    def tail_args(self):
        """(growth_factor, backoff_factor, growth_interval, on_overflow) as
        nsm_grad_tail_scaled takes them."""
        return (self.growth_factor, self.backoff_factor, self.growth_interval,
                _POLICIES[self.on_overflow])

    def state_tensor(self):
        """The device state (int32[NSM_SCALER_WORDS]); None when disabled."""
        return self._state

    # ---- torch.amp.GradScaler's surface, as main.py uses it -------------------
    def scale(self, loss):
        """loss * <the device scale>: no host read, correct under capture."""
        if not self._enabled:
            return loss
        return loss * self.seed

    def step(self, optimizer, *args, **kwargs):
        if getattr(optimizer, "grad_scaler", None) is not self:
            raise ValueError("GradScaler.step: the optimizer was not built with this scaler "
                             "(nsm_amd.FlatAdamW(..., sanitize=True, grad_scaler=scaler)); its "
                             "device tail is what unscales and updates the scale")
        return optimizer.step(*args, **kwargs)

    def update(self, new_scale=None):
        """None: nothing to do, the tail of the step already updated the scale.
        A float: set the scale on the device (in place) and zero the tracker."""
        if not self._enabled or new_scale is None:
            return
        if isinstance(new_scale, torch.Tensor):
            new_scale = float(new_scale.item())
        self._check_scale(new_scale)
        self._set(new_scale, 0)

    def unscale_(self, optimizer=None):
        raise RuntimeError("nsm_amd.GradScaler.unscale_: the optimizer's device tail "
                           "(nsm_grad_tail_scaled) unscales the gradient, with the sanitising and "
                           "clipping of main.py:287-418 — drop that block and call "
                           "scaler.step(optimizer)")

    def get_scale(self):
        """The scale as a host float (synchronises, like torch's)."""
        if not self._enabled:
            return 1.0
        return float(self.seed.item())

    def last(self):
        """{scale, growth_tracker, found_inf, overflows, growths} of the device
        state (synchronises: for logs and tests)."""
        if not self._enabled:
            return dict(zip(STATE_NAMES, (1.0, 0, 0, 0, 0)))
        w = self._state.cpu()
        d = dict(zip(STATE_NAMES, [0.0] + w[1:5].tolist()))
        d["scale"] = float(w.view(torch.float32)[0].item())
        return d

    def get_growth_factor(self):
        return self.growth_factor

    def get_backoff_factor(self):
        return self.backoff_factor

    def get_growth_interval(self):
        return self.growth_interval

    # ---- torch.amp.GradScaler's checkpoint format ------------------------------
    def state_dict(self):
        if not self._enabled:
            return {}
        d = self.last()
        return {"scale": d["scale"], "growth_factor": self.growth_factor,
                "backoff_factor": self.backoff_factor, "growth_interval": self.growth_interval,
                "_growth_tracker": d["growth_tracker"]}

    def load_state_dict(self, state_dict):
        if not self._enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved "
                               "from a disabled instance of GradScaler.")
        gf, bf = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        gi = int(state_dict["growth_interval"])
        if gf <= 1.0 or not 0.0 < bf < 1.0 or gi < 1:
            raise ValueError("GradScaler.load_state_dict: invalid growth/backoff settings")
        self._check_scale(state_dict["scale"])
        self.growth_factor, self.backoff_factor, self.growth_interval = gf, bf, gi
        self._set(float(state_dict["scale"]), int(state_dict["_growth_tracker"]))
