"""torch.amp.GradScaler's update rule (torch._amp_update_scale_) in plain Python,
on fp32 values: the reference the device scaler's trajectory is replayed with."""
import numpy as np


def update(scale, tracker, found_inf, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000,
           other_skip=False):
    """(scale, tracker) after one step. `other_skip`: the step was skipped for a
    reason that is no overflow (the reference `continue`s before update())."""
    if found_inf:
        return float(np.float32(np.float32(scale) * np.float32(backoff_factor))), 0
    if other_skip:
        return scale, tracker
    if tracker + 1 != growth_interval:
        return scale, tracker + 1
    with np.errstate(over="ignore"):
        s2 = np.float32(np.float32(scale) * np.float32(growth_factor))
    return (float(s2) if np.isfinite(s2) else scale), 0
