"""CPU: the dynamic loss scaler's C entries are declared, exported and bound, and
the pure-Python restatement of the update rule (tests/loss_scale_util.py) that
the GPU tests replay equals torch._amp_update_scale_ on CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

import loss_scale_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nsm.h")
LIB = os.path.join(ROOT, "pcss-unet_amd", "nsm_amd", "libnsm.so")
ENTRIES = ("nsm_grad_tail_scaled", "nsm_scaler_set")


def test_scaler_entries_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(LIB)
    import nsm_amd._lib as L
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} not declared in include/nsm.h"
        assert hasattr(lib, name), f"{name} not exported by libnsm.so"
        assert name in L.symbols(), f"{name} not bound in _lib.py"
    assert re.search(r"#define\s+NSM_SCALER_WORDS\s+8\b", txt)
    # nsm_grad_tail's arguments with `float scale` -> `void* scaler_state`, plus
    # growth_factor, backoff_factor, growth_interval, on_overflow before the stream
    static, scaled = L._SIGS["nsm_grad_tail"][1], L._SIGS["nsm_grad_tail_scaled"][1]
    want = list(static[:-1]) + [L.F, L.F, L.I, L.I, L.P]
    want[9] = L.P
    assert list(scaled) == want


def test_scaler_entries_validate_before_any_launch():
    import nsm_amd._lib as L
    assert L.lib.nsm_scaler_set(None, 1.0, 0, None) == 1
    assert L.lib.nsm_grad_tail_scaled(None, 0, None, None, None, None, None, 0, 1.0, None, 1.0,
                                      None, 0, None, 0, None, None, None, None, 2.0, 0.5, 1, 1,
                                      None) == 1
    assert "scaler" in L.last_error()


def test_grad_scaler_refuses_what_torch_refuses():
    import nsm_amd
    for kw in (dict(growth_factor=1.0), dict(growth_factor=0.5), dict(backoff_factor=1.0),
               dict(backoff_factor=2.0)):
        with pytest.raises(Exception):
            torch.amp.GradScaler("cpu", **kw)
        with pytest.raises(ValueError):
            nsm_amd.GradScaler(enabled=False, **kw)
    with pytest.raises(ValueError):
        nsm_amd.GradScaler(enabled=False, on_overflow="ignore")


def test_disabled_grad_scaler_is_a_pass_through():
    import nsm_amd
    sc = nsm_amd.GradScaler(enabled=False)
    loss = torch.tensor(3.0, requires_grad=True)
    assert sc.scale(loss) is loss
    assert sc.seed is None and sc.get_scale() == 1.0 and sc.state_dict() == {}
    sc.update()
    sc.update(4.0)
    assert sc.last() == dict(scale=1.0, growth_tracker=0, found_inf=0, overflows=0, growths=0)


def _torch_update(scale, tracker, found_inf, gf, bf, gi):
    s = torch.tensor([scale], dtype=torch.float32)
    t = torch.tensor([tracker], dtype=torch.int32)
    torch._amp_update_scale_(s, t, torch.tensor([float(found_inf)]), gf, bf, gi)
    return float(s.item()), int(t.item())


# (found_inf sequence, init scale, growth, backoff, interval): backoff, growth at
# the interval, the tracker reset by an overflow one step short of a growth, the
# non-finite growth guard (at interval 1 and after counting up to the interval)
SCRIPTS = [
    ([0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0], 65536.0, 2.0, 0.5, 3),
    ([0, 0, 1, 0, 0, 0], 1024.0, 4.0, 0.25, 3),
    ([0, 0, 0, 1, 0], 2.0 ** 127, 2.0, 0.5, 1),
    ([0, 0, 0, 0], 3e38, 2.0, 0.5, 2),
    ([1] * 6 + [0] * 6, 2.0 ** -120, 1.5, 0.5, 2),
]


@pytest.mark.parametrize("script", SCRIPTS)
def test_helper_equals_torch_update_rule(script):
    seq, scale, gf, bf, gi = script
    s_h = s_t = float(torch.tensor(scale, dtype=torch.float32).item())
    t_h = t_t = 0
    for k, f in enumerate(seq):
        s_h, t_h = U.update(s_h, t_h, f, gf, bf, gi)
        s_t, t_t = _torch_update(s_t, t_t, f, gf, bf, gi)
        assert (s_h, t_h) == (s_t, t_t), (k, f)


def test_helper_fixed_points():
    assert _torch_update(65536.0, 5, 1, 2.0, 0.5, 2000) == (32768.0, 0)
    assert U.update(65536.0, 5, 1) == (32768.0, 0)
    s38 = float(torch.tensor(3e38, dtype=torch.float32).item())
    assert _torch_update(s38, 0, 0, 2.0, 0.5, 1) == (s38, 0)       # not doubled
    assert U.update(s38, 0, 0, 2.0, 0.5, 1) == (s38, 0)
    # a skip that is no overflow moves nothing
    assert U.update(1024.0, 2, 0, 2.0, 0.5, 3, other_skip=True) == (1024.0, 2)
