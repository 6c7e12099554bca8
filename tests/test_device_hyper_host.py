"""CPU: the host side of the device hyper block (include/nsm.h, nsm_hyper_set):
its size, and the argument validation, which fails before any launch with a
readable message (the pattern of test_capi.test_error_path_without_gpu_work).
The values are checked before the pointer, so a NULL block with valid values
fails on the pointer alone: that is how `max_norm = +inf` is shown to pass the
validation on a machine with no GPU to launch on."""
import math

import pytest

# never dereferenced: every call that passes it fails its value check first
FAKE_BLOCK = 0x1000


def test_hyper_block_is_16_bytes():
    import nsm_amd._lib as L
    assert L.lib.nsm_hyper_bytes() == 16


def test_null_block_is_refused():
    import nsm_amd._lib as L
    assert L.lib.nsm_hyper_set(None, 1e-3, 1.0, None) == 1
    assert "null hyper block" in L.last_error()


@pytest.mark.parametrize("lr", [math.nan, -1e-3, math.inf, -math.inf])
def test_bad_lr_is_refused(lr):
    import nsm_amd._lib as L
    assert L.lib.nsm_hyper_set(FAKE_BLOCK, lr, 1.0, None) == 1
    assert "lr must be finite and >= 0" in L.last_error()


@pytest.mark.parametrize("max_norm", [math.nan, -0.5, -math.inf])
def test_bad_max_norm_is_refused(max_norm):
    import nsm_amd._lib as L
    assert L.lib.nsm_hyper_set(FAKE_BLOCK, 1e-3, max_norm, None) == 1
    assert "max_norm must be >= 0 or +inf" in L.last_error()


@pytest.mark.parametrize("lr,max_norm", [(1e-3, math.inf), (0.0, 0.0), (1e-3, 1.0)])
def test_valid_values_pass_the_value_checks(lr, max_norm):
    """+inf (no clipping), lr = 0 and max_norm = 0 are values the kernels take:
    with a NULL block the only complaint left is the pointer."""
    import nsm_amd._lib as L
    assert L.lib.nsm_hyper_set(None, lr, max_norm, None) == 1
    err = L.last_error()
    assert "null hyper block" in err and "must" not in err


def test_dev_entries_refuse_a_null_block():
    """The *_dev tail entries check the block pointer before any launch."""
    import nsm_amd._lib as L
    p = FAKE_BLOCK
    assert L.lib.nsm_adamw_tail_dev(p, p, p, p, p, p, p, 1, p, p, p, None, 0.9, 0.999, 1e-8, 1e-3,
                                    None) == 1
    assert "null hyper block" in L.last_error()
    assert L.lib.nsm_adam_tail_dev(p, p, p, p, p, p, p, 1, p, p, p, None, 0.9, 0.999, 1e-8, 1e-4,
                                   None) == 1
    assert "null hyper block" in L.last_error()
    assert L.lib.nsm_sgd_tail_dev(p, p, p, p, p, p, 1, p, p, p, None, 0.9, 1e-4, None) == 1
    assert "null hyper block" in L.last_error()
    assert L.lib.nsm_grad_tail_dev(p, 1, p, p, p, p, p, 1, 1.0, 1.0, None, None, 0, p, 1 << 20, p,
                                   p, p, p, None) == 1
    assert "null hyper block" in L.last_error()
    assert L.lib.nsm_grad_tail_scaled_dev(p, 1, p, p, p, p, p, 1, 1.0, p, None, None, 0, p,
                                          1 << 20, p, p, p, p, 2.0, 0.5, 100, 1, None) == 1
    assert "null hyper block" in L.last_error()
