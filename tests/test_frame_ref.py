"""CPU: the oracle of the inference-frame-path tests (frame_util) satisfies the
identities the issue states, and the C ABI of the frame path validates its
arguments before any GPU work."""
import numpy as np
import pytest
import torch

import frame_util as U
import nsm_amd._lib as L


@pytest.mark.parametrize("shape", U.PREP_SHAPES)
def test_pad_equals_the_index_formula(shape):
    """ReflectionPad2d((0, pad_w, 0, pad_h)) is out[y, x] = in[ry, rx] with
    r = i < n ? i : 2 (n - 1) - i."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, generator=g)
    ref = U.prep_ref(x, scrub_on=False)
    Hp, Wp = U.padded(shape[2]), U.padded(shape[3])
    assert ref.shape == shape[:2] + (Hp, Wp)
    assert torch.equal(ref, U.pad_by_index(x, Hp, Wp))
    assert torch.equal(ref[..., :shape[2], :shape[3]], x)


def test_pad_multiple_none_and_one_keep_the_size():
    x = U.prep_input((1, 2, 17, 19))
    for m in (None, 1):
        assert U.prep_ref(x, pad_multiple=m, scrub_on=False).shape == x.shape


def test_scrub_leaves_finite_values_alone():
    keep = torch.tensor([-0.0, U.DENORMAL, -U.DENORMAL, U.FLT_MAX, -U.FLT_MAX, 0.0, 1.5])
    assert keep[1] != 0 and keep[1] < np.finfo(np.float32).tiny
    out = U.scrub(keep)
    assert torch.equal(out.view(torch.int32), keep.view(torch.int32))   # bits: -0.0 stays -0.0
    bad = U.scrub(torch.tensor([float("nan"), float("inf"), float("-inf")]))
    assert bad.tolist() == [0.0, 1.0, 0.0]


def test_padded_copy_of_a_nan_is_scrubbed():
    x = U.prep_input((1, 4, 17, 19))
    assert not torch.isfinite(x).all()
    raw = U.prep_ref(x, scrub_on=False)
    assert not torch.isfinite(raw[..., 17:, :]).all() and not torch.isfinite(raw[..., :, 19:]).all()
    assert torch.isfinite(U.prep_ref(x)).all()


def test_8bit_conversion_is_the_fp32_floor():
    """(v * 255).astype(np.uint8) on clipped values is floor(fl32(v * 255))."""
    v = U.finish_values().view(1, 1, 1, -1)
    u8, f32 = U.finish_ref(v)
    assert u8.dtype == torch.uint8 and f32.dtype == torch.float32
    prod = f32.numpy().astype(np.float32) * np.float32(255)
    assert prod.dtype == np.float32
    assert np.array_equal(u8.numpy().reshape(-1), np.floor(prod).astype(np.int64).reshape(-1))
    assert 0 <= f32.min() and f32.max() <= 1 and int(u8.max()) == 255 and int(u8.min()) == 0
    # the neighbours matter: the value just below k/255 may land on k - 1
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    below = np.nextafter(k, np.float32(-np.inf))
    got = U.finish_ref(torch.from_numpy(below).view(1, 1, 1, -1))[0].numpy().reshape(-1)
    assert (got[1:] <= np.arange(1, 256)).all() and (got[1:] < np.arange(1, 256)).any()


def test_finish_layout_and_census():
    o = U.finish_input(3, 32, 32, (17, 19))
    u8, f32 = U.finish_ref(o, (17, 19))
    assert u8.shape == (o.shape[0], 17, 19, 3) and f32.shape == (o.shape[0], 3, 17, 19)
    assert torch.equal(u8[:, 5, 7, 2], (f32[:, 2, 5, 7] * 255).to(torch.uint8))
    assert U.finish_ref(U.finish_input(1, 16, 16))[0].dim() == 3
    crop = o[..., :17, :19]
    vals = U.finish_values()
    have = set(crop.reshape(-1).view(torch.int32).tolist())
    assert all(b in have for b in vals.view(torch.int32).tolist())     # every value, by its bits
    cen = U.finish_census(o, (17, 19))
    assert cen[:, 0].sum() == 3 and cen[:, 1].sum() > 0 and cen[:, 2].sum() > 0


def test_frame_blocks_plan():
    n = L.lib.nsm_frame_blocks
    assert n(1, 1, 1) == 1
    assert n(4, 1088, 1920) > n(4, 544, 960) > n(1, 16, 16) >= 1
    assert n(7, 1088, 1920) > n(4, 1088, 1920)
    assert n(1, 17, 19) == n(1, 17, 20)                 # ceil(W / 4) columns of 4
    assert n(0, 8, 8) == 0 and n(1, 0, 8) == 0 and n(1, 8, -1) == 0
    assert n(8, 16384, 16384) == 0                      # 2^31 samples in an image
    assert n(1, 1 << 15, (1 << 16) - 1) > 0             # just below


P1 = 4096    # a non-null pointer that is never dereferenced: the checks come first

BAD_PREP = [
    ("null x", "null", (None, 1, 4, 16, 16, 16, 16, None, None, 1e-8, 1, P1, None, None, None)),
    ("null out", "null", (P1, 1, 4, 16, 16, 16, 16, None, None, 1e-8, 1, None, None, None, None)),
    ("mean without stdv", "null", (P1, 1, 4, 16, 16, 16, 16, P1, None, 1e-8, 1, P1, None, None,
                                   None)),
    ("partial without report", "null", (P1, 1, 4, 16, 16, 16, 16, None, None, 1e-8, 1, P1, P1,
                                        None, None)),
    ("pad >= height", "height", (P1, 1, 4, 2, 33, 16, 48, None, None, 1e-8, 1, P1, None, None,
                                 None)),
    ("pad >= width", "width", (P1, 1, 4, 33, 2, 48, 16, None, None, 1e-8, 1, P1, None, None, None)),
    ("shrinking", "smaller", (P1, 1, 4, 16, 16, 8, 16, None, None, 1e-8, 1, P1, None, None, None)),
    ("2^31 samples", "2^31", (P1, 1, 8, 16384, 16384, 16384, 16384, None, None, 1e-8, 1, P1, None,
                              None, None)),
    ("empty", "shape", (P1, 0, 4, 16, 16, 16, 16, None, None, 1e-8, 1, P1, None, None, None)),
]

BAD_FINISH = [
    ("null o", "null", (None, 1, 1, 16, 16, 16, 16, P1, None, None, None, None)),
    ("no output", "null", (P1, 1, 1, 16, 16, 16, 16, None, None, None, None, None)),
    ("report without partial", "null", (P1, 1, 1, 16, 16, 16, 16, P1, None, None, P1, None)),
    ("2 channels", "channels", (P1, 1, 2, 16, 16, 16, 16, P1, None, None, None, None)),
    ("7 channels", "channels", (P1, 1, 7, 16, 16, 16, 16, P1, None, None, None, None)),
    ("crop height", "larger", (P1, 1, 1, 16, 16, 17, 16, P1, None, None, None, None)),
    ("crop width", "larger", (P1, 1, 1, 16, 16, 16, 17, P1, None, None, None, None)),
    ("2^31 samples", "2^31", (P1, 1, 4, 32768, 16384, 16, 16, P1, None, None, None, None)),
]


@pytest.mark.parametrize("name,word,args", BAD_PREP, ids=[c[0] for c in BAD_PREP])
def test_prep_error_paths_without_gpu_work(name, word, args):
    """Return code 1 (NSM_E_ARG) and a readable message; none of these reaches
    a launch (no GPU is needed to run them)."""
    assert L.lib.nsm_frame_prep(*args) == 1
    msg = L.last_error()
    assert "frame_prep" in msg and word in msg, msg


@pytest.mark.parametrize("name,word,args", BAD_FINISH, ids=[c[0] for c in BAD_FINISH])
def test_finish_error_paths_without_gpu_work(name, word, args):
    assert L.lib.nsm_frame_finish(*args) == 1
    msg = L.last_error()
    assert "frame_finish" in msg and word in msg, msg


def test_python_checks_need_no_gpu():
    """The host-side checks of the public functions come before any GPU work,
    so a CPU tensor and a bad pad raise ValueError on any machine."""
    import nsm_amd
    from nsm_amd.frames import padded_size
    with pytest.raises(ValueError, match="GPU"):
        nsm_amd.prepare_frames(torch.zeros(1, 4, 16, 16))
    with pytest.raises(ValueError, match="GPU"):
        nsm_amd.finish_frames(torch.zeros(1, 1, 16, 16))
    with pytest.raises(ValueError, match="height"):
        padded_size(2, 33, 16)
    with pytest.raises(ValueError, match="width"):
        padded_size(33, 2, 16)
    with pytest.raises(ValueError, match="pad_multiple"):
        padded_size(16, 16, 0)
    assert padded_size(1080, 1920) == (1088, 1920) and padded_size(17, 19, None) == (17, 19)
    assert padded_size(17, 19, 1) == (17, 19)
