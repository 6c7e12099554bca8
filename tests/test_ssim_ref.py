"""CPU: the comparator of the SSIM tests (ssim_util.py: pytorch_msssim.ssim
restated from its published algorithm) is sound, and the library exports the
SSIM entry points.

No fixture comes from running the reference: customLoss.py:187-191 is commented
out there (the term never executes) and pytorch_msssim is not installed."""
import pytest
import torch

import ssim_util as U

torch.set_num_threads(16)

CASES = [(s, f) for f in U.FAMILIES for s in U.SHAPES]
IDS = [f"{f}-" + "x".join(map(str, s)) for s, f in CASES]

# the float32 restatement against float64, as measured for the issue, times 2:
# gradient rel-L2, worst pixel / max|g|, value (absolute)
F32_BOUNDS = {"random": (1e-6, 1.6e-6, 4e-7), "smooth": (2.2e-4, 4.6e-4, 1.1e-5)}


@pytest.mark.parametrize("shape,family", CASES, ids=IDS)
def test_closed_form_gradient_matches_autograd(shape, family):
    o, t, (_, _, grad), _ = U.reference(shape, family)
    cf = U.closed_form_grad(o, t)
    err = ((cf - grad).norm() / grad.norm()).item()
    print(f"{family} {shape}: closed form vs autograd rel-L2 {err:.2e}")
    assert grad.abs().max() > 0
    assert err <= 1e-12


@pytest.mark.parametrize("shape,family", CASES, ids=IDS)
def test_float32_restatement_agrees_with_float64(shape, family):
    rel, worst, val, per = U.f32_errors(shape, family)
    print(f"{family} {shape}: grad rel-L2 {rel:.2e} pixel {worst:.2e} value {val:.2e} "
          f"per-image {per:.2e}")
    b = F32_BOUNDS[family]
    assert rel <= b[0] and worst <= b[1] and val <= b[2]


def test_input_families():
    """random: the SSIM maps go negative; smooth: near 1, every image distinct."""
    o, t = U.inputs((3, 1, 27, 75), "random")
    assert U.ssim_map(o.double(), t.double()).min() < 0
    o, t = U.inputs((3, 1, 27, 75), "smooth")
    per = U.ssim_per_image(o.double(), t.double())
    assert per.min() > 0.5 and len(set(per.tolist())) == 3
    assert not torch.equal(t[0], t[1]) and o.min() >= 0 and o.max() <= 1
    # data_range 255 on [0, 1] images: the term is almost constant
    assert 1 - U.ssim_per_image(o.double(), t.double(), 255.0).mean() < 1e-4


def test_library_binds_the_ssim_entries():
    import nsm_amd
    import nsm_amd._lib as L
    for name in ("nsm_ssim_blocks", "nsm_ssim_fwd", "nsm_ssim_bwd"):
        assert name in L.symbols()
    # 16 x 64 tiles of WINDOWS of one image each
    assert L.lib.nsm_ssim_blocks(2, 11, 11) == 2
    assert L.lib.nsm_ssim_blocks(2, 11, 75) == 2 * 1 * 2
    assert L.lib.nsm_ssim_blocks(3, 27, 75) == 3 * 2 * 2
    assert L.lib.nsm_ssim_blocks(3, 26, 74) == 3
    assert L.lib.nsm_ssim_blocks(2, 40, 90) == 2 * 2 * 2
    assert L.lib.nsm_ssim_blocks(1, 10, 64) == 0
    assert L.lib.nsm_ssim_blocks(1, 64, 10) == 0
    assert L.lib.nsm_ssim_blocks(0, 64, 64) == 0
    # argument validation fails before any launch
    assert L.lib.nsm_ssim_fwd(None, None, 1, 16, 16, 1.0, 0.0, None, None, None, None, None) == 1
    assert "null" in L.last_error()
    assert L.lib.nsm_ssim_bwd(None, None, None, 1, 16, 16, 1.0, None, None, 0, None) == 1
    assert "null" in L.last_error()
    assert callable(nsm_amd.ssim) and callable(nsm_amd.ssim_loss)


def test_custom_loss_takes_the_ssim_arguments():
    import nsm_amd
    crit = nsm_amd.CustomLoss(None, 0.9, vgg_weights=False, ssim_weight=0.1)
    assert crit.ssim_weight == 0.1 and crit.ssim_data_range == 1.0
    assert nsm_amd.CustomLoss(None, 0.9, vgg_weights=False).ssim_weight == 0.0
    enh = nsm_amd.EnhancedCustomLoss(None, 0.9, vgg_weights=False, ssim_weight=0.1,
                                     ssim_data_range=255.0)
    assert enh.ssim_weight == 0.1 and enh.base.ssim_data_range == 255.0
    with pytest.raises(nsm_amd.NsmError):
        nsm_amd.ssim(torch.rand(1, 1, 16, 16), torch.rand(1, 1, 16, 16))
