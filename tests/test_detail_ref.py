"""CPU: the comparator of the detail-term tests (detail_util.py) is sound in
the reference's own precision, its near-tie exclusions stay rare, and the
library exports the detail-term entry points."""
import pytest
import torch

import detail_util as U

torch.set_num_threads(16)


@pytest.mark.parametrize("shape", U.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float32_reference_agrees_with_float64(shape):
    """The reference's arithmetic (float32) against the float64 comparator, at
    the bounds the GPU kernels are held to."""
    o, t, vals, grads, ties = U.reference(shape)
    v32, g32 = U.evaluate(o, t, torch.float32)
    for k in U.TERMS:
        err = abs(v32[k] - vals[k]) / abs(vals[k])
        rel, worst, share = U.grad_errors(g32[k], grads[k], ties[k])
        print(f"{shape} {k}: value rel {err:.2e} grad rel-L2 {rel:.2e} pixel {worst:.2e} "
              f"excluded {share:.2e}")
        assert vals[k] > 0
        assert err <= U.VALUE_REL
        assert rel <= U.GRAD_REL_L2 and worst <= U.GRAD_PIXEL


@pytest.mark.parametrize("shape", U.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_near_tie_share_is_capped(shape):
    _, _, _, grads, ties = U.reference(shape)
    for k in U.TERMS:
        assert ties[k].shape == grads[k].shape
        assert ties[k].double().mean().item() <= U.TIE_SHARE, k


def test_formulas_match_hand_written_gradients():
    """The issue's closed-form gradients against autograd, in float64."""
    import torch.nn.functional as F
    o32, t32, _, grads, _ = U.reference((2, 1, 40, 72))
    o, t = o32.double(), t32.double()
    n = o.numel()
    G = U.gaussian(torch.float64)
    s = torch.sign(U.high_freq(o) - U.high_freq(t))
    hf = (s - F.conv2d(s, G.flip(2, 3), padding=2)) / n
    torch.testing.assert_close(hf, grads["hf"], rtol=1e-12, atol=1e-18)
    m = U.penumbra_mask(t32).double()
    pen = m * torch.sign(o - t) / (m.sum() + 1e-8)
    torch.testing.assert_close(pen, grads["pen"], rtol=1e-12, atol=1e-18)
    kx, ky = U.sobel_kernels(torch.float64)
    gx, gy = F.conv2d(o, kx, padding=1), F.conv2d(o, ky, padding=1)
    mo = torch.sqrt(gx ** 2 + gy ** 2 + 1e-6)
    u = torch.sign(mo - U.sobel_mag(t))
    sob = (F.conv2d(u * gx / mo, kx.flip(2, 3), padding=1)
           + F.conv2d(u * gy / mo, ky.flip(2, 3), padding=1)) / n
    torch.testing.assert_close(sob, grads["sob"], rtol=1e-10, atol=1e-16)


def test_library_binds_the_detail_entries():
    import nsm_amd
    import nsm_amd._lib as L
    for name in ("nsm_detail_blocks", "nsm_detail_loss_fwd", "nsm_detail_loss_bwd"):
        assert name in L.symbols()
    # 16 x 64 tiles of one image each
    assert L.lib.nsm_detail_blocks(2, 17, 65) == 2 * 2 * 2
    assert L.lib.nsm_detail_blocks(3, 33, 65) == 3 * 3 * 2
    assert L.lib.nsm_detail_blocks(0, 4, 4) == 0
    # argument validation fails before any launch
    assert L.lib.nsm_detail_loss_fwd(None, None, 1, 4, 4, 0.0, 0.0, 0.0, None, None, None, None) == 1
    assert "null" in L.last_error()
    assert callable(nsm_amd.detail_terms) and callable(nsm_amd.detail_loss)
