"""CPU: the fixed-decision gradient helper of the VGG-gradient tests
(tests/vgg_grad_util.py) checked against float64 autograd, and the refusals of
the `vgg_grad=True` interface (raised before any device work)."""
import pytest
import torch

import vgg_grad_util as U

torch.set_num_threads(8)


@pytest.mark.parametrize("name", ["b1_40x72", "b1_32x48"])
def test_fixed_decision_grad_reproduces_float64_autograd(name):
    """Fed the float64 reference's own activations, the helper takes the
    decisions autograd took: the two gradients differ by float64 rounding."""
    o, _ = U.inputs(name)
    _, ref, acts = U.autograd64(name)
    got = U.fixed_decision_grad(o, acts)
    err = U.rel(got, ref)
    print(f"{name}: fixed-decision vs float64 autograd rel-L2 {err:.2e}")
    assert ref.abs().max() > 0
    assert err <= 1e-12


def test_fixed_decision_grad_is_linear_in_the_upstream_gradient():
    o, _ = U.inputs("b1_32x48")
    _, _, acts = U.autograd64("b1_32x48")
    g1 = U.fixed_decision_grad(o, acts)
    g2 = U.fixed_decision_grad(o, acts, upstream=1024.0)
    assert torch.equal(g2, 1024.0 * g1)


def test_vgg_grad_refusals():
    """vgg_grad=True differentiates the package's own VGG stack: a user
    callable, or no VGG weights, cannot provide the gradient."""
    import nsm_amd
    with pytest.raises(ValueError):
        nsm_amd.CustomLoss(None, 0.9, vgg=lambda o, t: 0.0, vgg_grad=True)
    with pytest.raises(ValueError):
        nsm_amd.CustomLoss(None, 0.9, vgg_weights=False, vgg_grad=True)
    with pytest.raises(ValueError):
        nsm_amd.EnhancedCustomLoss(None, 0.9, vgg=lambda o, t: 0.0, vgg_grad=True)
    with pytest.raises(ValueError):
        nsm_amd.EnhancedCustomLoss(None, 0.9, vgg_weights=False, vgg_grad=True)
