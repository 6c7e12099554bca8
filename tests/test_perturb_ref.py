"""CPU: the fp64 restatement of the fused perturbation loss (tests/perturb_util.py)
pinned to the oracle on the reference's own fixture, the new C entries declared,
exported and bound, and the host-side refusals of the perturbation options."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import perturb_util as PU
from oracle import unet_ref as O
from oracle.weights import make_state
from util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nsm.h")
LIB = os.path.join(ROOT, "pcss-unet_amd", "nsm_amd", "libnsm.so")
ENTRIES = ("nsm_perturb_variants", "nsm_pert_loss_blocks", "nsm_pert_loss_fwd",
           "nsm_pert_loss_bwd")

torch.set_num_threads(8)


@pytest.fixture(scope="module")
def fixture_outputs():
    """The fixture's output, the oracle's three perturbed outputs and a target."""
    fx = load("perturb_c4_b1_64")
    sd = O.torch_state(make_state(4, int(fx["meta/seed_w"])))
    for k in list(sd):
        if "run_before/" + k in fx and "running" in k:
            sd[k] = torch.from_numpy(fx["run_before/" + k].copy())
    x = torch.from_numpy(fx["x"])
    ps = O.perturb_inputs(x, [torch.from_numpy(n) for n in fx["noise"]])
    with torch.no_grad():
        pouts = [O.forward(sd, p, True, None, 0.0)[0] for p in ps]
    out = torch.from_numpy(fx["out"])
    y = torch.rand(out.shape, generator=torch.Generator().manual_seed(4))
    return fx, out, y, pouts


def test_helper_matches_oracle_on_the_fixture(fixture_outputs):
    fx, out, y, pouts = fixture_outputs
    alpha, w, v = 0.9, 0.5, 0.37
    ref = PU.pert_loss_ref(out.numpy(), y.numpy(), [p.numpy() for p in pouts], alpha, w, vgg=v)
    pert = O.perturbation_loss(out, pouts).item()
    assert abs(ref["pert"] - pert) <= 1e-6 * pert
    assert abs(ref["pert"] - float(fx["loss"])) <= 2e-6 * float(fx["loss"])
    total = O.custom_loss(out, y, alpha, vgg=v).item() + w * pert
    assert abs(ref["total"] - total) <= 1e-6 * total
    assert abs(ref["l1"] - (out - y).abs().mean().item()) <= 1e-6 * ref["l1"]
    assert len(ref["means"]) == 3


def test_helper_gradient_matches_the_fixture(fixture_outputs):
    fx, out, y, pouts = fixture_outputs
    po = [p.numpy() for p in pouts]
    # the perturbation part alone (alpha = 0, w = 1) is the fixture's out_grad
    g = PU.pert_grad_ref(out.numpy(), y.numpy(), po, 0.0, 1.0).reshape(fx["out_grad"].shape)
    tie = np.zeros(out.numpy().shape, dtype=bool)
    for p in po:
        tie |= out.numpy() == p
    assert tie.mean() < 0.5
    assert np.abs(g - fx["out_grad"])[~tie].max() <= 1e-10
    # and the whole gradient adds alpha*sign(o - t)/n (customLoss.py:90,160)
    full = PU.pert_grad_ref(out.numpy(), y.numpy(), po, 0.9, 0.5)
    want = (0.9 * np.sign(out.numpy() - y.numpy()) / out.numel() + 0.5 * fx["out_grad"]).ravel()
    assert np.abs(full - want)[~tie.ravel()].max() <= 1e-10


def test_helper_planted_ties():
    o, t, ps = PU.make_operands(1000, 3)
    assert (ps[0] == o).mean() >= 0.125 and (t == o).mean() >= 0.125
    z = PU.all_tie(1000)
    assert z.sum() > 0
    assert (PU.pert_grad_ref(o, t, ps, 0.9, 0.5)[z] == 0).all()
    o1, t1, p1 = PU.make_operands(1, 1)
    assert o1[0] != t1[0] and o1[0] != p1[0][0]


def test_perturb_entries_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(LIB)
    import nsm_amd._lib as L
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} not declared in include/nsm.h"
        assert hasattr(lib, name), f"{name} not exported by libnsm.so"
        assert name in L.symbols(), f"{name} not bound in _lib.py"
    assert re.search(r"#define\s+NSM_PERT_MAX\s+8\b", txt)
    from nsm_amd import losses
    assert losses.PERT_MAX == 8


def test_perturb_entries_validate_before_any_launch():
    import nsm_amd._lib as L
    one = ctypes.c_void_p(16)   # never dereferenced: the checks come first
    tab = (ctypes.c_void_p * 1)(16)
    assert L.lib.nsm_perturb_variants(None, one, None, 0, None, 3, 1, 1, 1, 1, 0.01, one, None) == 1
    assert L.lib.nsm_perturb_variants(one, one, None, 0, None, 0, 1, 1, 1, 1, 0.01, one, None) == 1
    assert L.lib.nsm_perturb_variants(one, one, None, 0, None, 9, 1, 1, 1, 1, 0.01, one, None) == 1
    assert L.lib.nsm_pert_loss_blocks(0) == 0 and L.lib.nsm_pert_loss_blocks(2 ** 31) == 0
    assert L.lib.nsm_pert_loss_blocks(1) == 1 and L.lib.nsm_pert_loss_blocks(2049) == 2
    assert L.lib.nsm_pert_loss_fwd(one, one, tab, 0, 4, 0.9, 0.5, None, one, one, None) == 1
    assert L.lib.nsm_pert_loss_fwd(one, one, tab, 9, 4, 0.9, 0.5, None, one, one, None) == 1
    assert L.lib.nsm_pert_loss_fwd(one, one, None, 1, 4, 0.9, 0.5, None, one, one, None) == 1
    assert L.lib.nsm_pert_loss_fwd(None, one, tab, 1, 4, 0.9, 0.5, None, one, one, None) == 1
    nul = (ctypes.c_void_p * 1)(None)
    assert L.lib.nsm_pert_loss_fwd(one, one, nul, 1, 4, 0.9, 0.5, None, one, one, None) == 1
    assert L.lib.nsm_pert_loss_bwd(one, one, tab, 0, 4, 0.9, 0.5, None, one, 0, None) == 1
    assert L.lib.nsm_pert_loss_bwd(one, one, tab, 1, 0, 0.9, 0.5, None, one, 0, None) == 1
    assert L.lib.nsm_pert_loss_bwd(one, one, tab, 1, 4, 0.9, 0.5, None, None, 0, None) == 1


def test_option_refusals():
    """ValueError before any GPU work (CPU tensors never reach a kernel)."""
    import nsm_amd
    for bad in ("cuda", "", None, "Device"):
        with pytest.raises(ValueError):
            nsm_amd.PerturbationLoss(noise=bad)
        with pytest.raises(ValueError):
            nsm_amd.EnhancedCustomLoss(None, vgg_weights=False, noise=bad)
    for cls, kw in ((nsm_amd.PerturbationLoss, {}),
                    (nsm_amd.EnhancedCustomLoss, {"vgg_weights": False})):
        with pytest.raises(ValueError):
            cls(perturbation_count=0, **kw)
        with pytest.raises(ValueError):
            cls(perturbation_count=9, noise="device", **kw)
        cls(perturbation_count=9, **kw)          # the per-variant path has no limit
        cls(perturbation_count=8, noise="device", **kw)
    with pytest.raises(ValueError):          # a seed belongs to the device generator
        nsm_amd.PerturbationLoss(seed=3)
    nsm_amd.PerturbationLoss(noise="device", seed=3)
    with pytest.raises(ValueError):
        nsm_amd.EnhancedCustomLoss(None, vgg_weights=False, perturbation_count=9, fused=True)
    nsm_amd.EnhancedCustomLoss(None, vgg_weights=False, perturbation_count=8, fused=True)


@pytest.mark.parametrize("noise", ["torch", "device"])
def test_injected_noise_refusals(noise):
    import nsm_amd
    x = torch.zeros(2, 4, 8, 8)
    pl = nsm_amd.PerturbationLoss(noise=noise)
    for bad in ([torch.zeros(2, 4, 8, 8)] * 2,                       # count
                [torch.zeros(2, 4, 8, 8)] * 2 + [torch.zeros(2, 4, 8, 4)],   # one shape
                torch.zeros(2, 2, 4, 8, 8),                          # stacked: count
                torch.zeros(3, 2, 4, 8, 9)):                         # stacked: shape
        with pytest.raises(ValueError):
            pl.perturb_input(x, bad)
    crit = nsm_amd.EnhancedCustomLoss(None, vgg_weights=False, fused=True, noise=noise)
    with pytest.raises(ValueError):
        crit.set_noises([torch.zeros(2, 4, 8, 8)] * 2)
    crit.set_noises(torch.zeros(3, 2, 4, 8, 8))
    with pytest.raises(ValueError):          # set for another input shape
        crit(None, torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8), torch.zeros(2, 4, 8, 4))
    crit.set_noises(None)
