"""CPU: the comparator of the feature-sensitivity tests (sensitivity_util.py: the
paper's Eq. 1 in float64) is sound on a case with a closed form, the end-to-end
configuration separates its channels far beyond the bound the GPU test applies,
and the public entry points validate their arguments before any GPU work."""
import pytest
import torch

import nsm_amd
import sensitivity_util as U
from util import OUT_ABS

torch.set_num_threads(16)


def test_linear_phi_closed_form():
    """phi(x) = sum_c w_c x_c per pixel: d = w_i * eps_i, so S_i = |w_i| mean|z_i|.
    x on a 2^-8 grid, z on a 2^-6 grid and s_i = 2^-1 make x + z * s exact in
    float32, so the identity holds to float64 rounding."""
    gen = torch.Generator().manual_seed(3)
    B, C, H, W, R = 2, 5, 6, 9, 3
    x = torch.randint(-512, 513, (B, C, H, W), generator=gen).float() / 256
    z = torch.randint(-256, 257, (C, R, B, H, W), generator=gen).float() / 64
    w = torch.tensor([1.5, -0.25, 0.0625, -3.0, 0.5], dtype=torch.float64)

    def phi(t):
        return (t * w.view(1, C, 1, 1)).sum(1)

    absolute, signed, relative, terms = U.sensitivity_ref(phi, x, 1.0, z, 0.5)
    want = w.abs() * z.double().abs().mean((1, 2, 3, 4))
    assert (absolute - want).abs().max() <= 1e-12 * want.max()
    want_signed = w * z.double().mean((1, 2, 3, 4))
    assert (signed - want_signed).abs().max() <= 1e-12 * want.max()
    assert abs(relative.sum().item() - 1) <= 1e-15
    assert tuple(terms.shape) == (C, R, B, 2)
    # a subset, in the given order, with per-channel sigma
    sub = [3, 0]
    sig = torch.tensor([2.0, 1.0, 1.0, 4.0, 1.0])
    a2, _, r2, _ = U.sensitivity_ref(phi, x, sig, z[sub], 0.5, sub)
    assert (a2 - want[sub]).abs().max() <= 1e-12 * want.max()
    assert abs(r2.sum().item() - 1) <= 1e-15


def test_e2e_reference_separates_channels():
    """Every S_i of the end-to-end case is at least 20 times the bound the GPU
    test allows, so that bound cannot pass a wrong channel or a lost variant."""
    _, sigma, _, (absolute, signed, relative, _) = U.e2e_case()
    bound = 2 * OUT_ABS / (U.E2E_FACTOR * sigma.double())
    print("S_ref", absolute.tolist(), "ratio", (absolute / bound).tolist(),
          "relative", relative.tolist(), "signed", signed.tolist())
    assert (absolute >= 20 * bound).all()
    assert (absolute[:-1] > absolute[1:]).all()       # ordered by the gains


def _bad_calls():
    x = torch.zeros(2, 4, 8, 8)
    ok = dict(sigma=1.0, repeats=2, factor=0.1, channels=None, chunk=4, noises=None)
    bad = [
        ("sigma-length", dict(sigma=[1.0, 1.0, 1.0])),
        ("sigma-tensor-length", dict(sigma=torch.ones(5))),
        ("sigma-word", dict(sigma="dataset")),
        ("repeats", dict(repeats=0)),
        ("factor-zero", dict(factor=0.0)),
        ("factor-negative", dict(factor=-0.1)),
        ("channel-range", dict(channels=[0, 4])),
        ("channel-negative", dict(channels=[-1])),
        ("channel-repeated", dict(channels=[1, 2, 1])),
        ("noises-shape", dict(noises=torch.zeros(4, 2, 2, 8, 7))),
        ("noises-subset-shape", dict(channels=[1, 2], noises=torch.zeros(4, 2, 2, 8, 8))),
        ("chunk", dict(chunk=0)),
    ]
    return x, ok, bad


@pytest.mark.parametrize("idx", range(12), ids=[b[0] for b in _bad_calls()[2]])
def test_argument_errors_raise_before_gpu_work(idx):
    """The inputs are CPU tensors: a ValueError (not the library's no-GPU error)
    shows that the check came first."""
    x, ok, bad = _bad_calls()
    kw = {**ok, **bad[idx][1]}
    sigma = kw.pop("sigma")
    with pytest.raises(ValueError):
        nsm_amd.feature_sensitivity(None, x, sigma, **kw)
    noises = kw.pop("noises")
    with pytest.raises(ValueError):
        acc = nsm_amd.FeatureSensitivity(None, sigma, **kw)
        acc.update(x, noises=noises)


def test_valid_arguments_reach_the_gpu_requirement():
    x, ok, _ = _bad_calls()
    kw = dict(ok)
    with pytest.raises(nsm_amd.NsmError):
        nsm_amd.feature_sensitivity(None, x, kw.pop("sigma"), **kw)
    with pytest.raises(ValueError):
        nsm_amd.feature_sensitivity(None, x[0], 1.0)


def test_module_has_no_host_synchronisation():
    """Reading the result is the caller's: the module itself never moves a
    value to the host."""
    import inspect

    import nsm_amd.sensitivity as S
    src = inspect.getsource(S)
    for word in (".item(", ".cpu(", ".tolist(", "synchronize", ".numpy("):
        assert word not in src, word
