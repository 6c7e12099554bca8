"""The paper's feature-sensitivity analysis (§3.2, Eq. 1) stated in float64 on
the CPU for any callable phi and injected normals: the comparator of
test_sensitivity_ref.py and test_gpu_sensitivity.py.

    S_i = E[ |phi(f_i + eps_i) - phi(f_i)| ] / s_i,   eps_i = z_i * s_i on
    channel i only,  s_i = factor * sigma_i,   relative_i = S_i / sum_j S_j

The perturbed input is formed as the library forms it, in float32
(`x[:, i] + z * s`, s_i rounded once to float32); phi and every sum run in
float64. The expectation is over the R repeats, the B images and the output
elements of an image."""
import functools

import numpy as np
import torch

from oracle import unet_ref as O
from oracle.weights import make_state, synthetic_batch

GAINS = (2.0, 1.0, 0.5, 0.25)


def sensitivity_ref(phi, x, sigma, noises, factor, channels=None):
    """(absolute [C'], signed [C'], relative [C'], terms [C',R,B,2]) in float64.
    phi maps a float64 [B,C,H,W] tensor to a tensor with leading dimension B;
    noises is [C',R,B,H,W]; sigma a float or [C]."""
    x = x.to(torch.float32)
    B, C, H, W = x.shape
    chans = list(range(C)) if channels is None else list(channels)
    sig = torch.as_tensor(sigma, dtype=torch.float32).expand(C)
    noises = noises.to(torch.float32)
    R = noises.shape[1]
    assert tuple(noises.shape) == (len(chans), R, B, H, W)
    with torch.no_grad():
        base = phi(x.double()).double().reshape(B, -1)
        terms = torch.zeros(len(chans), R, B, 2, dtype=torch.float64)
        for ii, c in enumerate(chans):
            s = sig[c] * factor                       # float32
            for r in range(R):
                xp = x.clone()
                xp[:, c] = x[:, c] + noises[ii, r] * s
                d = phi(xp.double()).double().reshape(B, -1) - base
                terms[ii, r, :, 0] = d.abs().sum(1)
                terms[ii, r, :, 1] = d.sum(1)
    count = R * B * base.shape[1]
    s64 = (sig[chans] * factor).double()
    absolute = terms[..., 0].sum((1, 2)) / (count * s64)
    signed = terms[..., 1].sum((1, 2)) / (count * s64)
    return absolute, signed, absolute / absolute.sum(), terms


def sens_model_state():
    """The test network: the recipe weights for 4 input channels with every BN
    running_var at 0.25 (activations of a useful size in eval mode) and the
    input columns 4c..4c+3 of the first convolution (the pixel-unshuffled
    planes of input channel c) scaled by GAINS[c], so the four channels have
    clearly separated sensitivities."""
    sd = make_state(4, 42)
    for k in sd:
        if k.endswith("running_var"):
            sd[k] = np.full_like(sd[k], 0.25)
    w = sd["conv2.conv.0.weight"].copy()
    for c, g in enumerate(GAINS):
        w[:, 4 * c:4 * c + 4] *= np.float32(g)
    sd["conv2.conv.0.weight"] = w
    return sd


E2E_FACTOR, E2E_REPEATS = 0.5, 2


@functools.lru_cache(maxsize=None)
def e2e_case():
    """The end-to-end configuration and its reference, computed once:
    (x [2,4,64,64], sigma [4], noises [4,2,2,64,64], (absolute, signed, relative, terms))."""
    x = torch.from_numpy(synthetic_batch(2, 4, 64, 64)[0])
    sigma = torch.linspace(1, 2, 4)
    noises = torch.randn((4, E2E_REPEATS, 2, 64, 64), generator=torch.Generator().manual_seed(11))
    ref = sensitivity_ref(oracle_phi(sens_model_state()), x, sigma, noises, E2E_FACTOR)
    return x, sigma, noises, ref


def oracle_phi(np_sd):
    """The CPU oracle's eval forward on the given numpy state (the oracle runs
    in float32, the arithmetic the project's output bound OUT_ABS is stated
    against; the sums over its outputs are float64)."""
    sd = O.torch_state(np_sd)

    def phi(x):
        return O.forward(sd, x, training=False, masks=None, dropout_rate=0.0)[0]
    return phi
