"""CPU: the float64 reference of the learned feature extraction
(extract_util.reference) against torch.autograd through the plain nn.Sequential,
the exactness claim of the integer case, the FeatureExtractor / ExtractedUnet
modules' host side, and the C entries' argument validation and planning."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import extract_util as E


def plain(Cin, Hd, Cout, slope):
    return nn.Sequential(nn.Conv2d(Cin, Hd, 1), nn.LeakyReLU(slope), nn.Conv2d(Hd, Cout, 1))


def autograd64(x, dy, w1, b1, w2, b2, slope):
    net = plain(w1.shape[1], w1.shape[0], w2.shape[0], slope).double()
    with torch.no_grad():
        net[0].weight.copy_(torch.from_numpy(w1.astype(np.float64))[:, :, None, None])
        net[0].bias.copy_(torch.from_numpy(b1.astype(np.float64)))
        net[2].weight.copy_(torch.from_numpy(w2.astype(np.float64))[:, :, None, None])
        net[2].bias.copy_(torch.from_numpy(b2.astype(np.float64)))
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    y = net(xt)
    y.backward(torch.from_numpy(dy.astype(np.float64)))
    return {"y": y.detach().numpy(), "dx": xt.grad.numpy(),
            "dw1": net[0].weight.grad.numpy()[:, :, 0, 0], "db1": net[0].bias.grad.numpy(),
            "dw2": net[2].weight.grad.numpy()[:, :, 0, 0], "db2": net[2].bias.grad.numpy()}


@pytest.mark.parametrize("maker", ["gaussian", "integer"])
@pytest.mark.parametrize("name", list(E.SHAPES))
def test_reference_matches_autograd_float64(name, maker):
    shape, Cin, Hd, Cout = E.SHAPES[name]
    make = E.gaussian_case if maker == "gaussian" else E.integer_case
    case = make(shape, Cin, Hd, Cout, seed=3)
    r = E.reference(*case, sums=False)
    if maker == "integer":   # torch's convention at pre == 0 is exercised
        assert (r.pre == 0).sum() >= 5
    want = autograd64(*case)
    for k, w in want.items():
        got = getattr(r, k)
        scale = max(1.0, float(np.abs(w).max()))
        assert np.abs(got - w).max() <= 1e-12 * scale, k


def test_integer_case_is_exact_in_fp32():
    """Every intermediate and result of the largest fixed shape is a multiple of
    2^-4 below 2^24 in magnitude: each fp32 evaluation order gives it exactly."""
    shape, Cin, Hd, Cout = E.SHAPES["w73"]
    r = E.reference(*E.integer_case(shape, Cin, Hd, Cout, seed=1), sums=False)
    assert np.abs(r.dh).max() <= 8 and np.abs(r.h).max() <= 33
    for k in ("pre", "h", "g", "dh", "y") + E.GRADS:
        v = getattr(r, k)
        assert np.array_equal(v * 16, np.round(v * 16)), k
        assert np.abs(v).max() < 2 ** 24, k
    # partial sums too: the sums of absolute values stay below 2^24
    s = E.reference(*E.integer_case(shape, Cin, Hd, Cout, seed=1))
    N = shape[0] * shape[1] * shape[2]
    for k in ("dw1", "db1", "dw2", "db2"):
        n = N * (Cout if k in ("dw1", "db1") else (Cin + 1 if k == "dw2" else 1))
        assert (getattr(s, "bound_" + k) / ((n + 2) * E.U24)).max() < 2 ** 24, k


def test_gaussian_case_separates_pre_from_zero():
    shape, Cin, Hd, Cout = E.SHAPES["w73"]
    r = E.reference(*E.gaussian_case(shape, Cin, Hd, Cout, seed=0))
    assert (np.abs(r.pre) >= r.S_pre * 2.0 ** -10).all()
    assert (r.pre < 0).any() and (r.pre > 0).any()


def test_feature_extractor_is_the_plain_module():
    from nsm_amd import FeatureExtractor
    torch.manual_seed(0)
    m = FeatureExtractor()
    p = plain(15, 16, 4, 0.2)
    sd, psd = m.net.state_dict(), p.state_dict()
    assert list(m.state_dict()) == ["net." + k for k in psd]
    assert [tuple(v.shape) for v in m.state_dict().values()] == [tuple(v.shape) for v in psd.values()]
    # both directions
    p.load_state_dict(sd)
    m2 = FeatureExtractor()
    m2.load_state_dict({"net." + k: v for k, v in p.state_dict().items()})
    x = torch.randn(2, 15, 6, 5)
    assert torch.equal(m(x), p(x)) and torch.equal(m2(x), p(x))
    assert m(x[0]).shape == (1, 4, 6, 5)
    # torch's initialisation: the same draws as the plain module's constructor
    torch.manual_seed(5)
    a = FeatureExtractor(7, 3, 9, 0.1)
    torch.manual_seed(5)
    b = plain(7, 9, 3, 0.1)
    for u, v in zip(a.net.parameters(), b.parameters()):
        assert torch.equal(u, v)
    with pytest.raises(ValueError, match="float32"):
        m(x.double())
    with pytest.raises(ValueError, match="in_channels"):
        FeatureExtractor(33)


def test_extracted_unet_checks_channels():
    from nsm_amd import ExtractedUnet, FeatureExtractor, Unet
    with pytest.raises(ValueError, match="4 channels.*takes 7"):
        ExtractedUnet(FeatureExtractor(15, 4), Unet(in_ch=7))
    m = ExtractedUnet(FeatureExtractor(15, 4), Unet(in_ch=4))
    assert m._grad_allreduce is None
    assert len(list(m.parameters())) == 4 + len(list(m.unet.parameters()))
    with pytest.raises(NotImplementedError, match="all-reduce"):
        m.data_parallel()


def test_argument_validation_and_plan_without_gpu():
    import nsm_amd._lib as L
    lib = L.lib
    assert lib.nsm_extract_fwd(None, 1, 15, 4, 4, None, None, 16, None, None, 4, 0.2, None,
                               None) == 1
    assert "null" in L.last_error()
    p = 64   # never dereferenced: the checks come before any launch
    assert lib.nsm_extract_fwd(p, 1, 33, 4, 4, p, p, 16, p, p, 4, 0.2, p, None) == 1
    assert "33 input channels" in L.last_error()
    assert lib.nsm_extract_bwd(p, p, 1, 15, 4, 4, p, p, 33, p, p, 4, 0.2, p, p, p, p, None, p,
                               None) == 1
    assert "33 hidden channels" in L.last_error()
    assert lib.nsm_extract_bwd(p, None, 1, 15, 4, 4, p, p, 16, p, p, 4, 0.2, p, p, p, p, None, p,
                               None) == 1
    assert "null" in L.last_error()
    assert lib.nsm_extract_fwd(p + 2, 1, 15, 4, 4, p, p, 16, p, p, 4, 0.2, p, None) == 1
    assert "unaligned" in L.last_error()
    assert lib.nsm_extract_fwd(p, 1, 15, 1 << 15, 1 << 13, p, p, 16, p, p, 4, 0.2, p, None) == 1
    assert "2^31" in L.last_error()
    # the capped grid: the workspace stops growing with the image
    small = lib.nsm_extract_bwd_ws(1, 15, 5, 3, 16, 4)
    a = lib.nsm_extract_bwd_ws(8, 15, 512, 512, 16, 4)
    b = lib.nsm_extract_bwd_ws(8, 15, 5120, 5120, 16, 4)
    assert 0 < small <= a == b
    assert lib.nsm_extract_bwd_ws(8, 33, 512, 512, 16, 4) == 0
    from nsm_amd.extract import extract_bwd_plan
    plan = extract_bwd_plan(8, 15, 512, 512, 16, 4)
    assert plan["grid"] == plan["grid_cap"] and plan["partial"] == 15 * 16 + 16 + 16 * 4 + 4
    assert a == plan["grid"] * plan["partial"] * 4
    assert plan["tiles"] * plan["tile_units"] >= 8 * 512 * 128
    tiny = extract_bwd_plan(1, 11, 5, 3, 7, 3)
    assert tiny["grid"] == tiny["tiles"] == 1
    plan_buf = (ctypes.c_int32 * 6)()
    assert lib.nsm_extract_bwd_plan(1, 15, 4, 4, 16, 17, plan_buf) == 1
    assert "17 output channels" in L.last_error()
