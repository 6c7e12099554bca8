"""CPU: the comparator of the eval-epilogue tests (eval_util.py) is sound: it
is nn.Conv2d -> nn.BatchNorm2d.eval() -> nn.LeakyReLU(0.2) in float64, its
input maker populates both LeakyReLU branches in every case the GPU tests
run, and the large shapes land on the tiles they are written for (the host
queries need no GPU)."""
import pytest
import torch

import eval_util as E

torch.set_num_threads(16)

CONV_CASES = ([s + ("f32",) for s in E.SMALL] + [s[:6] + ("f32",) for s in E.F32_LARGE]
              + [s + (f,) for s in E.SMALL for f in ("bf16", "f16")]
              + [s[:6] + (f,) for s in E.S16_LARGE for f in ("bf16", "f16")])
WINO_CASES = ([(B, H, W, ci, co, None, "f32") for B, H, W, ci, co in E.WINO]
              + [(B, H, W, ci, co, (hi, wi), "f32") for B, hi, wi, H, W, ci, co in E.WINO_SRC]
              + [(B, H, W, ci, co, None, "bf16") for B, H, W, ci, co in E.WINO_F16]
              + [(B, H, W, ci, co, (hi, wi), "bf16") for B, hi, wi, H, W, ci, co in E.WINO_F16_SRC])


def _module_chain(case, dtype=torch.float64):
    conv = torch.nn.Conv2d(case.ci, case.co, case.k, padding=case.k // 2)
    bn = torch.nn.BatchNorm2d(case.co, eps=case.eps)
    with torch.no_grad():
        conv.weight.copy_(case.w)
        conv.bias.copy_(case.b)
        bn.weight.copy_(case.gamma)
        bn.bias.copy_(case.beta)
        bn.running_mean.copy_(case.rmean)
        bn.running_var.copy_(case.rvar)
    return conv.to(dtype), torch.nn.Sequential(bn, torch.nn.LeakyReLU(case.slope)).to(dtype).eval()


@pytest.mark.parametrize("B,H,W,ci,co,k,src_hw", [s + (None,) for s in E.SMALL]
                         + [(2, 10, 14, 32, 64, 3, (5, 7)), (1, 12, 9, 64, 32, 1, (6, 5))])
def test_eval_block_ref_is_the_module_chain(B, H, W, ci, co, k, src_hw):
    case = E.make_case(B, H, W, ci, co, k, src_hw=src_hw)
    conv, tail = _module_chain(case)
    x = case.x.double()
    if src_hw is not None:
        x = torch.nn.functional.interpolate(x, size=(H, W), mode="bilinear", align_corners=True)
    with torch.no_grad():
        c0 = conv(x)
        z0 = tail(c0)
    for res in (False, True):
        c, z = E.reference(case, res=res)
        want = z0 + case.res.double() if res else z0
        assert c.dtype == torch.float64 and z.shape == (B, co, H, W)
        assert ((c - c0).norm() / c0.norm()).item() <= 1e-12
        assert ((z - want).norm() / want.norm()).item() <= 1e-12
        assert (z - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def test_bn_vectors_are_the_affine_form():
    case = E.make_case(1, 4, 4, 32, 64, 1, seed=3)
    c, z = E.reference(case)
    scale, shift, mean, inv = E.bn_vectors(case.gamma, case.beta, case.rmean, case.rvar, case.eps)
    pre = c * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    z1 = torch.where(pre >= 0, pre, pre * case.slope)
    assert (z1 - z).abs().max().item() <= 1e-12 * z.abs().max().item()
    assert torch.equal(mean, case.rmean.double())
    assert (inv - (case.rvar.double() + case.eps).rsqrt()).abs().max().item() <= 1e-15 * inv.max().item()


def _check_maker(case):
    """The properties the GPU tests lean on."""
    pos, neg = E.branch_shares(case)
    print(f"branch shares +{pos:.3f} -{neg:.3f}")
    assert pos >= 0.25 and neg >= 0.25, (pos, neg)
    rnd = E.rounder(case.fmt)
    assert torch.equal(rnd(case.x), case.x) and torch.equal(rnd(case.res), case.res)
    frac_neg = (case.gamma < 0).float().mean().item()
    assert 0.05 <= frac_neg <= 0.5 and case.gamma.abs().min().item() >= 0.5
    assert 2.0 ** -4 <= case.rvar.min().item() and case.rvar.max().item() <= 2.0 ** 4
    assert case.rvar.max().item() / case.rvar.min().item() >= 16   # the variances do differ
    amp = case.x.abs().amax(dim=(0, 2, 3))
    assert amp.max().item() / amp.min().item() >= 4               # a permuted channel shows


@pytest.mark.parametrize("B,H,W,ci,co,k,fmt", CONV_CASES)
def test_conv_cases_populate_both_branches(B, H, W, ci, co, k, fmt):
    _check_maker(E.make_case(B, H, W, ci, co, k, fmt=fmt))


@pytest.mark.parametrize("B,H,W,ci,co,src_hw,fmt", WINO_CASES)
def test_wino_cases_populate_both_branches(B, H, W, ci, co, src_hw, fmt):
    _check_maker(E.make_case(B, H, W, ci, co, 3, fmt=fmt, src_hw=src_hw, round_w=fmt == "f32"))


def test_large_shapes_land_on_their_tiles():
    """nsm_conv_stat_rows / _bf16 report the M tile (256 for the 512-row one)."""
    from nsm_amd._lib import lib
    for B, H, W, ci, co, k, rows in E.F32_LARGE:
        assert lib.nsm_conv_stat_rows(B, H, W, co) == rows, (B, H, W, co)
        assert (B * H * W) % rows != 0
    for B, H, W, ci, co, k, rows in E.S16_LARGE:
        assert lib.nsm_conv_stat_rows_bf16(B, H, W, co) == rows, (B, H, W, co)
        assert (B * H * W) % rows != 0
    # one row fewer than the threshold falls back to the smaller tile
    assert lib.nsm_conv_stat_rows(1, 1, 65408, 128) == 64
    assert lib.nsm_conv_stat_rows(1, 1, 524160, 64) == 128
    for B, H, W, ci, co, k in E.SMALL:
        assert lib.nsm_conv_stat_rows(B, H, W, co) == 64
