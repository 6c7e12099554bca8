"""CPU: the comparator of the 16-bit train-path tests (f16_util.py) proves
itself. A CPU stand-in kernel (fp32 convolution / fp32 elementwise arithmetic
of the rounded operands, stored through .half() / .to(bfloat16)) passes every
bound, each listed mutant of it fails on at least one element, and the three
extra regimes (grad, tiny_out, overflow) have the properties the GPU tests
lean on, asserted on the float64 reference alone."""
import pytest
import torch
import torch.nn.functional as F

import eval_util as E
import f16_util as U

torch.set_num_threads(16)

SHAPES = [(2, 9, 11, 32, 64, 3), (3, 7, 5, 32, 128, 1)]
OVERFLOW_SHAPES = [(2, 9, 11, 32, 64, 3), (1, 351, 350, 64, 128, 1)]
TINY_SHAPES = [(2, 9, 11, 32, 64, 3), (3, 7, 5, 32, 128, 1)]


def store(t, fmt):
    return t.half() if fmt == "f16" else t.to(torch.bfloat16)


def standin_conv(x, w, b):
    return F.conv2d(x, w, b, padding=w.shape[-1] // 2)


def gemm_ratio(y, case, fmt):
    """worst err / bound of a stored conv output y against the case's float64 reference."""
    ref = U.conv_ref(case.x, case.w, case.b)
    S = U.conv_ref(case.x, case.w, case.b, absval=True)
    K = case.k * case.k * case.ci
    return U.ratio(y, ref, U.gemm_bound(ref, S, K, fmt))


# ---- the stored-GEMM bound ---------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("B,H,W,ci,co,k", SHAPES)
def test_gemm_bound_standin_and_mutants(B, H, W, ci, co, k, fmt):
    case = E.make_case(B, H, W, ci, co, k, fmt=fmt)
    acc = standin_conv(case.x, case.w, case.b)
    r = gemm_ratio(store(acc, fmt), case, fmt)
    print(f"stand-in {fmt}: {r:.3f}")
    assert r <= 1.0
    mutants = {}
    mutants["toward_zero"] = U.toward_zero_f16(acc) if fmt == "f16" else U.toward_zero_bf16(acc)
    if fmt == "f16":
        mutants["bf16_rounding"] = acc.to(torch.bfloat16).float().half()
    # one tap reads the pixel to its left
    w0 = case.w.clone()
    tap = torch.zeros_like(case.w)
    tap[:, :, 0, 0] = case.w[:, :, 0, 0]
    w0[:, :, 0, 0] = 0
    mutants["tap_shift"] = store(standin_conv(case.x, w0, case.b)
                                 + standin_conv(torch.roll(case.x, 1, 3), tap, None), fmt)
    b1 = case.b.clone()
    b1[5] = 0
    mutants["bias_dropped"] = store(standin_conv(case.x, case.w, b1), fmt)
    xs = case.x.clone()
    xs[:, 8:16], xs[:, 16:24] = case.x[:, 16:24], case.x[:, 8:16]
    mutants["chunk_swapped"] = store(standin_conv(xs, case.w, case.b), fmt)
    for name, y in mutants.items():
        rm = gemm_ratio(y, case, fmt)
        print(f"  {name}: {rm:.3g}")
        assert rm > 1.0, name


@pytest.mark.parametrize("B,H,W,ci,co,k", TINY_SHAPES)
def test_tiny_out_regime(B, H, W, ci, co, k):
    case = U.make_tiny_case(B, H, W, ci, co, k)
    assert torch.equal(case.x.half().float(), case.x) and torch.equal(case.w.half().float(), case.w)
    ref = U.conv_ref(case.x, case.w, case.b)
    a = ref.abs()
    sub = ((a < U.F16_MIN_NORMAL) & (a >= 2.0 ** -24)).double().mean().item()
    below = (a < 2.0 ** -24).double().mean().item()
    print(f"tiny_out: subnormal {sub:.3f}, below 2^-24 {below:.3f}")
    assert sub >= 0.25 and below >= 0.05
    acc = standin_conv(case.x, case.w, case.b)
    assert gemm_ratio(acc.half(), case, "f16") <= 1.0
    assert gemm_ratio(U.flush_subnormal(acc.half()), case, "f16") > 1.0      # results flushed
    assert gemm_ratio(U.toward_zero_f16(acc), case, "f16") > 1.0


@pytest.mark.parametrize("B,H,W,ci,co,k", SHAPES)
def test_grad_regime(B, H, W, ci, co, k):
    case = U.make_grad_case(B, H, W, ci, co, k, "f16")
    assert torch.equal(case.x.half().float(), case.x)
    share = U.subnormal_share(case.x)
    print(f"grad: subnormal share {share:.3f}")
    assert share >= 0.25
    assert case.x.abs().max().item() <= 16.0 and (case.x != 0).double().mean().item() >= 0.95
    acc = standin_conv(case.x, case.w, None)
    case.b = None
    assert gemm_ratio(acc.half(), case, "f16") <= 1.0
    # subnormal operands flushed to zero
    assert gemm_ratio(standin_conv(U.flush_subnormal(case.x), case.w, None).half(), case, "f16") > 1.0
    # bf16 takes the normal regime
    assert U.subnormal_share(U.make_grad_case(B, H, W, ci, co, k, "bf16").x) < 0.01


@pytest.mark.parametrize("B,H,W,ci,co,k", OVERFLOW_SHAPES)
def test_overflow_regime(B, H, W, ci, co, k):
    case = U.make_overflow_case(B, H, W, ci, co, k)
    base = E.make_case(B, H, W, ci, co, k, fmt="f16")
    assert int(case.hot.sum()) == co // 4
    assert torch.equal(case.w[~case.hot], base.w[~case.hot]) and torch.equal(case.x, base.x)
    ref = U.conv_ref(case.x, case.w, case.b)
    S = U.conv_ref(case.x, case.w, case.b, absval=True)
    K = k * k * ci
    inf, amb = U.overflow_classes(ref, S, K)
    f_inf, f_amb = inf.double().mean().item(), amb.double().mean().item()
    print(f"overflow: inf {f_inf:.4f} ambiguous {f_amb:.6f}")
    assert f_inf >= 0.01 and (~inf).double().mean().item() >= 0.5 and f_amb <= 1e-3
    assert not inf[:, ~case.hot].any()                      # the other channels stay finite
    assert inf[:, case.hot].double().mean().item() >= 0.2   # the scaled ones straddle 65504
    assert (~inf[:, case.hot]).double().mean().item() >= 0.2
    y = standin_conv(case.x, case.w, case.b).half()
    assert check_overflow(y, ref, S, K) <= 1.0
    sat = torch.clamp(standin_conv(case.x, case.w, case.b), -U.F16_MAX, U.F16_MAX).half()
    with pytest.raises(AssertionError):
        check_overflow(sat, ref, S, K)


def check_overflow(y, ref, S, K):
    """The overflow comparison of the GPU test: outside the ambiguous elements
    finiteness and sign as the reference's, the finite ones within the bound."""
    inf, amb = U.overflow_classes(ref, S, K)
    yd = y.double()
    ok = ~amb
    assert torch.equal(torch.isinf(yd)[ok], inf[ok])
    assert not torch.isnan(yd).any()
    assert torch.equal(torch.sign(yd)[ok & inf], torch.sign(ref)[ok & inf])
    fin = ok & ~inf
    return U.ratio(yd[fin], ref[fin], U.gemm_bound(ref, S, K, "f16")[fin])


# ---- the fp32 weight-gradient bound --------------------------------------------------
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("B,H,W,ci,co,k", SHAPES)
def test_wgrad_bound_standin_and_mutants(B, H, W, ci, co, k, fmt):
    case = E.make_case(B, H, W, ci, co, k, fmt=fmt)
    g = U.gen(B, H, W, ci, co, k, 3)
    dy = (U.grad_values((B, co, H, W), g, fmt) if fmt == "f16"
          else U.normal_values((B, co, H, W), g, fmt))
    ref = U.wgrad_ref(case.x, dy, k)
    bound = U.wgrad_bound(U.wgrad_ref(case.x, dy, k, absval=True), B * H * W)

    def standin(a, d):
        return torch.nn.grad.conv2d_weight(a, case.w.shape, d, padding=k // 2)

    r = U.ratio(standin(case.x, dy), ref, bound)
    print(f"wgrad stand-in {fmt}: {r:.3f}")
    assert r <= 1.0
    mutants = {"tap_shift": standin(torch.roll(case.x, 1, 3), dy)}
    xs = case.x.clone()
    xs[:, 8:16], xs[:, 16:24] = case.x[:, 16:24], case.x[:, 8:16]
    mutants["chunk_swapped"] = standin(xs, dy)
    if fmt == "f16":
        mutants["operands_flushed"] = standin(case.x, U.flush_subnormal(dy))
    for name, dw in mutants.items():
        assert U.ratio(dw, ref, bound) > 1.0, name


# ---- the elementwise bound -----------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_elementwise_bound_standin_and_mutants(fmt):
    B, C, H, W = 2, 64, 6, 5
    g = U.gen(B, C, H, W, 4)
    y = U.normal_values((B, C, H, W), g, fmt)
    res = U.normal_values((B, C, H, W), g, fmt)
    scale = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    shift = torch.randn(C, generator=g)
    mask = (torch.rand(B, C, generator=g) > 0.2).float() / 0.8
    z, A, bound = U.bn_act_ref(y, scale, shift, fmt, res=res, mask=mask)

    def standin(res_=res, mask_=mask):
        t = y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        return torch.where(t > 0, t, t * 0.2) * mask_[:, :, None, None] + res_

    acc = standin()
    assert U.ratio(store(acc, fmt), z, bound) <= 1.0
    mutants = {"toward_zero": U.toward_zero_f16(acc) if fmt == "f16" else U.toward_zero_bf16(acc),
               "res_dropped": store(standin(res_=torch.zeros_like(res)), fmt),
               "mask_other_image": store(standin(mask_=mask.flip(0)), fmt)}
    if fmt == "f16":
        mutants["bf16_rounding"] = acc.to(torch.bfloat16).float().half()
    for name, out in mutants.items():
        assert U.ratio(out, z, bound) > 1.0, name


def test_elementwise_bound_f16_edges():
    """Subnormal results (flush mutant) and overflow (saturation mutant) through
    the elementwise bound: bn_act of tiny and of huge activations."""
    B, C, H, W = 1, 32, 8, 8
    g = U.gen(B, C, H, W, 5)
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.zeros(C)
    y = (torch.randn(B, C, H, W, generator=g) * 2.0 ** -17).half().float()
    z, A, bound = U.bn_act_ref(y, scale, shift, "f16")
    acc = torch.where(y > 0, y * scale.view(1, -1, 1, 1), y * scale.view(1, -1, 1, 1) * 0.2)
    assert ((z.abs() < U.F16_MIN_NORMAL) & (z != 0)).double().mean().item() >= 0.25
    assert U.ratio(acc.half(), z, bound) <= 1.0
    assert U.ratio(U.flush_subnormal(acc.half()), z, bound) > 1.0
    y = (torch.randn(B, C, H, W, generator=g) * 40000).clamp(-60000, 60000).half().float()
    assert torch.isfinite(y).all()
    z, A, bound = U.bn_act_ref(y, scale, shift, "f16")
    acc = torch.where(y > 0, y * scale.view(1, -1, 1, 1), y * scale.view(1, -1, 1, 1) * 0.2)
    inf = z.abs() >= U.F16_INF_FROM
    assert inf.double().mean().item() >= 0.01
    got = acc.half().double()
    assert torch.equal(torch.isinf(got), inf)
    sat = torch.clamp(acc, -U.F16_MAX, U.F16_MAX).half().double()
    assert not torch.equal(torch.isinf(sat), inf)


# ---- the references themselves ---------------------------------------------------------
@pytest.mark.parametrize("hi,wi,ho,wo", [(4, 5, 8, 10), (8, 10, 4, 5), (1, 1, 2, 2), (5, 5, 5, 5), (67, 120, 134, 240)])
def test_lin_matrix_is_aten_bilinear(hi, wi, ho, wo):
    g = U.gen(hi, wi, ho, wo)
    x = torch.randn(2, 3, hi, wi, generator=g)
    wy, wx = U.resize_mats(hi, wi, ho, wo)
    ref = F.interpolate(x, size=(ho, wo), mode="bilinear", align_corners=True)
    assert (U.resample(x, wy, wx) - ref.double()).abs().max().item() <= 1e-5
    assert (wy.sum(1) - 1).abs().max().item() <= 1e-6 and (wx >= 0).all()
    xr = x.clone().requires_grad_(True)
    gy = torch.randn(2, 3, ho, wo, generator=g)
    F.interpolate(xr, size=(ho, wo), mode="bilinear", align_corners=True).backward(gy)
    assert (U.resample(gy, wy.t(), wx.t()) - xr.grad.double()).abs().max().item() <= 2e-5


def test_up2_mats_are_the_two_step_path():
    h, w, th, tw = 5, 7, 9, 16
    x = torch.randn(1, 2, h, w, generator=U.gen(h, w))
    wy, wx = U.up2_mats(h, w, th, tw)
    ref = F.interpolate(F.interpolate(x, size=(2 * h, 2 * w), mode="bilinear", align_corners=True),
                        size=(th, tw), mode="bilinear", align_corners=True)
    assert (U.resample(x, wy, wx) - ref.double()).abs().max().item() <= 1e-5


@pytest.mark.parametrize("k", [1, 3])
def test_conv_references_are_autograd(k):
    B, H, W, ci, co = 2, 5, 6, 8, 16
    g = U.gen(k)
    x = torch.randn(B, ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(co, ci, k, k, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, co, H, W, generator=g, dtype=torch.float64)
    F.conv2d(x, w, padding=k // 2).backward(dy)
    assert (U.dgrad_ref(dy, w.detach()) - x.grad).abs().max().item() <= 1e-12
    assert (U.wgrad_ref(x.detach(), dy, k) - w.grad).abs().max().item() <= 1e-12
    xp = torch.randn(B, ci, 5, 6, generator=g, dtype=torch.float64, requires_grad=True)
    F.avg_pool2d(xp, 2).backward(dy[:, :ci, :2, :3])
    assert (U.avgpool_bwd(dy[:, :ci, :2, :3], 5, 6) - xp.grad).abs().max().item() <= 1e-15


def test_prologue_ref_flags_boundary_elements():
    g = U.gen(11)
    y1 = U.normal_values((2, 32, 6, 7), g, "f16")
    sc, sh = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g)
    mask = (torch.rand(2, 32, generator=g) > 0.2).float() / 0.8
    a, d = U.prologue_ref(y1, sc, sh, mask, "f16")
    assert torch.equal(a.half().float(), a) and (d >= 0).all()
    assert (d > 0).double().mean().item() <= 0.02
    # the fp32 loader arithmetic lands on a or one grid step from it, only where d says so
    t = y1 * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    a32 = (torch.where(t > 0, t, t * 0.2) * mask[:, :, None, None]).half().float()
    assert ((a32 - a).abs().double() <= d).all()
