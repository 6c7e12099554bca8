"""CPU: the comparator of the fp32 direct-GEMM tests (f32_util.py) proves
itself without the kernels. Emulations of the f16x2-split GEMM and of the
bf16 three-way split (fp32 accumulation of the exact products of the 16-bit
pieces) stay within the mode-2 / mode-1 bounds on uniform and on spread
operands, and each mutant (a dropped product term, a dropped K element, the
other tensor's scale) exceeds them on at least one element: the GPU tests
would fail on a kernel that is wrong in one of these ways."""
import numpy as np
import pytest
import torch

import eval_util as E
import f32_util as U

torch.set_num_threads(16)

# (B, H, W, cin, cout, k): a 1x1 and a 3x3 of the 64-row tiles
SHAPES = [(3, 7, 5, 32, 128, 1), (2, 9, 11, 32, 64, 3)]


def make(kind, B, H, W, ci, co, k):
    if kind == "spread":
        return U.make_spread_case(B, H, W, ci, co, k)
    return E.make_case(B, H, W, ci, co, k)


def operands(case):
    """The GEMM of a case: a [M, K], b [co, K] (K ordered as im2col orders it)."""
    return U.im2col(case.x, case.k), case.w.reshape(case.co, -1)


def refs(case):
    ref = E.nhwc(U.conv_ref(case.x, case.w, None))
    S = E.nhwc(U.conv_ref(case.x, case.w, None, absval=True))
    return ref, S


@pytest.mark.parametrize("kind", ["uniform", "spread"])
@pytest.mark.parametrize("B,H,W,ci,co,k", SHAPES)
def test_f16x2_emulation_and_mutants(B, H, W, ci, co, k, kind):
    case = make(kind, B, H, W, ci, co, k)
    a, b = operands(case)
    ref, S = refs(case)
    K = k * k * ci
    ax, aw = case.x.abs().max().item(), case.w.abs().max().item()

    def bound(sx, sw):
        return U.gemm_bound(2, S, K, floor=E.nhwc(U.conv_floor(case.x, case.w, sx, sw)))

    r = U.ratio(U.f16x2_gemm(a, b, ax, aw), ref, bound(ax, aw))
    print(f"f16x2 {kind}: {r:.3f}")
    assert r <= 1.0
    # slots that hold 8x the maxima: a coarser scale, the bound from the slot values
    r8 = U.ratio(U.f16x2_gemm(a, b, 8 * ax, 8 * aw), ref, bound(8 * ax, 8 * aw))
    print(f"f16x2 {kind}, 8x slots: {r8:.3f}")
    assert r8 <= 1.0
    for name, kw in (("hl_dropped", dict(drop_hl=True)), ("last_k_dropped", dict(drop_last=True))):
        rm = U.ratio(U.f16x2_gemm(a, b, ax, aw, **kw), ref, bound(ax, aw))
        print(f"  {name}: {rm:.3g}")
        assert rm > 1.0, name


@pytest.mark.parametrize("B,H,W,ci,co,k", SHAPES)
def test_f16x2_wrong_tensor_scale(B, H, W, ci, co, k):
    """Each operand scaled from the other's maximum: with maxima 2^7 apart the
    larger operand leaves the f16 range and the smaller one loses 7 bits."""
    case = E.make_case(B, H, W, ci, co, k)
    case.w = case.w * 2.0 ** -7
    a, b = operands(case)
    ref, S = refs(case)
    ax, aw = case.x.abs().max().item(), case.w.abs().max().item()
    assert U.pow2_up(ax) >= 2.0 ** 6 * U.pow2_up(aw)
    bound = U.gemm_bound(2, S, k * k * ci, floor=E.nhwc(U.conv_floor(case.x, case.w, ax, aw)))
    assert U.ratio(U.f16x2_gemm(a, b, ax, aw), ref, bound) <= 1.0
    assert U.ratio(U.f16x2_gemm(a, b, ax, aw, swap_scales=True), ref, bound) > 1.0


@pytest.mark.parametrize("kind", ["uniform", "spread"])
@pytest.mark.parametrize("B,H,W,ci,co,k", SHAPES)
def test_bf16x6_emulation_and_mutant(B, H, W, ci, co, k, kind):
    """The exact three-way split passes and a split without the am bh term
    (2^-8 relative) fails everywhere. Without the am bm term (2^-16 relative
    at most, 2^-20 typically) the outputs that sum few products fail at K =
    32: the lone-channel rows of the spread case. At K = 288 the accumulation
    term alone, K e32 S = 2^-15.8 S, is above that term's worst case, so no
    worst-case bound can see it there: the mutant is asserted at K = 32."""
    case = make(kind, B, H, W, ci, co, k)
    a, b = operands(case)
    ref, S = refs(case)
    bound = U.gemm_bound(1, S, k * k * ci)
    r = U.ratio(U.bf16x6_gemm(a, b), ref, bound)
    print(f"bf16x6 {kind}: {r:.3f}")
    assert r <= 1.0
    assert U.ratio(U.bf16x6_gemm(a, b, drop_mh=True), ref, bound) > 1.0
    if kind == "spread" and k * k * ci == 32:
        rm = U.ratio(U.bf16x6_gemm(a, b, drop_mm=True), ref, bound)
        print(f"  mm_dropped: {rm:.3g}")
        assert rm > 1.0


@pytest.mark.parametrize("B,H,W,ci,co,k", SHAPES)
def test_mode0_bound_holds_for_fp32_chain(B, H, W, ci, co, k):
    """A plain fp32 GEMM (one rounding per K element) meets the mode-0 bound,
    and the mode-0 bound is the smallest of the three."""
    case = E.make_case(B, H, W, ci, co, k)
    a, b = operands(case)
    ref, S = refs(case)
    K = k * k * ci
    assert U.ratio(U._mm32(a, b), ref, U.gemm_bound(0, S, K)) <= 1.0
    ax, aw = case.x.abs().max().item(), case.w.abs().max().item()
    b2 = U.gemm_bound(2, S, K, floor=E.nhwc(U.conv_floor(case.x, case.w, ax, aw)))
    assert (U.gemm_bound(0, S, K) <= U.gemm_bound(1, S, K)).all() and (U.gemm_bound(0, S, K) <= b2).all()


@pytest.mark.parametrize("B,H,W,ci,co,k", SHAPES + [(1, 209, 313, 32, 32, 3)])
def test_spread_case_exercises_the_floor(B, H, W, ci, co, k):
    """A meaningful share of both operands lies below 2^-17 of the maximum,
    and on some of the outputs (those of the lone-channel rows whose one product
    is small) the floor term is at least the representation term of the bound
    (on the uniform case no operand element is that small)."""
    case = U.make_spread_case(B, H, W, ci, co, k)
    sx, sw = U.tiny_share(case.x), U.tiny_share(case.w)
    print(f"spread: share below 2^-17 of the maximum: x {sx:.3f} w {sw:.3f}")
    assert sx >= 0.1 and sw >= 0.1
    assert case.lone.any() and not case.lone.all()
    ax, aw = case.x.abs().max().item(), case.w.abs().max().item()
    S = U.conv_ref(case.x, case.w, case.b, absval=True)
    floor = U.conv_floor(case.x, case.w, ax, aw)
    material = (floor >= U.REP_F16X2 * S).double().mean().item()
    print(f"spread: floor >= the representation term on {material:.3f} of the outputs")
    assert material >= 0.01
    u = E.make_case(B, H, W, ci, co, k)
    assert U.tiny_share(u.x) <= 0.01


@pytest.mark.parametrize("B,H,W,ci,co", [(2, 9, 11, 32, 64), (2, 37, 29, 64, 32)])
def test_wgrad_bound_emulation_and_mutant(B, H, W, ci, co):
    """The 1x1 weight gradient as a GEMM over the pixels (a = dy, b = the
    activation): the f16x2 and the bf16 emulations meet wgrad_bound, a dropped
    last pixel fails it."""
    g = U.gen(B, H, W, ci, co, 6)
    x = torch.randn(B, ci, H, W, generator=g) * U.spread(g, ci, -4, 0).view(1, ci, 1, 1)
    dy = torch.randn(B, co, H, W, generator=g) * U.spread(g, co, -4, 0).view(1, co, 1, 1)
    a, b = E.nhwc(dy).t().contiguous(), E.nhwc(x).t().contiguous()        # [co, K], [ci, K]
    ref = U.wgrad_ref(x, dy, 1).view(co, ci)
    S = U.wgrad_ref(x, dy, 1, absval=True).view(co, ci)
    ady, ax = dy.abs().max().item(), x.abs().max().item()
    K = B * H * W
    b2 = U.wgrad_bound(2, S, K, floor=U.wgrad_floor(x, dy, 1, ady, ax).view(co, ci))
    assert U.ratio(U.f16x2_gemm(a, b, ady, ax), ref, b2) <= 1.0
    assert U.ratio(U.bf16x6_gemm(a, b), ref, U.wgrad_bound(1, S, K)) <= 1.0
    assert U.ratio(U._mm32(a, b), ref, U.wgrad_bound(0, S, K)) <= 1.0
    assert U.ratio(U.f16x2_gemm(a, b, ady, ax, drop_last=True), ref, b2) > 1.0


def test_pow2_up_mirrors_the_scale_exponent():
    assert U.pow2_up(1.0) == 1.0 and U.pow2_up(1.0000001) == 2.0 and U.pow2_up(0.75) == 1.0
    assert U.pow2_up(0.0) == 2.0 ** 15 and U.pow2_up(float("inf")) == 2.0 ** 15
    assert U.pow2_up(3.0e38) == 2.0 ** 128 and U.pow2_up(2.0 ** -120) == 2.0 ** -111
    assert U.pow2_up(np.float32(8 * 0.3)) == 4.0
