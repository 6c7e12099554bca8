"""GPU: the stages of the fp32 Winograd convolutions on pre-split (h2)
operands, one C entry at a time, against the float64 restatement of that stage
alone under the element-wise bounds of tests/wino_util.py (derived there; none
measured on the kernels): the input transforms (fp32 and h2, with the fused
align_corners resize), the dual transforms (plain and BN-fused), the filter
transforms, the batched h2 GEMM on every tile of its policy, the output
transforms, the h2 weight gradient on every tile of its plan, and one chained
convolution per tile. The worst err / bound of every stage goes to
parity_margins.json as wino_f32_ops.<stage>."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f16_util as H
import f32_util as S
import wino_util as Wn
from util import record_margin

pytestmark = pytest.mark.gpu
KINDS = ["calib", "spread"]
MIN_TINY = 0.10


@pytest.fixture(scope="module")
def ops(device):
    from nsm_amd import ops as O
    prev = O.set_f32_split(2)
    yield O
    O.set_f32_split(prev)


_WORST = {}


def check(family, case_id, r):
    """assert a worst err / bound ratio, recording the family's worst."""
    print(f"{family} {case_id}: worst err / bound {r:.3f}")
    if r >= _WORST.get(family, (-1.0, None))[0]:
        _WORST[family] = (float(r), case_id)
        record_margin("wino_f32_ops." + family, worst_err_over_bound=float(r), case=case_id)
    assert r <= 1.0, (family, case_id, r)


def sid(*s):
    return "x".join(str(v) for v in s)


def slot_holding(ops, device, value):
    """A slot whose content is `value` (one line set: the readers take the maximum)."""
    s = ops.amax_slots(1, device)
    s.view(torch.float32)[0] = value
    return s


def make_x(kind, B, H_, W_, C, seed=0):
    return (Wn.make_spread if kind == "spread" else Wn.make_calib)(B, H_, W_, C, seed)


def h2_check(family, case_id, t, ref, tbound, slot, beta, spread):
    """Both storage bounds of an h2 tensor against ref [nb][rows][C]; on a
    spread case the reference's share below 2^-17 of P is asserted too."""
    C = ref.shape[-1]
    r2, b2 = ref.reshape(-1, C), tbound.reshape(-1, C)
    if spread:
        share = Wn.tiny_share(ref, Wn.h2_P(slot, beta))
        assert share >= MIN_TINY, (family, case_id, share)
    check(family, case_id, Wn.h2_ratio(t.reshape(-1, 2 * C), r2, b2, slot, beta))


# ---- input transforms ----------------------------------------------------------------
# (B, H, W, source size or None): ragged last tiles in both directions; the
# last two sample the x2 align_corners upsample inside the transform
IN_SHAPES = [(2, 9, 11, None), (1, 13, 7, None), (2, 37, 53, None), (2, 10, 14, (5, 7)),
             (1, 34, 60, (17, 30))]
# channel counts on both sides of the wave-uniform variant (C / channels per thread % 64)
IN_CH = [(2, 32), (4, 256), (4, 64), (6, 64), (6, 96)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,H_,W_,src", IN_SHAPES)
@pytest.mark.parametrize("tile,C", IN_CH)
def test_wino_input(ops, device, tile, C, B, H_, W_, src, kind):
    """nsm_wino_input_resize (fp32 V, recorded max|V|) and nsm_wino_input_h2
    against float64 Bt d B of the (resampled) input, strided ldx."""
    hi, wi = src or (H_, W_)
    x = make_x(kind, B, hi, wi, C).to(device)
    mats = None if src is None else H.resize_mats(hi, wi, H_, W_)
    ref, bound, _ = Wn.input_ref(x, tile, src=mats)
    nb, T = (tile + 2) ** 2, ops.wino_tiles(B, H_, W_, tile)
    xr = Wn.nhwc(x, C + 32)
    cid = sid(tile, C, B, H_, W_, "up" if src else "same", kind)
    V = torch.empty(nb * T * C, device=device)
    slot = ops.amax_slots(1, device)
    ops.call("nsm_wino_input_resize", ops.ptr(xr), xr.stride(0), B, hi, wi, H_, W_, C, tile, 0,
             ops.ptr(V), ops.ptr(slot), ops.stream())
    torch.cuda.synchronize()
    assert Wn.slot_value(slot) == V.abs().max().item()          # bit for bit
    check("input", cid, H.ratio(V.view(nb, T, C), ref, bound))
    if tile == 2:
        return
    ax = ops.absmax(Wn.nhwc(x))
    Vh = torch.empty(nb * T * 2 * C, dtype=ops.H2, device=device)
    ops.call("nsm_wino_input_h2", ops.ptr(xr), xr.stride(0), B, hi, wi, H_, W_, C, tile, ops.ptr(Vh),
             ops.ptr(ax), ops.stream())
    torch.cuda.synchronize()
    h2_check("input_h2", cid, Vh, ref, bound, Wn.slot_value(ax), ops.wino_beta(tile, 0),
             kind == "spread")


@pytest.mark.parametrize("ulp", [0, 1])
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("tile", Wn.TILES)
def test_wino_beta_attained(ops, device, tile, which, ulp):
    """The input whose signs match the row of largest absolute sum, every
    element at the slot's value: one output is (row sum)^2 max. With the slot
    at a power of two and one ulp above it the h2 operand decodes finite and
    within its bound (an understated beta would store Inf)."""
    s, n = Wn.beta_pattern(tile, which)
    m = float(np.nextafter(np.float32(8.0), np.float32(16.0))) if ulp else 8.0
    C = 32
    pat = (m * torch.outer(s, s)).float()
    slot = slot_holding(ops, device, m)
    beta = ops.wino_beta(tile, which)
    nb = (tile + 2) ** 2
    if which == 0:
        x = torch.zeros(1, C, 3 * tile, 3 * tile)
        x[:, :, tile - 1:tile - 1 + n, tile - 1:tile - 1 + n] = pat
        x = x.to(device)
        ref, bound, _ = Wn.input_ref(x, tile)
        T = ops.wino_tiles(1, 3 * tile, 3 * tile, tile)
        got = torch.empty(nb * T * 2 * C, dtype=ops.H2, device=device)
        xr = Wn.nhwc(x)
        ops.call("nsm_wino_input_h2", ops.ptr(xr), C, 1, 3 * tile, 3 * tile, 3 * tile, 3 * tile, C, tile,
                 ops.ptr(got), ops.ptr(slot), ops.stream())
    elif which == 1:
        dy = pat.expand(1, C, n, n).contiguous().to(device)
        _, _, ref, bound = Wn.dual_ref(dy, tile)
        _, got = ops.wino_dual_input_h2(Wn.nhwc(dy), 1, n, n, tile, slot)
    else:
        w = pat.expand(C, C, 3, 3).contiguous().to(device)
        ref, bound = Wn.filter_ref(w, tile, False, C, C)
        U = ops.wino_weight(w, C, C, False, tile)
        got = ops.to_h2(U.view(nb * C, C), slot, beta)
    torch.cuda.synchronize()
    top = ref.abs().max().item()
    assert abs(top - float(Wn.beta_exact(tile, which)) * m) <= 1e-12 * top
    assert beta * m >= top
    assert torch.isfinite(got.float()).all()
    h2_check("beta", sid(tile, which, ulp), got, ref, bound, m, beta, False)


# ---- dual transforms ---------------------------------------------------------------------
DUAL_SHAPES = [(2, 37, 53), (3, 13, 7)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("B,H_,W_", DUAL_SHAPES)
@pytest.mark.parametrize("tile", [4, 6])
def test_wino_dual_input(ops, device, tile, B, H_, W_, C, kind):
    """nsm_wino_dual_input (fp32 Vd, dM and their recorded maxima) and
    nsm_wino_dual_input_h2 against float64 Bt dY B and A dY A^T."""
    dy = make_x(kind, B, H_, W_, C, seed=1).to(device)
    Vr, Vb, Mr, Mb = Wn.dual_ref(dy, tile)
    dyr = Wn.nhwc(dy)
    nb, T = (tile + 2) ** 2, ops.wino_tiles(B, H_, W_, tile)
    cid = sid(tile, C, B, H_, W_, kind)
    slots = ops.amax_slots(2, device)
    s0, s1 = ops.amax_slot(slots, 0), ops.amax_slot(slots, 1)
    Vd, dM = ops.wino_dual_input(dyr, B, H_, W_, tile=tile, amax=(s0, s1))
    ady = ops.absmax(dyr)
    Vh, dMh = ops.wino_dual_input_h2(dyr, B, H_, W_, tile, ady)
    torch.cuda.synchronize()
    assert Wn.slot_value(s0) == Vd.abs().max().item() and Wn.slot_value(s1) == dM.abs().max().item()
    check("dual_v", cid, H.ratio(Vd.view(nb, T, C), Vr, Vb))
    check("dual_dm", cid, H.ratio(dM.view(nb, T, C), Mr, Mb))
    sv = Wn.slot_value(ady)
    h2_check("dual_v_h2", cid, Vh, Vr, Vb, sv, ops.wino_beta(tile, 0), kind == "spread")
    h2_check("dual_dm_h2", cid, dMh, Mr, Mb, sv, ops.wino_beta(tile, 1), kind == "spread")


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("C", [32, 64, 96])
@pytest.mark.parametrize("B,H_,W_", DUAL_SHAPES)
@pytest.mark.parametrize("tile", [4, 6])
def test_wino_dual_input_bn(ops, device, tile, B, H_, W_, C, drop):
    """nsm_wino_dual_input_bn and nsm_wino_dual_input_bn_h2 (F(6x6): the
    LDS-region kernel, >= 3 regions each way with ragged last region and tile
    at 37 x 53) on spread operands: dY1 restated in float64 from the fp32
    vectors the kernels read, its bound carried through both transforms. The
    h2 scale source is the bound slot bn_bwd fills, as the model passes it."""
    g = H.gen(tile, B, H_, W_, C, 21)
    y = Wn.make_spread(B, H_, W_, C, seed=2) + torch.randn(1, C, 1, 1, generator=g) * S.spread(g, C).view(1, C, 1, 1)
    gr = Wn.make_spread(B, H_, W_, C, seed=3)
    y, gr = y.to(device), gr.to(device)
    mask = ((torch.rand(B, C, generator=g) > 0.2).float() / 0.8).to(device) if drop else None
    bn = torch.nn.BatchNorm2d(C).to(device)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g) * S.spread(g, C))
        bn.bias.uniform_(-0.2, 0.2)
    yr, gg = Wn.nhwc(y), Wn.nhwc(gr)
    st = ops.bn_train(yr, bn, C, 0.1, 1e-5)
    zeros = lambda: [torch.zeros(C, device=device) for _ in range(3)]  # noqa: E731
    d32 = ops.bn_bwd(gg, yr, st, H_ * W_, mask, C, *zeros(), defer=True)
    slots = ops.amax_slots(4, device)
    s0, s1, k1dz, bnd = (ops.amax_slot(slots, i) for i in range(4))
    Vd, dM = ops.wino_dual_input_bn(d32, yr, st, mask, B, H_, W_, tile=tile, amax=(s0, s1))
    dh = ops.bn_bwd(gg, yr, st, H_ * W_, mask, C, *zeros(), defer=True, h2=(k1dz, bnd))
    Vh, dMh = ops.wino_dual_input_bn_h2(dh, yr, st, mask, B, H_, W_, tile, bnd)
    torch.cuda.synchronize()
    assert torch.equal(d32.coef, dh.coef)
    dy, dyb = Wn.bn_dy_ref(gr, y, st.scale, st.shift, st.mean, dh.coef.view(3, C), mask)
    Vr, Vb, Mr, Mb = Wn.dual_ref(dy, tile, dyb)
    nb, T = (tile + 2) ** 2, ops.wino_tiles(B, H_, W_, tile)
    cid = sid(tile, C, B, H_, W_, "drop%d" % drop)
    assert Wn.slot_value(s0) == Vd.abs().max().item() and Wn.slot_value(s1) == dM.abs().max().item()
    check("dual_bn_v", cid, H.ratio(Vd.view(nb, T, C), Vr, Vb))
    check("dual_bn_dm", cid, H.ratio(dM.view(nb, T, C), Mr, Mb))
    sv = Wn.slot_value(bnd)
    assert sv >= (dy.abs() + dyb).max().item(), (sv, dy.abs().max().item())
    h2_check("dual_bn_v_h2", cid, Vh, Vr, Vb, sv, ops.wino_beta(tile, 0), True)
    h2_check("dual_bn_dm_h2", cid, dMh, Mr, Mb, sv, ops.wino_beta(tile, 1), True)


# ---- filters -------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("tile", Wn.TILES)
def test_wino_weight(ops, device, tile, flip):
    """nsm_wino_weight against float64 G g G^T on spread filters, real channels
    below the padded ones: the padding holds exact zeros."""
    co, ci = 50, 70
    w = Wn.make_filters(co, ci).to(device)
    n, k = (ci, co) if flip else (co, ci)
    n_p, k_p = ops.pad32(n), ops.pad32(k)
    ref, bound = Wn.filter_ref(w, tile, bool(flip), n_p, k_p)
    U = ops.wino_weight(w, n_p, k_p, bool(flip), tile).view(-1, n_p, k_p)
    torch.cuda.synchronize()
    assert (U[:, n:, :] == 0).all() and (U[:, :, k:] == 0).all()
    check("filter", sid(tile, flip), H.ratio(U, ref, bound))


def test_wino_weight_prep_h2(ops, device):
    """Prep kind 4 through StepWeights (max|w| pass, then U written pre-split),
    decoded from the slot it filled, against float64 G g G^T of spread filters."""
    from nsm_amd import Unet
    from nsm_amd.prep import StepWeights
    from nsm_amd.unet import WINOGRAD_MIN_CHANNELS, block_shapes, wino_tile
    torch.manual_seed(3)
    m = Unet(in_ch=7).to(device).train()
    blocks = (3, 6, 9)
    with torch.no_grad():
        for k in blocks:
            wt = m.block(k).conv[0].weight
            wt.copy_(Wn.make_filters(wt.shape[0], wt.shape[1], seed=k).to(device))
    sw = StepWeights(m, torch.float32, block_shapes(64, 64), True, WINOGRAD_MIN_CHANNELS, wino_tile,
                     h2=True)
    sw.run()
    torch.cuda.synchronize()
    for k in blocks:
        conv = m.block(k).conv[0]
        cip, cop = ops.pad32(conv.in_channels), ops.pad32(conv.out_channels)
        h, w_ = block_shapes(64, 64)[k]
        tile = wino_tile(cip, h, w_)
        pb = sw.block(k)
        wt = conv.weight.detach()
        for flip in (False, True):
            n_p, k_p = (cip, cop) if flip else (cop, cip)
            ref, bound = Wn.filter_ref(wt, tile, flip, n_p, k_p)
            got = pb.U1(tile, flip)
            assert got.dtype == ops.H2 and got.numel() == ref.numel() * 2
            sv = Wn.slot_value(pb.amax_U1(flip))
            assert sv == wt.abs().max().item()
            h2_check("filter_prep_h2", sid(k, tile, int(flip)), got, ref, bound, sv,
                     ops.wino_beta(tile, 2), False)


# ---- output transforms -----------------------------------------------------------------------
OUT_SHAPES = [(2, 9, 11), (1, 13, 7), (2, 37, 53)]


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("B,H_,W_", OUT_SHAPES)
@pytest.mark.parametrize("tile,N", [(2, 32), (4, 64), (6, 64), (6, 96)])
def test_wino_output(ops, device, tile, N, B, H_, W_, stats):
    """nsm_wino_output / nsm_wino_output_stats (F(6x6): the buffer-offset
    kernel) of a given M with per-component magnitudes 2^U(-3, 3), bias and a
    strided ldy, against float64 At M A + b cropped to H x W; the columns
    past cout_p of y stay untouched."""
    from nsm_amd._lib import lib
    nb, T = (tile + 2) ** 2, ops.wino_tiles(B, H_, W_, tile)
    Mp = Wn.make_planes(nb, T, N, seed=tile).to(device)
    bias = (torch.randn(N, generator=H.gen(N, tile)) * 0.1).to(device)
    ref, bound = Wn.output_ref(Mp, bias, B, H_, W_, tile)
    ld = N + 32
    y = torch.full((B * H_ * W_, ld), float("nan"), device=device)
    Mf = Mp.reshape(-1).contiguous()
    if stats:
        step = int(lib.nsm_wino_stat_step(N, tile))
        nslot = max(int(lib.nsm_wino_stat_slots(B, H_, W_, N, tile)), step)
        part = torch.empty(nslot * 3 * N, device=device)
        ops.call("nsm_wino_output_stats", ops.ptr(Mf), B, H_, W_, N, tile, ops.ptr(bias), ops.ptr(y), ld,
                 ops.ptr(part), nslot, ops.stream())
    else:
        ops.call("nsm_wino_output", ops.ptr(Mf), B, H_, W_, N, tile, ops.ptr(bias), ops.ptr(y), ld,
                 ops.stream())
    torch.cuda.synchronize()
    assert torch.isnan(y[:, N:]).all()
    got = y[:, :N].reshape(B, H_, W_, N).permute(0, 3, 1, 2)
    check("output_stats" if stats else "output", sid(tile, N, B, H_, W_), H.ratio(got, ref, bound))


# ---- the batched h2 GEMM -------------------------------------------------------------------
TILE_OF = {1: (256, 256), 2: (256, 128), 3: (128, 128), 4: (256, 64), 5: (128, 32)}
BIG = (2, 228, 228)     # F(6x6): T = 2888 = 12 row tiles of 256 (ragged), 64 x 12 = 768 blocks
# (B, H, W, tile, cin_p, cout_p, expected tile, expected form)
GEMM_CASES = (
    # 256x256 and 256x128 at 1, 2, 3 and 6 K-tiles of 64 f16 columns: two and six run the
    # persistent kernel (K % 128 == 0), one and three one tile per block
    [BIG + (6, ci, co, t, "gemm_h2p" if ci % 64 == 0 else "gemm_h2q")
     for co, t in ((256, 1), (128, 2)) for ci in (32, 64, 96, 192)]
    # 128x128, 256x64, 128x32 (cout_p 32 and 96) at T = 8 and T = 42 / 90
    + [s + (tile, ci, co, t, "gemm_h2")
       for co, t in ((128, 3), (64, 4), (32, 5), (96, 5))
       for s, tile, ci in (((2, 12, 12), 6, 64), ((1, 40, 36), 6, 32), ((1, 40, 36), 4, 96))])


def run_gemm_h2(ops, device, V, U, B, H_, W_, tile, sv, su, plan):
    """M of nsm_wino_gemm_h2 on nsm_to_h2 of fp32 V [nb][T][K], U [nb][N][K]
    with slots holding sv / su and the betas the model passes; asserts the
    plan and the guard behind Mb."""
    nb, T, K = V.shape
    N = U.shape[1]
    assert ops.wino_gemm_h2_plan(B, H_, W_, K, N, tile) == plan
    bv, bu = ops.wino_beta(tile, 0), ops.wino_beta(tile, 2)
    av, au = slot_holding(ops, device, sv), slot_holding(ops, device, su)
    Vh = ops.to_h2(V.reshape(nb * T, K).contiguous(), av, bv)
    Uh = ops.to_h2(U.reshape(nb * N, K).contiguous(), au, bu)
    guard = 4096
    Mb = torch.full((nb * T * N + guard,), float("nan"), device=device)
    ops.call("nsm_wino_gemm_h2", ops.ptr(Vh), ops.ptr(Uh), B, H_, W_, K, N, tile, ops.ptr(Mb),
             ops.ptr(av), bv, ops.ptr(au), bu, ops.stream())
    torch.cuda.synchronize()
    assert torch.isnan(Mb[nb * T * N:]).all()
    return Mb[:nb * T * N].view(nb, T, N), Wn._mv(sv, bv), Wn._mv(su, bu)


def gemm_operands(kind, nb, T, K, N, device):
    V = Wn.make_planes(nb, T, K, seed=1, spread=kind == "spread").to(device)
    U = Wn.make_planes(nb, N, K, seed=2, spread=kind == "spread", lo=-6, hi=-3).to(device)
    return V, U


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,H_,W_,tile,ci,co,t,form", GEMM_CASES)
def test_wino_gemm_h2(ops, device, B, H_, W_, tile, ci, co, t, form, kind):
    """Every tile and kernel form of the default policy against float64
    V[c] U[c]^T, every component; T no multiple of 256 or 128."""
    nb, T = (tile + 2) ** 2, ops.wino_tiles(B, H_, W_, tile)
    assert T % 128 != 0
    V, U = gemm_operands(kind, nb, T, ci, co, device)
    sv, su = V.abs().max().item(), U.abs().max().item()
    got, mv, mu = run_gemm_h2(ops, device, V, U, B, H_, W_, tile, sv, su, (t, form))
    ref, bound = Wn.gemm_ref(V, U, mv, mu)
    if kind == "spread":
        # the floor is the leading term on part of the outputs
        fl = bound - S.gemm_bound(2, V.double().abs() @ U.double().abs().transpose(1, 2), ci,
                                  floor=torch.zeros((), dtype=torch.float64, device=device))
        assert (fl > 0.5 * bound).double().mean().item() > 0.01
    check("gemm_h2_%dx%d_%s" % (TILE_OF[t] + (form,)), sid(B, H_, W_, tile, ci, co, kind),
          H.ratio(got, ref, bound))


@pytest.mark.parametrize("variant", ["slots_x8", "zero_u"])
@pytest.mark.parametrize("B,H_,W_,tile,ci,co,t,form",
                         [BIG + (6, 64, 256, 1, "gemm_h2p"), BIG + (6, 96, 128, 2, "gemm_h2q"),
                          (1, 40, 36, 6, 32, 96, 5, "gemm_h2")])
def test_wino_gemm_h2_scales(ops, device, B, H_, W_, tile, ci, co, t, form, variant):
    """Slots holding 8x the maxima (a coarser grid, within its own larger
    floor) and an all-zero U (M exactly zero)."""
    nb, T = (tile + 2) ** 2, ops.wino_tiles(B, H_, W_, tile)
    V, U = gemm_operands("spread", nb, T, ci, co, device)
    sv, su = V.abs().max().item(), U.abs().max().item()
    if variant == "zero_u":
        U = torch.zeros_like(U)
        got, _, _ = run_gemm_h2(ops, device, V, U, B, H_, W_, tile, sv, su, (t, form))
        assert (got == 0).all()
        return
    got, mv, mu = run_gemm_h2(ops, device, V, U, B, H_, W_, tile, 8 * sv, 8 * su, (t, form))
    ref, bound = Wn.gemm_ref(V, U, mv, mu)
    check("gemm_h2_slots_x8", sid(B, H_, W_, tile, ci, co), H.ratio(got, ref, bound))


# ---- the h2 weight gradient ------------------------------------------------------------------
# (B, H, W, tile, cin_p, cout_p, (BM, BN)): the nine tiles of plan_wino_wgrad at F(2x2),
# T = 1026 (an odd split count with a short last split), two at the larger
# tiles, and 256x256 where both channel counts are multiples of 256
WG_CASES = ([(2, 37, 53, 2, ci, co, (min(co, 128), min(ci, 128))) for co in (32, 64, 128) for ci in (32, 64, 128)]
            + [(2, 37, 53, 4, 64, 64, (64, 64)), (2, 37, 53, 6, 64, 32, (32, 64))]
            + [BIG + (6, 256, 256, (256, 256))])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,H_,W_,tile,ci,co,bmn", WG_CASES)
def test_wino_wgrad_h2(ops, device, B, H_, W_, tile, ci, co, bmn, kind):
    """nsm_conv3x3_wgrad_wino_h2 on h2 dM and V made by nsm_to_h2 of the
    float64 transforms rounded to fp32 (the stage alone), real channel counts
    below the padded ones, a workspace of exactly the entry's size."""
    from nsm_amd._lib import lib
    nb, T = (tile + 2) ** 2, ops.wino_tiles(B, H_, W_, tile)
    BM, BN, splits, kchunk = ops.wino_wgrad_h2_plan(B, H_, W_, ci, co, tile)
    assert (BM, BN) == bmn and (splits - 1) * kchunk < T <= splits * kchunk
    if tile == 2:
        assert splits % 2 == 1 and splits >= 3 and T % kchunk != 0
    cin, cout = ci - 3, co - 5
    x = make_x(kind, B, H_, W_, ci, seed=4).to(device)
    dy = make_x(kind, B, H_, W_, co, seed=5).to(device)
    V = Wn.input_ref(x, tile)[0].float()
    dM = Wn.dm_ref(dy, tile)[0].float()
    ax, ady = ops.absmax(Wn.nhwc(x)), ops.absmax(Wn.nhwc(dy))
    b0, b1 = ops.wino_beta(tile, 0), ops.wino_beta(tile, 1)
    Vh = ops.to_h2(V.reshape(nb * T, ci).contiguous(), ax, b0)
    dMh = ops.to_h2(dM.reshape(nb * T, co).contiguous(), ady, b1)
    n = int(lib.nsm_wino_wgrad_h2_ws(B, H_, W_, ci, co, tile))
    assert n == nb * splits * co * ci + (nb * co * ci if splits > 1 else 0)
    guard = 1024
    ws = torch.full((n + guard,), float("nan"), device=device)
    dw = torch.empty(cout, cin, 3, 3, device=device)
    ops.call("nsm_conv3x3_wgrad_wino_h2", ops.ptr(dMh), ops.ptr(Vh), B, H_, W_, ci, co, cin, cout, tile,
             ops.ptr(dw), ops.ptr(ws), n, ops.ptr(ady), ops.ptr(ax), ops.stream())
    torch.cuda.synchronize()
    assert torch.isnan(ws[n:]).all()
    ref, bound = Wn.wgrad_ref(dM, V, tile, cout, cin, Wn._mv(Wn.slot_value(ady), b1),
                              Wn._mv(Wn.slot_value(ax), b0))
    check("wgrad_h2_%dx%d" % (BM, BN), sid(B, H_, W_, tile, ci, co, kind, "s%d" % splits),
          H.ratio(dw, ref, bound))


# ---- one chained convolution per tile ---------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tile", Wn.TILES)
def test_wino_chain(ops, device, tile, kind):
    """conv3x3_wino forward, the input gradient from wino_dual_input_h2 and
    the weight gradient on h2 operands as unet.py calls them, 64 -> 64 at
    (2, 37, 53), against float64 conv2d / autograd. The bound is the sum of the
    stage bounds, each carried through the absolute values of the later
    stages, all from the float64 stage references."""
    B, H_, W_, C = 2, 37, 53, 64
    nb, T = (tile + 2) ** 2, ops.wino_tiles(B, H_, W_, tile)
    x = make_x(kind, B, H_, W_, C, seed=6).to(device)
    dy = make_x(kind, B, H_, W_, C, seed=7).to(device)
    w = Wn.make_filters(C, C, seed=8, spread=kind == "spread").to(device)
    bias = (torch.randn(C, generator=H.gen(tile, 9)) * 0.1).to(device)
    xr, dyr = Wn.nhwc(x), Wn.nhwc(dy)
    ax, ady, aw = ops.absmax(xr), ops.absmax(dyr), ops.absmax(w.contiguous())
    b0, b1, b2 = (ops.wino_beta(tile, i) for i in range(3))
    Uh = ops.to_h2(ops.wino_weight(w, C, C, False, tile).view(nb * C, C), aw, b2)
    Udh = ops.to_h2(ops.wino_weight(w, C, C, True, tile).view(nb * C, C), aw, b2)
    y, Vh = ops.conv3x3_wino(xr, B, H_, W_, Uh, bias, C, tile=tile, keep_v=True, amax_v=ax, amax_u=aw)
    Vdh, dMh = ops.wino_dual_input_h2(dyr, B, H_, W_, tile, ady)
    dx = ops.conv3x3_wino(dyr, B, H_, W_, Udh, None, C, tile=tile, v_in=Vdh, amax_v=ady, amax_u=aw)
    dw = torch.empty(C, C, 3, 3, device=device)
    ops.conv3x3_wgrad_wino(dyr, Vh, B, H_, W_, C, C, C, dw, tile=tile, dM=dMh, amax=(ady, ax))
    torch.cuda.synchronize()
    # float64 conv2d / autograd
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yref = F.conv2d(x64, w64, bias.double(), padding=1)
    yref.backward(dy.double())
    # stage references and the chained bounds
    sx, sdy, sw = (Wn.slot_value(s) for s in (ax, ady, aw))
    Vr, eV, _ = Wn.input_ref(x, tile)
    Ur, eU = Wn.filter_ref(w, tile, False, C, C)
    Udr, eUd = Wn.filter_ref(w, tile, True, C, C)
    Vdr, eVd, Dr, eD = Wn.dual_ref(dy, tile)
    Mr, eM = Wn.chain_gemm(Vr, eV, Ur, eU, Wn._mv(sx, b0), Wn._mv(sw, b2))
    _, yb = Wn.chain_output(Mr, eM, bias, B, H_, W_, tile)
    Mdr, eMd = Wn.chain_gemm(Vdr, eVd, Udr, eUd, Wn._mv(sdy, b0), Wn._mv(sw, b2))
    _, dxb = Wn.chain_output(Mdr, eMd, None, B, H_, W_, tile)
    _, dwb = Wn.chain_wgrad(Dr, eD, Vr, eV, tile, C, C, Wn._mv(sdy, b1), Wn._mv(sx, b0))
    img = lambda t: t.reshape(B, H_, W_, C).permute(0, 3, 1, 2)  # noqa: E731
    cid = sid(tile, kind)
    check("chain_fwd", cid, H.ratio(img(y), yref.detach(), yb))
    check("chain_dgrad", cid, H.ratio(img(dx), x64.grad, dxb))
    check("chain_wgrad", cid, H.ratio(dw, w64.grad, dwb))
