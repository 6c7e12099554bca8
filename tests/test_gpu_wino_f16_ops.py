"""GPU: the stages of the bf16 step's Winograd F(4x4,3x3) path on single-plane
scaled f16 operands, one C entry at a time, against the float64 restatement of
that stage alone under the element-wise bounds of tests/wino_f16_util.py
(derived there; none measured on the kernels): the input, resize, output-
gradient, dual and BN-fused dual transforms, prep kind 6, the batched GEMM
with fp32 and with f16 M (tile exponents asserted against the reference's tile
maxima) on both tiles and both kernel forms, the three output transforms with
their BN partials, the weight gradient on its planned tiles, one chained
convolution per forward tile, and the generic kernel forms in one child
process. The worst err / bound of every stage goes to parity_margins.json as
wino_f16_ops.<stage>."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import f16_util as H
import wino_f16_util as Wf
import wino_util as Wn
from util import record_margin

pytestmark = pytest.mark.gpu
KINDS = ["calib", "spread"]
MIN_TINY = 0.10
NAN = float("nan")
GUARD = 4096
SENT = 12345


@pytest.fixture(scope="module")
def ops(device):
    from nsm_amd import ops as O
    return O


_WORST = {}


def check(family, case_id, r):
    """assert a worst err / bound ratio, recording the family's worst."""
    print(f"{family} {case_id}: worst err / bound {r:.3f}")
    if r >= _WORST.get(family, (-1.0, None))[0]:
        _WORST[family] = (float(r), case_id)
        record_margin("wino_f16_ops." + family, worst_err_over_bound=float(r), case=case_id)
    assert r <= 1.0, (family, case_id, r)


def sid(*s):
    return "x".join(str(v) for v in s)


def slot_holding(ops, device, value):
    s = ops.amax_slots(1, device)
    s.view(torch.float32)[0] = value
    return s


def rows16(x, ld=None):
    """NCHW (bf16 values) -> bf16 [B H W][C] rows; ld > C: a strided view."""
    return Wn.nhwc(x.to(torch.bfloat16), ld)


def guarded16(n, device):
    """f16 buffer of n elements followed by a NaN guard: (whole, the n)."""
    buf = torch.full((n + GUARD,), NAN, dtype=torch.float16, device=device)
    return buf, buf[:n]


def guard_ok(buf, n):
    return bool(torch.isnan(buf[n:].float()).all())


def sp_check(family, cid, t, ref, tb, slot, beta, spread):
    """The storage bound of a single-plane operand against ref [36][T][C]; on
    a spread case the reference's share below 2^-29 of P is asserted too."""
    if spread:
        share = Wf.sp_tiny_share(ref, slot, beta)
        assert share >= MIN_TINY, (family, cid, share)
    r = Wf.sp_ratio(t, ref, tb, slot, beta)
    check(family, cid, r)
    return r


# ---- transforms --------------------------------------------------------------------------
TX_SHAPES = [(2, 9, 11), (1, 6, 7), (3, 13, 22)]
TX_C = [32, 128]


def run_input(ops, device, kind, B, H_, W_, C, src=None, slot_mul=1.0):
    """nsm_wino_input_f16 / _resize on a strided bf16 source -> (V, ref, tb, slot)."""
    hi, wi = src or (H_, W_)
    x = Wf.make_x(kind, B, hi, wi, C).to(device)
    if kind == "zero":
        x = torch.zeros_like(x)
    xr = rows16(x, C + 32)
    sv = x.abs().max().item() * slot_mul
    ax = ops.absmax(rows16(x))
    assert Wn.slot_value(ax) == x.abs().max().item()
    ax = slot_holding(ops, device, sv)
    T = ops.wino_tiles(B, H_, W_, 4)
    buf, V = guarded16(36 * T * C, device)
    if src is None:
        ops.call("nsm_wino_input_f16", ops.ptr(xr), xr.stride(0), B, H_, W_, C, 4, ops.ptr(V), ops.ptr(ax),
                 ops.stream())
    else:
        ops.call("nsm_wino_input_f16_resize", ops.ptr(xr), xr.stride(0), B, hi, wi, H_, W_, C, 4, ops.ptr(V),
                 ops.ptr(ax), ops.stream())
    torch.cuda.synchronize()
    assert guard_ok(buf, 36 * T * C)
    ref, tb = Wf.input_ref(x, None if src is None else H.resize_mats(hi, wi, H_, W_))
    return V, ref, tb, sv


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,H_,W_", TX_SHAPES)
@pytest.mark.parametrize("C", TX_C)
def test_wino_input_f16(ops, device, C, B, H_, W_, kind):
    """nsm_wino_input_f16 against float64 Bt d B of the bf16 input."""
    V, ref, tb, sv = run_input(ops, device, kind, B, H_, W_, C)
    sp_check("input", sid(C, B, H_, W_, kind), V, ref, tb, sv, ops.wino_beta(4, 0), kind == "spread")


# (B, hi, wi, H, W): even and odd upsampled extents
UP_SHAPES = [(2, 5, 7, 10, 14), (1, 6, 7, 11, 13), (3, 4, 11, 8, 21)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,hi,wi,H_,W_", UP_SHAPES)
@pytest.mark.parametrize("C", TX_C)
def test_wino_input_f16_resize(ops, device, C, B, hi, wi, H_, W_, kind):
    """nsm_wino_input_f16_resize against float64 Bt d B of the float64
    align_corners resample, each patch element within one bf16 rounding of it."""
    V, ref, tb, sv = run_input(ops, device, kind, B, H_, W_, C, src=(hi, wi))
    sp_check("input_resize", sid(C, B, hi, wi, H_, W_, kind), V, ref, tb, sv, ops.wino_beta(4, 0),
             kind == "spread")


def run_dual(ops, device, kind, B, H_, W_, C, slot_mul=1.0):
    """nsm_wino_dout_f16 and nsm_wino_dual_f16 of one dY -> (dM of dout, V, dM
    of dual, refs and bounds, slot)."""
    dy = Wf.make_x(kind, B, H_, W_, C, seed=1).to(device)
    if kind == "zero":
        dy = torch.zeros_like(dy)
    dyr = rows16(dy, C + 32)
    sv = dy.abs().max().item() * slot_mul
    ady = slot_holding(ops, device, sv)
    n = 36 * ops.wino_tiles(B, H_, W_, 4) * C
    (b0, dM0), (b1, V), (b2, dM) = (guarded16(n, device) for _ in range(3))
    ops.call("nsm_wino_dout_f16", ops.ptr(dyr), dyr.stride(0), B, H_, W_, C, 4, ops.ptr(dM0), ops.ptr(ady),
             ops.stream())
    ops.call("nsm_wino_dual_f16", ops.ptr(dyr), dyr.stride(0), B, H_, W_, C, 4, ops.ptr(V), ops.ptr(dM),
             ops.ptr(ady), ops.stream())
    torch.cuda.synchronize()
    assert guard_ok(b0, n) and guard_ok(b1, n) and guard_ok(b2, n)
    return dM0, V, dM, Wn.dual_ref(dy, 4), sv


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,H_,W_", TX_SHAPES)
@pytest.mark.parametrize("C", TX_C)
def test_wino_dout_dual_f16(ops, device, C, B, H_, W_, kind):
    """nsm_wino_dout_f16 and both outputs of nsm_wino_dual_f16 against float64
    A dY A^T and Bt dY B."""
    dM0, V, dM, (Vr, Vb, Mr, Mb), sv = run_dual(ops, device, kind, B, H_, W_, C)
    cid, sp = sid(C, B, H_, W_, kind), kind == "spread"
    sp_check("dout", cid, dM0, Mr, Mb, sv, ops.wino_beta(4, 1), sp)
    sp_check("dual_v", cid, V, Vr, Vb, sv, ops.wino_beta(4, 0), sp)
    sp_check("dual_dm", cid, dM, Mr, Mb, sv, ops.wino_beta(4, 1), sp)


def run_dual_bn(ops, device, kind, B, H_, W_, C, drop, given=False, slot_mul=1.0):
    """nsm_wino_dual_bn_f16 -> (V, dM, refs and bounds, slot). Every input
    comes from the seeded generator. The BN vectors and the scale slot are
    those of bn_train / bn_bwd(h2=...), as in the model; given: vectors written
    by the test (k2, k3 following the channel's gradient magnitude as the sums
    behind them do) and a slot holding slot_mul times the reference's own
    bound: the slot is the caller's, so its edges are set this way."""
    g = H.gen(B, H_, W_, C, int(drop), 51)
    y = Wf.bf(torch.randn(B, C, H_, W_, generator=g) * 2 + 0.5).to(device)
    gr = Wf.make_x(kind, B, H_, W_, C, seed=3).to(device)
    if kind == "zero":
        gr = torch.zeros_like(gr)
    mask = ((torch.rand(B, C, generator=g) > 0.2).float() / 0.8).to(device) if drop else None
    yr, gg = rows16(y, C + 32), rows16(gr, C + 64)
    if given:
        cm = gr.abs().amax((0, 2, 3)).cpu()
        scale, shift, mean = (torch.randn(C, generator=g).to(device) for _ in range(3))
        coef = torch.stack((torch.randn(C, generator=g), torch.randn(C, generator=g) * cm * 1e-2,
                            torch.randn(C, generator=g) * cm * 1e-2)).to(device).contiguous()
        dy, dyb = Wf.bn_dy_ref(gr, y, scale, shift, mean, coef, mask)
        bnd = slot_holding(ops, device, (dy.abs() + dyb).max().item() * slot_mul)
    else:
        bn = torch.nn.BatchNorm2d(C).to(device)
        with torch.no_grad():
            bn.weight.copy_(torch.randn(C, generator=g))
            bn.bias.copy_(torch.rand(C, generator=g) * 0.4 - 0.2)
        st = ops.bn_train(rows16(y), bn, C, 0.1, 1e-5)
        slots = ops.amax_slots(2, device)
        k1dz, bnd = ops.amax_slot(slots, 0), ops.amax_slot(slots, 1)
        z = [torch.zeros(C, device=device) for _ in range(3)]
        d = ops.bn_bwd(rows16(gr), rows16(y), st, H_ * W_, mask, C, *z, defer=True, h2=(k1dz, bnd))
        scale, shift, mean, coef = st.scale, st.shift, st.mean, d.coef
    n = 36 * ops.wino_tiles(B, H_, W_, 4) * C
    (b1, V), (b2, dM) = guarded16(n, device), guarded16(n, device)
    ops.call("nsm_wino_dual_bn_f16", ops.ptr(gg), gg.stride(0), ops.ptr(yr), yr.stride(0), B, H_, W_, C, 4,
             ops.ptr(scale), ops.ptr(shift), 0.2, ops.ptr(mask), ops.ptr(mean), ops.ptr(coef),
             ops.ptr(V), ops.ptr(dM), ops.ptr(bnd), ops.stream())
    torch.cuda.synchronize()
    assert guard_ok(b1, n) and guard_ok(b2, n)
    dy, dyb = Wf.bn_dy_ref(gr, y, scale, shift, mean, coef.view(3, C), mask)
    sv = Wn.slot_value(bnd)
    assert sv >= dy.abs().max().item(), (sv, dy.abs().max().item())
    return V, dM, Wn.dual_ref(dy, 4, dyb), sv


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("B,H_,W_", TX_SHAPES)
@pytest.mark.parametrize("C", TX_C)
def test_wino_dual_bn_f16(ops, device, C, B, H_, W_, drop, kind):
    """nsm_wino_dual_bn_f16: dY1 restated in float64 from the fp32 vectors the
    kernel reads, within one bf16 rounding per element, its bound carried
    through both transforms; scale source = the finalize's dY1 bound slot."""
    V, dM, (Vr, Vb, Mr, Mb), sv = run_dual_bn(ops, device, kind, B, H_, W_, C, drop)
    cid, sp = sid(C, B, H_, W_, "drop%d" % drop, kind), kind == "spread"
    sp_check("dual_bn_v", cid, V, Vr, Vb, sv, ops.wino_beta(4, 0), sp)
    sp_check("dual_bn_dm", cid, dM, Mr, Mb, sv, ops.wino_beta(4, 1), sp)


@pytest.mark.parametrize("variant", ["slot_x8", "zero"])
def test_wino_f16_transform_slot_edges(ops, device, variant):
    """A slot holding 8x the true maximum (a coarser grid, within its own
    larger floor); an all-zero source with a zero slot: exact zeros, no NaN.
    Every transform entry, nsm_wino_dual_bn_f16 on vectors given by the test."""
    B, H_, W_, C = 2, 9, 11, 32
    kind, mul = ("zero", 1.0) if variant == "zero" else ("spread", 8.0)
    V, ref, tb, sv = run_input(ops, device, kind, B, H_, W_, C, slot_mul=mul)
    Vu, refu, tbu, _ = run_input(ops, device, kind, B, 10, 14, C, src=(5, 7), slot_mul=mul)
    dM0, Vd, dM, (Vr, Vb, Mr, Mb), sd = run_dual(ops, device, kind, B, H_, W_, C, slot_mul=mul)
    Vn, dMn, (Vnr, Vnb, Mnr, Mnb), sn = run_dual_bn(ops, device, kind, B, H_, W_, C, True, given=True,
                                                    slot_mul=mul)
    if variant == "zero":
        assert sn == 0
        for t in (V, Vu, dM0, Vd, dM):
            assert (t.view(torch.int16) == 0).all()
        # dY1 = k1 0 + k2 (y - mean) + k3 with zero coefficients is +0 or -0 by the signs of k1 and
        # y - mean: zero in value, either sign bit
        for t in (Vn, dMn):
            assert (t.float() == 0).all()
        return
    b0, b1 = ops.wino_beta(4, 0), ops.wino_beta(4, 1)
    sp_check("slot_x8", "input", V, ref, tb, sv, b0, False)
    sp_check("slot_x8", "resize", Vu, refu, tbu, sv, b0, False)
    sp_check("slot_x8", "dout", dM0, Mr, Mb, sd, b1, False)
    sp_check("slot_x8", "dual_v", Vd, Vr, Vb, sd, b0, False)
    sp_check("slot_x8", "dual_dm", dM, Mr, Mb, sd, b1, False)
    sp_check("slot_x8", "dual_bn_v", Vn, Vnr, Vnb, sn, b0, False)
    sp_check("slot_x8", "dual_bn_dm", dMn, Mnr, Mnb, sn, b1, False)


def prep_u(ops, w, n_p, k_p, flip, device):
    """prep kind 6 (single-plane f16 U [36][n_p][k_p]) through nsm_prep_weights."""
    from nsm_amd import prep
    am = ops.amax_slots(1, device)
    buf, U = guarded16(36 * n_p * k_p, device)
    j = prep.NsmPrepJob()
    j.kind = prep.KIND_WINO_F16
    for i, v in enumerate((w.shape[0], w.shape[1], n_p, k_p, int(flip), 4, 0)):
        j.a[i] = v
    j.base = 0
    j.src = w.data_ptr()
    j.dst = U.data_ptr()
    j.amax = am.data_ptr()
    prep.run_jobs([j], device)
    torch.cuda.synchronize()
    assert guard_ok(buf, 36 * n_p * k_p)
    return U, am


@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("flip", [0, 1])
def test_wino_prep_f16(ops, device, flip, spread):
    """Prep kind 6, forward and flipped (the 180 degree rotated, transposed
    filter), real channel counts below the padded ones: float64 G g G^T under
    the storage bound, exact zeros in the padding, the slot = max|w|."""
    co, ci = 100, 150
    w = Wf.make_filters(co, ci, seed=flip, spread=spread).to(device).contiguous()
    n, k = (ci, co) if flip else (co, ci)
    n_p, k_p = -(-n // 128) * 128, -(-k // 128) * 128
    U, am = prep_u(ops, w, n_p, k_p, flip, device)
    sv = Wn.slot_value(am)
    assert sv == w.abs().max().item()
    ref, tb = Wn.filter_ref(w, 4, bool(flip), n_p, k_p)
    Uv = U.view(36, n_p, k_p)
    assert (Uv[:, n:, :].view(torch.int16) == 0).all() and (Uv[:, :, k:].view(torch.int16) == 0).all()
    sp_check("prep_f16", sid(flip, int(spread)), U, ref, tb, sv, ops.wino_beta(4, 2), spread)


# ---- the batched GEMM ---------------------------------------------------------------------------
T150, T300 = (1, 60, 40), (2, 60, 40)         # T = 150, 300: ragged 256-row and 64-row tiles
TILE_OF = {1: "256x256", 2: "256x128"}


def persistent_shape(ops, ci, co):
    """The smallest (1, 156, 4 TW) whose GEMM the plan runs on the persistent
    grid (more tiles than CUs), from the plan query."""
    for tw in range(1, 200):
        if ops.wino_gemm_f16_plan(1, 156, 4 * tw, ci, co, True)[1] == "gemm_h2p":
            assert tw > 1
            return 1, 156, 4 * tw
    raise AssertionError("no persistent shape under T = 7800")


# (shape or None = persistent_shape, cin_p, cout_p, tile, form)
GEMM_CASES = [(T150, 128, 128, 2, "gemm_h2q"), (T300, 384, 128, 2, "gemm_h2q"),
              (T300, 128, 256, 1, "gemm_h2q"), (T150, 384, 256, 1, "gemm_h2q"),
              (None, 128, 256, 1, "gemm_h2p"), (None, 128, 128, 2, "gemm_h2p")]


def run_gemm(ops, device, V, U, shape, sv, su, m16, plan):
    """nsm_wino_gemm_f16 / _f16m on the test's own stored operands (rn_f16 of V,
    U times the slots' powers of two, beta 1), a NaN-filled row region behind
    V, guards behind M and the exponents. The entry's layout is packed: only
    the last component has free space behind its rows, so the NaN rows and
    the sentinel words sit behind the whole of V and of m16e; for components
    0..34 the rows past T (past ceil(T / 64)) are the next component's live
    data, and a read or write there shows only through the exponent and ratio
    assertions of both components. Returns (M [nb][T][N], exponents or None,
    V16, U16, ev, eu)."""
    nb, T, K = V.shape
    N = U.shape[1]
    B, H_, W_ = shape
    assert ops.wino_tiles(B, H_, W_, 4) == T
    assert ops.wino_gemm_f16_plan(B, H_, W_, K, N, m16) == plan
    ev, eu = Wn.h2_exp(sv, 1.0), Wn.h2_exp(su, 1.0)
    V16, U16 = Wf.sp_encode(V, ev), Wf.sp_encode(U, eu).contiguous()
    assert torch.isfinite(V16.float()).all() and torch.isfinite(U16.float()).all()
    vb = torch.full((nb * T * K + 256 * K,), NAN, dtype=torch.float16, device=device)
    vb[:nb * T * K] = V16.reshape(-1)
    av, au = slot_holding(ops, device, sv), slot_holding(ops, device, su)
    n = nb * T * N
    if m16:
        R, Q = -(-T // 64), N // 64
        buf, M = guarded16(n, device)
        me = torch.full((nb * R * Q + 64,), SENT, dtype=torch.int32, device=device)
        ops.call("nsm_wino_gemm_f16m", ops.ptr(vb), ops.ptr(U16), B, H_, W_, K, N, 4, ops.ptr(M), ops.ptr(me),
                 ops.ptr(av), 1.0, ops.ptr(au), 1.0, ops.stream())
        torch.cuda.synchronize()
        assert guard_ok(buf, n) and (me[nb * R * Q:] == SENT).all()
        return M.view(nb, T, N), me[:nb * R * Q].view(nb, R, Q), V16, U16, ev, eu
    Mb = torch.full((n + GUARD,), NAN, device=device)
    ops.call("nsm_wino_gemm_f16", ops.ptr(vb), ops.ptr(U16), B, H_, W_, K, N, 4, ops.ptr(Mb), ops.ptr(av), 1.0,
             ops.ptr(au), 1.0, ops.stream())
    torch.cuda.synchronize()
    assert torch.isnan(Mb[n:]).all()
    return Mb[:n].view(nb, T, N), None, V16, U16, ev, eu


def gemm_check(family, cid, got, et, V16, U16, ev, eu, spread):
    ref, bound = Wf.gemm_ref(V16, U16, ev, eu)
    if et is None:
        return check(family, cid, H.ratio(got, ref, bound))
    r, adm, ok = Wf.m16_ratio(got, et, ref, bound, ev, eu)
    e_lo, e_hi = Wf.m16_expect(ref, bound, ev, eu)
    print(f"{family} {cid}: tiles with two admissible exponents {(e_lo != e_hi).double().mean().item():.3f}")
    assert adm, (family, cid, "a tile exponent outside the reference's range")
    assert ok, (family, cid, "a tile's maximum outside [2^14, 2^15], or Inf")
    if spread:
        share = Wf.m16_tiny_share(ref, e_lo, ev, eu)
        assert share >= MIN_TINY, (family, cid, share)
    check(family, cid, r)


@pytest.mark.parametrize("m16", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,ci,co,t,form", GEMM_CASES)
def test_wino_gemm_f16(ops, device, shape, ci, co, t, form, kind, m16):
    """Both tiles and both kernel forms against the float64 product of the
    decoded stored operands, every component; with f16 M every tile exponent
    against the reference's tile maximum."""
    shape = shape or persistent_shape(ops, ci, co)
    T = ops.wino_tiles(*shape, 4)
    assert T % 64 != 0
    V, U = (t_.to(device) for t_ in Wf.gemm_operands(kind, 36, T, ci, co))
    sv, su = V.abs().max().item(), U.abs().max().item()
    got, et, V16, U16, ev, eu = run_gemm(ops, device, V, U, shape, sv, su, m16, (t, form))
    gemm_check("gemm_%s_%s_%s" % (TILE_OF[t], form, "m16" if m16 else "m32"),
               sid(*shape, ci, co, kind), got, et, V16, U16, ev, eu, kind == "spread")


@pytest.mark.parametrize("m16", [False, True])
@pytest.mark.parametrize("variant", ["slots_x8", "zero_u"])
@pytest.mark.parametrize("shape,ci,co,t,form", [GEMM_CASES[0], GEMM_CASES[2], GEMM_CASES[4]])
def test_wino_gemm_f16_scales(ops, device, shape, ci, co, t, form, variant, m16):
    """Slots holding 8x the maxima (three bits of the operands' f16 range
    unused) and an all-zero U: M exactly zero, e_t = 0, no NaN."""
    shape = shape or persistent_shape(ops, ci, co)
    T = ops.wino_tiles(*shape, 4)
    V, U = (t_.to(device) for t_ in Wf.gemm_operands("spread", 36, T, ci, co, seed=1))
    sv, su = V.abs().max().item(), U.abs().max().item()
    if variant == "zero_u":
        got, et, *_ = run_gemm(ops, device, V, torch.zeros_like(U), shape, sv, su, m16, (t, form))
        assert (got.float() == 0).all()
        assert et is None or (et == 0).all()
        return
    got, et, V16, U16, ev, eu = run_gemm(ops, device, V, U, shape, 8 * sv, 8 * su, m16, (t, form))
    gemm_check("gemm_slots_x8_%s" % ("m16" if m16 else "m32"), sid(*shape, ci, co), got, et, V16, U16, ev, eu,
               False)


# ---- output transforms ---------------------------------------------------------------------------------
OUT_SHAPES = [(3, 13, 22), (2, 9, 11)]         # T = 72 (two exponent row tiles, the last of 8 rows), 18
# e_t fill, e_v, e_u: -e_t - e_v = 140 (clamped to 126), -140 (to -126), 100 (not clamped)
EXTREME = {"hi": (-150, 10, 126), "lo": (130, 10, -100), "far": (-90, -10, 110)}


def out_case(device, B, H_, W_, N, extreme=None):
    """The test's own f16 M, tile exponents (different per tile and per
    component), e_v, e_u and bias."""
    T = B * Wn.tiles_hw(H_, W_, 4)[0] * Wn.tiles_hw(H_, W_, 4)[1]
    g = H.gen(T, N, 41)
    Mp = Wn.make_planes(36, T, N, seed=4)
    et = torch.randint(-20, 21, (36, -(-T // 64), N // 64), generator=g)
    ev, eu = 7, 12
    if extreme is not None:
        fill, ev, eu = EXTREME[extreme]
        et = torch.full_like(et, fill)
    bias = torch.randn(N, generator=g) * 0.1
    return Wf.sp_encode(Mp, 3).to(device), et.to(device), ev, eu, bias.to(device)


def run_output(ops, device, B, H_, W_, N, variant, extreme=None, nslot=0):
    """One output entry on the test's own M -> (y NCHW float64 as stored, ref,
    bound, partial buffer or None). variant: m32 (nsm_wino_output_bf16 on the
    decoded fp32 M), m16 (nsm_wino_output_bf16m), act (nsm_wino_output_bf16m_act)."""
    M16, et, ev, eu, bias = out_case(device, B, H_, W_, N, extreme)
    Mown = Wf.m16_decode(M16, et, ev, eu, clamp=True)
    if extreme:
        bias = bias * Mown.abs().max().float()
    g = H.gen(N, 42)
    act = None
    if variant == "act":
        act = (torch.randn(N, generator=g).to(device), torch.randn(N, generator=g).to(device), 0.2)
    ref, bound = Wf.output_ref(Mown, bias, B, H_, W_, act=act)
    ld = N + 32
    y = torch.full((B * H_ * W_, ld), NAN, dtype=torch.bfloat16, device=device)
    sv_, su_ = slot_holding(ops, device, 2.0 ** (15 - ev)), slot_holding(ops, device, 2.0 ** (15 - eu))
    assert Wn.h2_exp(2.0 ** (15 - ev), 1.0) == ev and Wn.h2_exp(2.0 ** (15 - eu), 1.0) == eu
    part = torch.full((nslot * 3 * N + GUARD,), NAN, device=device) if nslot else None
    me = et.to(torch.int32).contiguous()
    if variant == "m32":
        Mf = Mown.float().contiguous()
        assert torch.equal(Mf.double(), Mown)
        ops.call("nsm_wino_output_bf16", ops.ptr(Mf), B, H_, W_, N, 4, ops.ptr(bias), ops.ptr(y), ld,
                 ops.ptr(part), nslot, ops.stream())
    elif variant == "m16":
        ops.call("nsm_wino_output_bf16m", ops.ptr(M16), ops.ptr(me), B, H_, W_, 128, N, 4, ops.ptr(sv_), 1.0,
                 ops.ptr(su_), 1.0, ops.ptr(bias), ops.ptr(y), ld, ops.ptr(part), nslot, ops.stream())
    else:
        ops.call("nsm_wino_output_bf16m_act", ops.ptr(M16), ops.ptr(me), B, H_, W_, 128, N, 4, ops.ptr(sv_),
                 1.0, ops.ptr(su_), 1.0, ops.ptr(bias), ops.ptr(y), ld, ops.ptr(act[0]), ops.ptr(act[1]), 0.2,
                 ops.stream())
    torch.cuda.synchronize()
    assert torch.isnan(y[:, N:].float()).all()
    if part is not None:
        assert torch.isnan(part[nslot * 3 * N:]).all()
    got = y[:, :N].reshape(B, H_, W_, N).permute(0, 3, 1, 2).double()
    return got, ref, bound, part, y


def check_partials(ops, device, cid, part, got, y, nslot, N):
    """Every slot on its own (count exactly; sum and M2 against float64 sums
    over the kernel's own rounded y under fp32 operation-count bounds), then
    the merged mean and inverse deviation through bn_train(part=...), under
    the slots' bounds carried through nsm_bn_finalize_train's double merge
    (wino_f16_util.merged_ref)."""
    p = part[:nslot * 3 * N].view(nslot, 3, N)
    cnt, rs, rm = Wf.partials_ratio(p, got, nslot)
    assert cnt, (cid, "a slot's count")
    check("partial_sum", cid, rs)
    check("partial_m2", cid, rm)
    bn = torch.nn.BatchNorm2d(N).to(device)
    st = ops.bn_train(y[:, :N], bn, N, 0.1, 1e-5, part=ops.Partials(part[:nslot * 3 * N], nslot, 0))
    torch.cuda.synchronize()
    mean, mb, inv, ib = Wf.merged_ref(got, nslot, 1e-5)
    check("merged_mean", cid, H.ratio(st.mean, mean, mb))
    check("merged_invstd", cid, H.ratio(st.invstd, inv, ib))


@pytest.mark.parametrize("variant", ["m32", "m16", "act", "m32_stats", "m16_stats"])
@pytest.mark.parametrize("N", [64, 192])
@pytest.mark.parametrize("B,H_,W_", OUT_SHAPES)
def test_wino_output_bf16(ops, device, B, H_, W_, N, variant):
    """nsm_wino_output_bf16 / _bf16m / _bf16m_act of the test's own M, bias, a
    strided ldy, with and without partials, against float64 At M A + b (and
    the affine map and LeakyReLU) cropped to H x W; the columns past cout_p of
    y stay untouched."""
    T = ops.wino_tiles(B, H_, W_, 4)
    stats = variant.endswith("_stats")
    nslot = (32 if T > 32 else 16) if stats else 0
    got, ref, bound, part, y = run_output(ops, device, B, H_, W_, N, variant.split("_")[0], nslot=nslot)
    cid = sid(B, H_, W_, N)
    check("output_" + variant, cid, H.ratio(got, ref, bound))
    if stats:
        assert T % nslot != 0 and T > nslot
        check_partials(ops, device, sid(cid, variant), part, got, y, nslot, N)


@pytest.mark.parametrize("variant", ["m16", "act", "m16_stats"])
@pytest.mark.parametrize("extreme", sorted(EXTREME))
def test_wino_output_bf16m_extreme_exponents(ops, device, extreme, variant):
    """|e_t + e_v| far beyond 24. The kernels undo 2^clamp(-e_t - e_v, -126,
    126) 2^-e_u: up to the clamp the result is the true M's transform; past it
    (hi: -e_t - e_v = 140, lo: -140) the factor saturates at 2^(+-126 - e_u)
    and the result is the transform of M16 2^(+-126 - e_u), finite and without
    NaN, which is what the reference restates (m16_decode(clamp=True))."""
    B, H_, W_, N = 3, 13, 22, 64
    nslot = 32 if variant == "m16_stats" else 0
    got, ref, bound, part, y = run_output(ops, device, B, H_, W_, N, variant.split("_")[0], extreme, nslot)
    assert torch.isfinite(got).all()
    check("output_extreme_" + variant, extreme, H.ratio(got, ref, bound))
    if nslot:
        cnt, rs, rm = Wf.partials_ratio(part[:nslot * 3 * N].view(nslot, 3, N), got, nslot)
        assert cnt
        check("partial_sum", sid("extreme", extreme), rs)
        check("partial_m2", sid("extreme", extreme), rm)


# ---- the weight gradient ----------------------------------------------------------------------------------
def wg256_shape(ops, c):
    """The smallest (1, 64, 4 TW) the planner gives 256 x 256 tiles at c channels."""
    for tw in range(1, 600):
        if ops.wino_wgrad_f16_plan(1, 64, 4 * tw, c, c)[:2] == (256, 256):
            assert tw > 1 and ops.wino_wgrad_f16_plan(1, 64, 4 * (tw - 1), c, c)[:2] == (128, 128)
            return 1, 64, 4 * tw
    raise AssertionError("no 256 x 256 plan under T = 9600")


# (shape or None = wg256_shape, cin_p, cout_p, (BM, BN))
WG_CASES = [((1, 99, 96), 128, 128, (128, 128)), ((1, 99, 96), 128, 256, (128, 128)),
            ((3, 13, 22), 256, 128, (128, 128)), (None, 256, 256, (256, 256))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,ci,co,bmn", WG_CASES)
def test_wino_wgrad_f16(ops, device, shape, ci, co, bmn, kind):
    """nsm_conv3x3_wgrad_wino_f16 on the test's own stored dM and V (the stage
    alone), real channel counts below the padded ones, a workspace of exactly
    the entry's size between NaN guards, the plan read and asserted."""
    from nsm_amd._lib import lib
    B, H_, W_ = shape or wg256_shape(ops, ci)
    T = ops.wino_tiles(B, H_, W_, 4)
    BM, BN, splits, kchunk = ops.wino_wgrad_f16_plan(B, H_, W_, ci, co)
    assert (BM, BN) == bmn and (splits - 1) * kchunk < T <= splits * kchunk
    if T == 600:
        assert splits == 3 and T % kchunk != 0          # a three-way split with a short last one
    cin, cout = ci - 3, co - 5
    sp = kind == "spread"
    dM = Wn.make_planes(36, T, co, seed=7, spread=sp).to(device)
    V = Wn.make_planes(36, T, ci, seed=8, spread=sp).to(device)
    b0, b1 = ops.wino_beta(4, 0), ops.wino_beta(4, 1)
    sdy, sx = dM.abs().max().item() / b1, V.abs().max().item() / b0
    ed, ev = Wn.h2_exp(sdy, b1), Wn.h2_exp(sx, b0)
    dM16, V16 = Wf.sp_encode(dM, ed).contiguous(), Wf.sp_encode(V, ev).contiguous()
    assert torch.isfinite(dM16.float()).all() and torch.isfinite(V16.float()).all()
    ady, ax = slot_holding(ops, device, sdy), slot_holding(ops, device, sx)
    n = int(lib.nsm_wino_wgrad_f16_ws(B, H_, W_, ci, co, 4))
    assert n == 36 * splits * co * ci + (36 * co * ci if splits > 1 else 0)
    buf = torch.full((n + 2 * 1024,), NAN, device=device)
    ws = buf[1024:1024 + n]
    dwb = torch.full((cout * cin * 9 + 1024,), NAN, device=device)
    ops.call("nsm_conv3x3_wgrad_wino_f16", ops.ptr(dM16), ops.ptr(V16), B, H_, W_, ci, co, cin, cout, 4,
             ops.ptr(dwb), ops.ptr(ws), n, ops.ptr(ady), ops.ptr(ax), ops.stream())
    torch.cuda.synchronize()
    assert torch.isnan(buf[:1024]).all() and torch.isnan(buf[1024 + n:]).all()
    assert torch.isnan(dwb[cout * cin * 9:]).all()
    ref, bound = Wf.wgrad_ref(dM16, V16, ed, ev, cout, cin)
    check("wgrad_%dx%d" % (BM, BN), sid(B, H_, W_, ci, co, kind, "s%d" % splits, "k%d" % kchunk),
          H.ratio(dwb[:cout * cin * 9].view(cout, cin, 3, 3), ref, bound))


# ---- one chained convolution per forward tile ---------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ci,co,t", [(128, 128, 2), (128, 256, 1)])
def test_wino_f16_chain(ops, device, ci, co, t, kind):
    """conv3x3_wino_f16 (f16 M) forward and the input gradient through the
    flipped filters as unet.py calls them, at (2, 37, 53), against float64
    conv2d / autograd of the bf16 operands. The bound is the sum of the stage
    bounds, each carried through the absolute values of the later stages."""
    B, H_, W_ = 2, 37, 53
    sp = kind == "spread"
    x = Wf.make_x(kind, B, H_, W_, ci, seed=6).to(device)
    dy = Wf.make_x(kind, B, H_, W_, co, seed=7).to(device)
    w = Wf.make_filters(co, ci, seed=8, spread=sp, lo=-12).to(device).contiguous()
    bias = (torch.randn(co, generator=H.gen(9)) * 0.1).to(device)
    assert ops.wino_gemm_f16_plan(B, H_, W_, ci, co, True)[0] == t
    xr, dyr = rows16(x), rows16(dy)
    ax, ady = ops.absmax(xr), ops.absmax(dyr)
    U, au = prep_u(ops, w, co, ci, 0, device)
    Ud, aud = prep_u(ops, w, ci, co, 1, device)
    y, _ = ops.conv3x3_wino_f16(xr, B, H_, W_, U, bias, co, amax=(ax, au), stats=False, m16=True)
    Vd, _ = ops.wino_dual_f16(dyr, B, H_, W_, ady)
    dx, _ = ops.conv3x3_wino_f16(dyr, B, H_, W_, Ud, None, ci, amax=(ady, aud), stats=False, m16=True, v_in=Vd)
    torch.cuda.synchronize()
    x64, w64 = x.double().requires_grad_(True), w.double()
    yref = F.conv2d(x64, w64, bias.double(), padding=1)
    yref.backward(dy.double())
    sx, sdy, sw = (Wn.slot_value(s) for s in (ax, ady, au))
    assert Wn.slot_value(aud) == sw
    b0, b2 = ops.wino_beta(4, 0), ops.wino_beta(4, 2)
    img = lambda t_, c: t_.reshape(B, H_, W_, c).permute(0, 3, 1, 2)  # noqa: E731
    for name, src, s_src, flip, n_, k_, bb, got, want in (
            ("chain_fwd", x, sx, False, co, ci, bias, img(y, co), yref.detach()),
            ("chain_dgrad", dy, sdy, True, ci, co, None, img(dx, ci), x64.grad)):
        Vr, tb = Wf.input_ref(src)
        eV = Wf.sp_bound(Vr, tb, s_src, b0)
        Ur, ub = Wn.filter_ref(w, 4, flip, n_, k_)
        eU = Wf.sp_bound(Ur, ub, sw, b2)
        Mr, eM = Wf.chain_gemm(Vr, eV, Ur, eU, Wn.h2_exp(s_src, b0), Wn.h2_exp(sw, b2), True)
        _, yb = Wf.chain_output(Mr, eM, bb, B, H_, W_)
        check(name, sid(ci, co, kind), H.ratio(got, want, yb))


# ---- the generic kernel forms ----------------------------------------------------------------------------------
CHILD_ENV = {"NSM_F16_UP_BUF": "0", "NSM_F16_TX_CW": "4", "NSM_F16_OUT_CW": "2"}


def _digest(t):
    return hashlib.sha256(t.contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()


def form_cases(ops, device):
    """{case: [worst err / bound, sha256 of the output bytes]} of the entries
    whose kernel form depends on NSM_F16_UP_BUF / NSM_F16_TX_CW / NSM_F16_OUT_CW,
    on ragged shapes."""
    out = {}
    b0, b1 = ops.wino_beta(4, 0), ops.wino_beta(4, 1)
    B, H_, W_, C = 3, 13, 22, 32
    V, ref, tb, sv = run_input(ops, device, "spread", B, H_, W_, C)
    out["input"] = [Wf.sp_ratio(V, ref, tb, sv, b0), _digest(V)]
    V, ref, tb, sv = run_input(ops, device, "spread", 2, 11, 13, 128, src=(6, 7))
    out["resize"] = [Wf.sp_ratio(V, ref, tb, sv, b0), _digest(V)]
    dM0, V, dM, (Vr, Vb, Mr, Mb), sv = run_dual(ops, device, "spread", B, H_, W_, C)
    out["dout"] = [Wf.sp_ratio(dM0, Mr, Mb, sv, b1), _digest(dM0)]
    out["dual_v"] = [Wf.sp_ratio(V, Vr, Vb, sv, b0), _digest(V)]
    out["dual_dm"] = [Wf.sp_ratio(dM, Mr, Mb, sv, b1), _digest(dM)]
    for drop in (False, True):
        V, dM, (Vr, Vb, Mr, Mb), sv = run_dual_bn(ops, device, "spread", B, H_, W_, C, drop)
        out["dual_bn_v%d" % drop] = [Wf.sp_ratio(V, Vr, Vb, sv, b0), _digest(V)]
        out["dual_bn_dm%d" % drop] = [Wf.sp_ratio(dM, Mr, Mb, sv, b1), _digest(dM)]
    for variant, nslot in (("m16", 0), ("m16", 32), ("act", 0)):
        for N in (64, 192):
            got, ref, bound, part, y = run_output(ops, device, B, H_, W_, N, variant, nslot=nslot)
            key = "output_%s_%d_%d" % (variant, N, nslot)
            out[key] = [H.ratio(got, ref, bound), _digest(y[:, :N])]
            if nslot:
                p = part[:nslot * 3 * N]
                cnt, rs, rm = Wf.partials_ratio(p.view(nslot, 3, N), got, nslot)
                out[key + "_part"] = [max(rs, rm) if cnt else float("inf"),
                                      _digest(p.view(torch.int16))]
    return out


def test_wino_f16_generic_forms(ops, device, tmp_path):
    """The generic kernels (wino_input_f16_up_kernel, wino_dual_bn_f16_kernel,
    the wino_output_kernel<M16> training form, the 4- and 2-channel widths)
    run only with NSM_F16_UP_BUF=0 / NSM_F16_TX_CW=4 / NSM_F16_OUT_CW=2, read
    once per process: one fresh child runs the transform and output cases with
    them set. It must meet the same bounds and write the default forms' bits."""
    here = form_cases(ops, device)
    for k, (r, _) in here.items():
        check("forms_default", k, r)
    out = tmp_path / "child.json"
    env = dict(os.environ)
    env.update(CHILD_ENV)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, timeout=240,
                       capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    there = json.loads(out.read_text())
    assert sorted(there) == sorted(here)
    for k, (r, _) in there.items():
        check("forms_generic", k, r)
    diff = [k for k in here if here[k][1] != there[k][1]]
    assert not diff, ("bits differ from the default forms", diff)


if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "pcss-unet_amd")):
        if _p not in sys.path:
            sys.path.insert(0, _p)
    assert all(os.environ.get(k) == v for k, v in CHILD_ENV.items())
    from nsm_amd import ops as _ops
    _res = form_cases(_ops, torch.device("cuda:0"))
    with open(sys.argv[1], "w") as _f:
        json.dump(_res, _f)
