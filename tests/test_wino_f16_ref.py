"""CPU: the bounds of tests/wino_f16_util.py bite. A numpy / torch stand-in
that follows the operation sequence of the bf16 step's F(4x4) kernels (the
fp32 two-pass transforms, the single-plane f16 store, the two same-plane
products of an SP k-step, the per-tile O16 epilogue, the output undo, the
Chan-merged BN partials, fp32 slab sums) meets every bound on calibrated and
spread inputs at the ragged shapes of test_gpu_wino_f16_ops.py (fewer
channels), each mutant of it fails at least one, and the spread inputs put at
least 10 % of their non-zero reference values under the f16 floor."""
import numpy as np
import pytest
import torch

import f16_util as H
import f32_util as S
import wino_f16_util as Wf
import wino_util as Wn

KINDS = ["calib", "spread"]
SHAPES = [(2, 9, 11), (1, 6, 7)]
C = 16
MIN_TINY = 0.10
B0, B1, B2 = (float(Wn.beta_exact(4, i)) for i in range(3))


def _amax(t):
    return float(t.abs().max())


def _ok(r, what):
    assert r <= 1, f"{what}: worst err / bound {r:.3f}"


# ---- transforms and the single-plane store ----------------------------------------------
def stand_input(x, clamp_fill=False, shift_last=False):
    """fp32 V planes of NCHW x. Mutants: clamp_fill (the patch outside the
    image holds the clamped pixel), shift_last (the last tile column's origin
    one pixel to the right)."""
    p = Wn.patches(x, 4)
    B, Cc, H_, W_ = x.shape
    TH, TW = Wn.tiles_hw(H_, W_, 4)
    if clamp_fill:
        xp = torch.nn.functional.pad(x, (1, TW * 4 + 1 - W_, 1, TH * 4 + 1 - H_), mode="replicate")
        p = xp.unfold(2, 6, 4).unfold(3, 6, 4)
    if shift_last:
        xs = torch.nn.functional.pad(x[..., 1:], (0, 1))
        p = p.clone()
        p[:, :, :, -1] = Wn.patches(xs, 4)[:, :, :, -1]
    return Wn.emu_transform(p, 4, "Bt")


def _v_ratio(kind, shape, pure=False, beta_store=None, **mut):
    """The input transform + store on the stand-in. pure: the store alone
    (ref = the fp32 values). beta_store: the producer's beta (mutant)."""
    tmut = {k: mut.pop(k) for k in ("clamp_fill", "shift_last") if k in mut}
    x = Wf.make_x(kind, *shape, C)
    ref, tb = Wf.input_ref(x)
    v = stand_input(x, **tmut)
    if pure:
        ref, tb = v.double(), torch.zeros_like(ref)
    slot = _amax(x)
    t = Wf.emu_sp(v.reshape(-1, C), slot, B0 if beta_store is None else beta_store, **mut)
    return Wf.sp_ratio(t, ref.reshape(-1, C), tb.reshape(-1, C), slot, B0), Wf.sp_tiny_share(ref, slot, B0)


def _dm_ratio(kind, shape, beta_store=None, **mut):
    dy = Wf.make_x(kind, *shape, C, seed=1)
    ref, tb = Wn.dm_ref(dy, 4)
    v = Wn.emu_transform(Wn.inner(Wn.patches(dy, 4)), 4, "A")
    slot = _amax(dy)
    t = Wf.emu_sp(v.reshape(-1, C), slot, B1 if beta_store is None else beta_store, **mut)
    return Wf.sp_ratio(t, ref.reshape(-1, C), tb.reshape(-1, C), slot, B1), Wf.sp_tiny_share(ref, slot, B1)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_standin_transforms(kind, shape):
    for name, (r, share) in (("input", _v_ratio(kind, shape)), ("store", _v_ratio(kind, shape, pure=True)),
                             ("dout", _dm_ratio(kind, shape))):
        _ok(r, f"{name} {kind} {shape}")
        if kind == "spread":
            assert share >= MIN_TINY, (name, shape, share)


@pytest.mark.parametrize("hi,wi", [(5, 7), (4, 6)])
def test_standin_resize(hi, wi):
    """Odd and even upsampled extents: the fp32 interpolation (the float64
    resample rounded to fp32) rounded to bf16, then transformed and stored."""
    x = Wf.make_x("spread", 2, hi, wi, C, seed=2)
    mats = H.resize_mats(hi, wi, 2 * hi - (hi % 2), 2 * wi - (wi % 2))
    ref, tb = Wf.input_ref(x, src=mats)
    d = Wf.bf(H.resample(x, *mats).float())
    slot = _amax(x)
    t = Wf.emu_sp(stand_input(d).reshape(-1, C), slot, B0)
    _ok(Wf.sp_ratio(t, ref.reshape(-1, C), tb.reshape(-1, C), slot, B0), "resize")
    assert Wf.sp_tiny_share(ref, slot, B0) >= MIN_TINY


def _bn_case(drop, seed=3):
    B, H_, W_ = 2, 9, 11
    g = H.gen(seed, int(drop))
    y = Wf.bf(torch.randn(B, C, H_, W_, generator=g) * 2 + 0.5)
    gr = Wf.make_spread(B, H_, W_, C, seed=seed)
    mask = ((torch.rand(B, C, generator=g) > 0.2).float() / 0.8) if drop else None
    scale, shift = torch.randn(C, generator=g), torch.rand(C, generator=g) * 0.4 - 0.2
    mean = torch.randn(C, generator=g) * 0.5
    cm = gr.abs().amax((0, 2, 3))          # the sums behind k2, k3 scale with the channel's gradient
    coef = torch.stack((torch.randn(C, generator=g), torch.randn(C, generator=g) * cm * 1e-2,
                        torch.randn(C, generator=g) * cm * 1e-2))
    return gr, y, scale, shift, mean, coef, mask


@pytest.mark.parametrize("drop", [False, True])
def test_standin_dual_bn(drop):
    """dY1 formed in fp32 per element, rounded to bf16, both transforms."""
    gr, y, scale, shift, mean, coef, mask = _bn_case(drop)
    v = (1, -1, 1, 1)
    z = y * scale.view(v) + shift.view(v)
    dz = gr * torch.where(z > 0, torch.ones(()), torch.full((), 0.2))
    if mask is not None:
        dz = dz * mask[:, :, None, None]
    d = Wf.bf(coef[0].view(v) * dz + coef[1].view(v) * (y - mean.view(v)) + coef[2].view(v))
    dy, dyb = Wf.bn_dy_ref(gr, y, scale, shift, mean, coef, mask)
    Vr, Vb, Mr, Mb = Wn.dual_ref(dy, 4, dyb)
    slot = float((dy.abs() + dyb).max())
    tv = Wf.emu_sp(stand_input(d).reshape(-1, C), slot, B0)
    tm = Wf.emu_sp(Wn.emu_transform(Wn.inner(Wn.patches(d, 4)), 4, "A").reshape(-1, C), slot, B1)
    _ok(Wf.sp_ratio(tv, Vr.reshape(-1, C), Vb.reshape(-1, C), slot, B0), "dual_bn V")
    _ok(Wf.sp_ratio(tm, Mr.reshape(-1, C), Mb.reshape(-1, C), slot, B1), "dual_bn dM")
    assert Wf.sp_tiny_share(Vr, slot, B0) >= MIN_TINY and Wf.sp_tiny_share(Mr, slot, B1) >= MIN_TINY


def _filter_ratio(spread, flip):
    w = Wf.make_filters(5, 7, spread=spread)
    ref, tb = Wn.filter_ref(w, 4, flip, 8, 8)
    g = w.flip(2, 3).transpose(0, 1) if flip else w
    n, k = g.shape[:2]
    u = torch.from_numpy(Wn.emu_wmat2(Wn.cmat32(4, "G"), g.contiguous().numpy())).permute(2, 3, 0, 1)
    U = torch.zeros(36, 8, 8)
    U[:, :n, :k] = u.reshape(36, n, k)
    slot = _amax(w)
    t = Wf.emu_sp(U.reshape(-1, 8), slot, B2)
    return Wf.sp_ratio(t, ref.reshape(-1, 8), tb.reshape(-1, 8), slot, B2), Wf.sp_tiny_share(ref, slot, B2)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("spread", [False, True])
def test_standin_filters(spread, flip):
    r, share = _filter_ratio(spread, flip)
    _ok(r, "prep kind 6")
    if spread:
        assert share >= MIN_TINY, share


# ---- GEMM, fp32 and f16 M ------------------------------------------------------------------------
NBG, TG, KG, NG = 3, 150, 128, 128     # 3 row tiles (the last 22 rows), 2 column tiles, 2 K-tiles


def _gemm_case(kind, scale=1.0):
    """Stored operands of a GEMM whose exponent tiles differ along rows,
    columns and components (row tile r times 2^-2r, column tile q times 2^-3q
    on top of the per-component magnitudes)."""
    V, U = Wf.gemm_operands(kind, NBG, TG, KG, NG)
    V = V * torch.pow(2.0, -2.0 * (torch.arange(TG) // 64)).view(1, TG, 1)
    U = U * torch.pow(2.0, -3.0 * (torch.arange(NG) // 64)).view(1, NG, 1)
    ev, eu = Wn.h2_exp(_amax(V) * scale, 1.0), Wn.h2_exp(_amax(U) * scale, 1.0)
    return Wf.sp_encode(V, ev), Wf.sp_encode(U, eu), ev, eu


def _acc(V16, U16, **mut):
    return torch.stack([Wf.emu_gemm_sp(V16[c], U16[c], **mut) for c in range(V16.shape[0])])


def _gemm32_ratio(kind, scale=1.0, no_eu=False, **mut):
    V16, U16, ev, eu = _gemm_case(kind, scale)
    ref, bound = Wf.gemm_ref(V16, U16, ev, eu)
    got = (_acc(V16, U16, **mut).double() * 2.0 ** -ev) * (1.0 if no_eu else 2.0 ** -eu)
    return H.ratio(got.float(), ref, bound)


def _gemm16(kind, scale=1.0, roll=None, no_eu=False, static=False, gmut=None, **mut):
    """(ratio, admissible, tiles ok, tiny share) of the f16 M. roll = axis:
    the decode reads the exponent of the neighbouring component (0), row tile
    (1) or column tile (2)."""
    V16, U16, ev, eu = _gemm_case(kind, scale)
    ref, bound = Wf.gemm_ref(V16, U16, ev, eu)
    M16, et = Wf.emu_o16(_acc(V16, U16, **(gmut or {})), static_k=KG if static else 0, **mut)
    if roll is not None:
        assert (et != torch.roll(et, 1, roll)).any()
        et = torch.roll(et, 1, roll)
    r, adm, ok = Wf.m16_ratio(M16, et, ref, bound, ev, 0 if no_eu else eu)
    if no_eu:      # the undo without 2^-e_u against the true reference
        e_lo, _ = Wf.m16_expect(ref, bound, ev, eu)
        r = H.ratio(Wf.m16_decode(M16, et, ev, 0), ref, Wf.m16_bound(ref, bound, e_lo, ev, eu))
    e_lo, _ = Wf.m16_expect(ref, bound, ev, eu)
    return r, adm, ok, Wf.m16_tiny_share(ref, e_lo, ev, eu)


@pytest.mark.parametrize("scale", [1.0, 8.0])
@pytest.mark.parametrize("kind", KINDS)
def test_standin_gemm(kind, scale):
    _ok(_gemm32_ratio(kind, scale), "gemm fp32 M")
    r, adm, ok, share = _gemm16(kind, scale)
    _ok(r, "gemm f16 M")
    assert adm and ok
    if kind == "spread":
        assert share >= MIN_TINY, share


def test_standin_gemm_zero_u():
    V16, U16, ev, eu = _gemm_case("calib")
    M16, et = Wf.emu_o16(_acc(V16, torch.zeros_like(U16)))
    assert (M16 == 0).all() and (et == 0).all() and Wf.m16_tiles_ok(M16, et)


# ---- output transform ---------------------------------------------------------------------------------
OUT = (3, 13, 22)     # T = 72: two 64-row exponent tiles, the last 8 rows
NO = 64
NSLOT = 32            # slots 0..7 take three tiles, the others two


def _out_case(extreme=None):
    B, H_, W_ = OUT
    TH, TW = Wn.tiles_hw(H_, W_, 4)
    T = B * TH * TW
    g = H.gen(T, NO, 41)
    Mp = Wn.make_planes(36, T, NO, seed=4)
    et = torch.randint(-20, 21, (36, -(-T // 64), NO // 64), generator=g)
    ev, eu = 7, 12
    if extreme == "hi":        # -e_t - e_v = 140 -> 126
        et, ev, eu = torch.full_like(et, -150), 10, 126
    elif extreme == "lo":      # -e_t - e_v = -140 -> -126
        et, ev, eu = torch.full_like(et, 130), 10, -100
    elif extreme == "far":     # |e_t + e_v| = 100, not clamped
        et, ev, eu = torch.full_like(et, -90), -10, 110
    bias = torch.randn(NO, generator=g) * 0.1
    M16 = Wf.sp_encode(Mp, 3)            # values around 2^3: what the f16 M holds is the test's choice
    return M16, et, ev, eu, bias


def _out_ratio(extreme=None, act=False, **mut):
    B, H_, W_ = OUT
    M16, et, ev, eu, bias = _out_case(extreme)
    Mown = Wf.m16_decode(M16, et, ev, eu, clamp=True)
    a = (torch.randn(NO, generator=H.gen(5)), torch.randn(NO, generator=H.gen(6)), 0.2) if act else None
    if extreme:
        bias = bias * float(Mown.abs().max())
    ref, bound = Wf.output_ref(Mown, bias, B, H_, W_, act=a)
    y, _ = Wf.emu_output(Mown.float(), bias, B, H_, W_, act=a, **mut)
    return H.ratio(y, ref, bound)


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("extreme", [None, "hi", "lo", "far"])
def test_standin_output(extreme, act):
    _ok(_out_ratio(extreme, act), f"output {extreme} act {act}")


def test_clamp_changes_the_value():
    """Past the clamp the undo is 2^(+-126 - e_u), not 2^-(e_t + e_v + e_u)."""
    M16, et, ev, eu, _ = _out_case("hi")
    a, b = Wf.m16_decode(M16, et, ev, eu, clamp=True), Wf.m16_decode(M16, et, ev, eu)
    assert torch.equal(a * 2.0 ** 14, b) and torch.equal(a, M16.double())


def _part_ratio(unrounded=False):
    B, H_, W_ = OUT
    M16, et, ev, eu, bias = _out_case()
    y, raw = Wf.emu_output(Wf.m16_decode(M16, et, ev, eu).float(), bias, B, H_, W_)
    return Wf.partials_ratio(Wf.emu_partials(raw if unrounded else y, NSLOT), y, NSLOT)


def test_standin_partials():
    cnt, rs, rm = _part_ratio()
    assert cnt
    _ok(rs, "partial sums")
    _ok(rm, "partial M2")


def test_standin_merged_statistics():
    """nsm_bn_finalize_train's merge of the stand-in's partials (double, then
    fp32 mean, variance and 1 / sqrtf(var + eps)) within merged_ref's bounds."""
    B, H_, W_ = OUT
    M16, et, ev, eu, bias = _out_case()
    y, _ = Wf.emu_output(Wf.m16_decode(M16, et, ev, eu).float(), bias, B, H_, W_)
    p = Wf.emu_partials(y, NSLOT).double().numpy()
    Mn = B * H_ * W_
    mean = p[:, 0].sum(0) / Mn
    on = p[:, 2] > 0
    d = np.where(on, p[:, 0] / np.maximum(p[:, 2], 1) - mean, 0.0)
    m2 = (np.where(on, p[:, 1], 0.0) + p[:, 2] * d * d).sum(0)
    var_b = np.float32(m2 / Mn)
    inv = np.float32(1.0) / np.sqrt(var_b + np.float32(1e-5), dtype=np.float32)
    rm, mb, ri, ib = Wf.merged_ref(y, NSLOT, 1e-5)
    _ok(H.ratio(torch.from_numpy(mean.astype(np.float32)), rm, mb), "merged mean")
    _ok(H.ratio(torch.from_numpy(inv), ri, ib), "merged 1/sigma")


# ---- weight gradient -------------------------------------------------------------------------------------
def _wgrad_ratio(kind, splits=3, **mut):
    T, co, ci = 70, 5, 7
    dM = Wn.make_planes(36, T, 8, seed=7, spread=kind == "spread")
    V = Wn.make_planes(36, T, 8, seed=8, spread=kind == "spread")
    ed, ev = Wn.h2_exp(_amax(dM), 1.0), Wn.h2_exp(_amax(V), 1.0)
    dM16, V16 = Wf.sp_encode(dM, ed), Wf.sp_encode(V, ev)
    ref, bound = Wf.wgrad_ref(dM16, V16, ed, ev, co, ci)
    dU = Wn.emu_split_sum((dM16.double() * 2.0 ** -ed).float(), (V16.double() * 2.0 ** -ev).float(), splits, **mut)
    u = dU[:, :co, :ci].reshape(6, 6, co, ci).permute(2, 3, 0, 1).contiguous().numpy()
    return H.ratio(torch.from_numpy(Wn.emu_wmat2(Wn.cmat32(4, "Gt"), u)), ref, bound)


@pytest.mark.parametrize("kind", KINDS)
def test_standin_wgrad(kind):
    _ok(_wgrad_ratio(kind), "wgrad")


# ---- the mutants ---------------------------------------------------------------------------------------------
S0 = SHAPES[0]
MUTANTS = {
    "f16_store_truncated": lambda: _v_ratio("calib", S0, pure=True, trunc=True)[0],
    "f16_subnormals_flushed": lambda: _v_ratio("spread", S0, pure=True, flush=True)[0],
    "exponent_plus_one": lambda: _v_ratio("calib", S0, exp_off=1)[0],
    "exponent_minus_one": lambda: _v_ratio("calib", S0, exp_off=-1)[0],
    "beta_of_input_for_dout": lambda: _dm_ratio("calib", S0, beta_store=B0)[0],
    "static_m16_exponent": lambda: _gemm16("spread", static=True)[0],
    "exponent_of_next_row_tile": lambda: _gemm16("calib", roll=1)[0],
    "exponent_of_next_column_tile": lambda: _gemm16("calib", roll=2)[0],
    "exponent_of_next_component": lambda: _gemm16("calib", roll=0)[0],
    "e_u_not_undone": lambda: _gemm16("calib", no_eu=True)[0],
    "half_chunk_dropped": lambda: _gemm32_ratio("calib", drop_half=True),
    "half_chunk_dropped_m16": lambda: _gemm16("calib", gmut={"drop_half": True})[0],
    "halves_cross_paired": lambda: _gemm32_ratio("calib", cross=True),
    "m16_store_truncated": lambda: _gemm16("calib", trunc=True)[0],
    "m16_subnormals_flushed": lambda: _gemm16("spread", flush=True)[0],
    "last_k_split_dropped": lambda: _wgrad_ratio("calib", drop_last=True),
    "edge_clamped": lambda: _v_ratio("calib", S0, clamp_fill=True)[0],
    "last_tile_shifted": lambda: _v_ratio("calib", S0, shift_last=True)[0],
    "chunks_swapped": lambda: _v_ratio("calib", S0, swap_chunks=True)[0],
    "bias_dropped": lambda: _out_ratio(drop_bias=True),
    "bf16_store_truncated": lambda: _out_ratio(trunc=True),
    "partials_of_unrounded_y": lambda: max(_part_ratio(unrounded=True)[1:]),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_fails_a_bound(name):
    r = MUTANTS[name]()
    assert r > 1, (name, r)


def test_e_u_is_not_zero_in_the_gemm_case():
    """(the e_u mutant would pass trivially otherwise)"""
    assert _gemm_case("calib")[3] != 0


def test_exp_of_matches_the_scalar_mirror():
    v = torch.tensor([0.0, 1.0, 1.5, 2.0, 2.0 ** 15, 2.0 ** 15 + 1, 3e-39, 1e38, float("inf")])
    assert Wf.exp_of(v).tolist() == [Wn.h2_exp(float(np.float32(x)), 1.0) for x in v.tolist()]
