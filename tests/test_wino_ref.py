"""CPU: the bounds of tests/wino_util.py bite. A numpy stand-in that follows
the kernels' operation sequence (wmat2 with fp32 roundings, the h2 split, the
three-product f16 GEMM, fp32 slab sums) passes every bound on the cases of
test_gpu_wino_f32_ops.py (at their ragged shapes, fewer channels), and each of
twelve mutants of it fails at least one. Also the host check that
nsm_wino_beta bounds its exact transform."""
import numpy as np
import pytest
import torch

import f16_util as H
import wino_util as Wn

SHAPES = [(2, 9, 11), (1, 13, 7)]
C = 16


def _x(kind, B, H_, W_, seed=0):
    return (Wn.make_spread if kind == "spread" else Wn.make_calib)(B, H_, W_, C, seed)


def _amax(t):
    return float(t.abs().max())


# ---- the stand-in stages --------------------------------------------------------------
def stand_input(x, tile, C32=None, clamp_fill=False, shift_last=False):
    """fp32 V planes of NCHW x. Mutants: clamp_fill (the patch outside the
    image holds the clamped pixel), shift_last (the last tile column's origin
    one pixel to the right)."""
    p = Wn.patches(x, tile)
    if clamp_fill:
        B, Cc, H_, W_ = x.shape
        TH, TW = Wn.tiles_hw(H_, W_, tile)
        xp = torch.nn.functional.pad(x, (1, TW * tile + 1 - W_, 1, TH * tile + 1 - H_), mode="replicate")
        p = xp.unfold(2, tile + 2, tile).unfold(3, tile + 2, tile)
    if shift_last:
        B, Cc, H_, W_ = x.shape
        xs = torch.nn.functional.pad(x[..., 1:], (0, 1))
        p = p.clone()
        p[:, :, :, -1] = Wn.patches(xs, tile)[:, :, :, -1]
    return Wn.emu_transform(p, tile, "Bt", C32)


def _input_ratio(kind, shape, tile, **mut):
    x = _x(kind, *shape)
    ref, bound, _ = Wn.input_ref(x, tile)
    return H.ratio(stand_input(x, tile, **mut), ref, bound)


@pytest.mark.parametrize("tile", Wn.TILES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["calib", "spread"])
def test_standin_transforms_within_bounds(kind, shape, tile):
    """Bt, A, At of the three tiles on the stand-in: every ratio <= 1."""
    B, H_, W_ = shape
    assert _input_ratio(kind, shape, tile) <= 1
    dy = _x(kind, B, H_, W_, seed=1)
    ref, bound = Wn.dm_ref(dy, tile)
    assert H.ratio(Wn.emu_transform(Wn.inner(Wn.patches(dy, tile)), tile, "A"), ref, bound) <= 1
    TH, TW = Wn.tiles_hw(H_, W_, tile)
    Mp = Wn.make_planes((tile + 2) ** 2, B * TH * TW, C, seed=2, spread=kind == "spread")
    bias = torch.randn(C, generator=H.gen(3)) * 0.1
    assert _output_ratio(Mp, bias, B, H_, W_, tile) <= 1


def stand_output(Mp, bias, B, H_, W_, tile, drop_bias=False):
    TH, TW = Wn.tiles_hw(H_, W_, tile)
    X = Wn.from_planes(Mp, B, TH, TW).contiguous().numpy().astype(np.float32)
    o = torch.from_numpy(Wn.emu_wmat2(Wn.cmat32(tile, "At"), X))
    y = o.permute(0, 1, 2, 4, 3, 5).reshape(B, -1, TH * tile, TW * tile)[:, :, :H_, :W_]
    return y if drop_bias else y + bias.view(1, -1, 1, 1)


def _output_ratio(Mp, bias, B, H_, W_, tile, **mut):
    ref, bound = Wn.output_ref(Mp, bias, B, H_, W_, tile)
    return H.ratio(stand_output(Mp, bias, B, H_, W_, tile, **mut), ref, bound)


def test_standin_upsampled_input():
    """The resampled source: the stand-in rounds the float64 resample to fp32."""
    B, hi, wi = 2, 5, 7
    x = _x("spread", B, hi, wi)
    for tile in (4, 6):
        mats = H.resize_mats(hi, wi, 2 * hi, 2 * wi)
        ref, bound, xr = Wn.input_ref(x, tile, src=mats)
        assert H.ratio(stand_input(xr.float(), tile), ref, bound) <= 1


@pytest.mark.parametrize("tile", Wn.TILES)
def test_standin_filters(tile):
    w = Wn.make_filters(5, 7)
    for flip in (False, True):
        n, k = (7, 5) if flip else (5, 7)
        ref, bound = Wn.filter_ref(w, tile, flip, 8, 8)
        assert H.ratio(_stand_filter(w, tile, flip), ref[:, :n, :k], bound[:, :n, :k]) <= 1


def _stand_filter(w, tile, flip, C32=None):
    g = w.flip(2, 3).transpose(0, 1) if flip else w
    n, k = g.shape[:2]
    u = Wn.emu_wmat2(Wn.cmat32(tile, "G") if C32 is None else C32, g.contiguous().numpy())
    return torch.from_numpy(u).permute(2, 3, 0, 1).reshape(-1, n, k)


# ---- h2 storage, GEMM, weight gradient ---------------------------------------------------
def _h2_case(kind, tile):
    x = _x(kind, 2, 9, 11)
    ref, tb, _ = Wn.input_ref(x, tile)
    v = stand_input(x, tile)
    return x, ref.reshape(-1, C), tb.reshape(-1, C), v.reshape(-1, C)


def _h2_ratio(kind, tile, pure=False, **mut):
    """pure: the storage step alone (nsm_to_h2 of given fp32 values: ref = v)."""
    x, ref, tb, v = _h2_case(kind, tile)
    if pure:
        ref, tb = v.double(), 0.0
    slot, beta = _amax(x), float(Wn.beta_exact(tile, 0))
    r = Wn.h2_ratio(Wn.emu_h2(v, slot, beta, **mut), ref, tb, slot, beta)
    return r, Wn.tiny_share(ref, Wn.h2_P(slot, beta))


@pytest.mark.parametrize("tile", [4, 6])
@pytest.mark.parametrize("kind", ["calib", "spread"])
def test_standin_h2_storage(kind, tile):
    r, share = _h2_ratio(kind, tile)
    assert r <= 1
    assert _h2_ratio(kind, tile, pure=True)[0] <= 1
    if kind == "spread":
        assert share >= 0.10, share


def _gemm_case(kind, T=37, K=32, N=32, nb=4, scale=1.0):
    V = Wn.make_planes(nb, T, K, seed=5, spread=kind == "spread")
    U = Wn.make_planes(nb, N, K, seed=6, spread=kind == "spread", lo=-6, hi=-4)
    return V, U, _amax(V) * scale, _amax(U) * scale


def _gemm_ratio(kind, scale=1.0, **mut):
    V, U, mv, mu = _gemm_case(kind, scale=scale)
    nb, T, K = V.shape
    ref, bound = Wn.gemm_ref(V, U, mv, mu)
    ev, eu = Wn.h2_exp(mv, 1.0), Wn.h2_exp(mu, 1.0)
    got = torch.stack([Wn.emu_gemm_h2(Wn.emu_h2(V[c], mv, 1.0), Wn.emu_h2(U[c], mu, 1.0), K, ev, eu, **mut)
                       for c in range(nb)])
    return H.ratio(got, ref, bound)


@pytest.mark.parametrize("kind", ["calib", "spread"])
@pytest.mark.parametrize("scale", [1.0, 8.0])
def test_standin_gemm(kind, scale):
    assert _gemm_ratio(kind, scale) <= 1


def _wgrad_ratio(kind, tile=4, splits=3, **mut):
    nb, T, co, ci = (tile + 2) ** 2, 70, 5, 7
    dM = Wn.make_planes(nb, T, 8, seed=7, spread=kind == "spread")
    V = Wn.make_planes(nb, T, 8, seed=8, spread=kind == "spread")
    ref, bound = Wn.wgrad_ref(dM, V, tile, co, ci, _amax(dM), _amax(V))
    dU = Wn.emu_split_sum(dM, V, splits, **mut)
    a = tile + 2
    u = dU[:, :co, :ci].reshape(a, a, co, ci).permute(2, 3, 0, 1).contiguous().numpy()
    got = torch.from_numpy(Wn.emu_wmat2(Wn.cmat32(tile, "Gt"), u))
    return H.ratio(got, ref, bound)


@pytest.mark.parametrize("kind", ["calib", "spread"])
@pytest.mark.parametrize("tile", Wn.TILES)
def test_standin_wgrad(kind, tile):
    assert _wgrad_ratio(kind, tile) <= 1


# ---- the mutants ---------------------------------------------------------------------------
def _swapped_rows(tile):
    C32 = Wn.cmat32(tile, "Bt").copy()
    C32[[1, 2]] = C32[[2, 1]]
    return C32


def _perturbed_g(tile):
    C32 = Wn.cmat32(tile, "G").copy()
    C32[1, 1] = np.float32(C32[1, 1] * (1 + 2.0 ** -12))
    return C32


def _filter_mut(tile):
    w = Wn.make_filters(5, 7)
    ref, bound = Wn.filter_ref(w, tile, False, 8, 8)
    return H.ratio(_stand_filter(w, tile, False, _perturbed_g(tile)), ref[:, :5, :7], bound[:, :5, :7])


def _bias_mut(tile):
    B, H_, W_ = 2, 9, 11
    TH, TW = Wn.tiles_hw(H_, W_, tile)
    Mp = Wn.make_planes((tile + 2) ** 2, B * TH * TW, C, seed=2)
    bias = torch.randn(C, generator=H.gen(3)) * 0.1
    return _output_ratio(Mp, bias, B, H_, W_, tile, drop_bias=True)


MUTANTS = {
    "bt_rows_swapped": lambda t: _input_ratio("calib", SHAPES[0], t, C32=_swapped_rows(t)),
    "ct_x_c": lambda t: _input_ratio("calib", SHAPES[0], t, C32=Wn.cmat32(t, "Bt").T.copy()),
    "edge_clamped": lambda t: _input_ratio("calib", SHAPES[0], t, clamp_fill=True),
    "last_tile_shifted": lambda t: _input_ratio("calib", SHAPES[0], t, shift_last=True),
    "l_dropped": lambda t: _h2_ratio("calib", t, drop_l=True)[0],
    "h_truncated": lambda t: _h2_ratio("calib", t, pure=True, trunc=True)[0],
    "exponent_off_by_one": lambda t: _h2_ratio("calib", t, exp_off=-1)[0],
    "g_coefficient": _filter_mut,
    "hl_product_dropped": lambda t: _gemm_ratio("calib", drop_hl=True),
    "last_slab_dropped": lambda t: _wgrad_ratio("calib", t, splits=3, drop_last=True),
    "bias_dropped": _bias_mut,
    "chunk_swapped": lambda t: _h2_ratio("calib", t, swap_chunks=True)[0],
}


@pytest.mark.parametrize("tile", [4, 6])
@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_fails_a_bound(name, tile):
    r = MUTANTS[name](tile)
    assert r > 1, (name, tile, r)


def test_ops_table():
    """c = 2 nnz + 1 (+ 2 where a coefficient is not an fp32 number): only the
    G matrices of F(4x4) and F(6x6) carry the + 2."""
    for (tile, name), (c, nnz, inexact) in Wn.OPS.items():
        assert c == 2 * nnz + 1 + 2 * inexact
        assert inexact == (name in ("G", "Gt") and tile in (4, 6)), (tile, name)
    assert Wn.OPS[(6, "Bt")][1] == 6 and Wn.OPS[(4, "Bt")][1] == 5 and Wn.OPS[(6, "A")][1] == 6


@pytest.mark.parametrize("tile", Wn.TILES)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_wino_beta_bounds_exact_transform(tile, which):
    """nsm_wino_beta(tile, which) >= (max row sum of |C|)^2 of the exact matrix
    (host function of the library)."""
    from nsm_amd._lib import lib
    beta = float(lib.nsm_wino_beta(tile, which))
    assert beta >= float(Wn.beta_exact(tile, which)), (beta, Wn.beta_exact(tile, which))
