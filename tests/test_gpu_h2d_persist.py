"""The persistent form of the h2 1x1 input-gradient GEMM with the first BN's
backward in its epilogue (csrc/nsm_conv_h2d.inc gemm_h2bp_kernel, behind
nsm_conv1x1_dgrad_bnbwd_h2): a fixed grid walks the output tiles with the
K-tile stream and the Y1 fetch running across them.

GPU: its results do not depend on the grid (bitwise), they are bitwise those
of the one-tile-per-block kernel at the same tile (same MFMA shape, product
and K order, same epilogue arithmetic and merge order), they meet the float64
bounds of tests/test_gpu_h2d.py::test_conv1x1_dgrad_bnbwd_h2, and the plan
query reports what runs. The shapes are chosen for where a tile walk can go
wrong: ragged last tile, fewer tiles than blocks, one and two N tiles per
partial row, even and odd K-tile counts, a Dropout2d mask row that changes
inside a tile.

CPU: the exported tile decoder (the function the kernel uses) visits every
tile exactly once for every grid, N tiles of an M block consecutive."""
import functools

import pytest
import torch

gpu = pytest.mark.gpu

SLOPE = 0.2
# K = 2 cop f16 columns = cop / 32 K-tiles: 2, 4, 16 and the odd 3; K = 64 (one
# K-tile) is not covered by the persistent form and must run the old kernel
COPS = {128: 64, 256: 128, 1024: 512, 192: 96}
BM = 128  # rows of the tile h2d_tile gives every shape below but BIG (asserted in _case)
SMALL = [(M, N, K) for N in (128, 256) for M in (5 * BM + 37, BM - 5) for K in (128, 256, 1024, 192)]
# the 256x128 tile (K > 512, >= 256 tiles): 33 M blocks (the last one ragged) x 8 N tiles
BIG = (32 * 256 + 37, 1024, 1024)
HW = 100


@pytest.fixture(scope="module")
def ops(device):
    from nsm_amd import ops as O
    prev = O.set_f32_split(2)
    form = O.set_h2d_bnb_persist()
    yield O
    O.set_h2d_bnb_persist(*form)
    O.set_f32_split(prev)


def _spread(g, n, lo, hi):
    return torch.pow(2.0, torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo)


@functools.lru_cache(maxsize=None)
def _case(M, cip, K, hw=HW):
    """Inputs of test_conv1x1_dgrad_bnbwd_h2's generator (float64 on the
    device), the fp32 / h2 operands and the BN state; made once per shape."""
    from nsm_amd import ops
    device = torch.device("cuda:0")
    cop = K // 2
    g = torch.Generator().manual_seed(M + cip * 3 + cop)
    B = -(-M // hw)
    dY2 = torch.randn(M, cop, generator=g, dtype=torch.float64) * _spread(g, cop, -4, 0)
    w = torch.randn(cop, cip, generator=g, dtype=torch.float64) / cop ** 0.5
    Y1 = torch.randn(M, cip, generator=g, dtype=torch.float64) * _spread(g, cip, -4, 2)
    gamma = torch.randn(cip, generator=g, dtype=torch.float64) * _spread(g, cip, -4, 0)
    beta = torch.randn(cip, generator=g, dtype=torch.float64) * 0.1
    mask = (torch.rand(B, cip, generator=g) > 0.2).double() / 0.8
    c = dict(M=M, cip=cip, cop=cop, hw=hw)
    c["f64"] = tuple(t.to(device) for t in (dY2, w, Y1, gamma, beta, mask))
    f32 = lambda t: t.float().to(device).contiguous()  # noqa: E731
    c["dY2"], c["Y1"], c["mask"] = f32(dY2), f32(Y1), f32(mask)
    bn = torch.nn.BatchNorm2d(cip).to(device)
    with torch.no_grad():
        bn.weight.copy_(gamma.float())
        bn.bias.copy_(beta.float())
    c["st"] = ops.bn_train(c["Y1"], bn, cip, 0.1, 1e-5)
    am = ops.amax_slots(2, device)
    c["ady"], c["aw"] = ops.amax_slot(am, 0), ops.amax_slot(am, 1)
    ops.absmax(c["dY2"], c["ady"])
    c["wd"] = ops.pack_conv_weight(f32(w).view(cop, cip, 1, 1), cop, cip, ops.PACK_DGRAD)
    ops.absmax(c["wd"], c["aw"])
    c["dY2h"] = ops.to_h2(c["dY2"], c["ady"])
    c["wdh"] = ops.to_h2(c["wd"].view(cip, cop), c["aw"])
    return c


def _run(ops, c, form, grid=0):
    """Every output of the op in one kernel form: mode 1 (dA1, partial rows,
    max|scale dz| slot, then dgamma / dbeta / coef from the finalize), mode 0
    (partial rows alone) and mode 2 (dy, max|dy| slot)."""
    from nsm_amd._lib import call, ptr, stream
    device = c["dY2"].device
    M, cip, cop = c["M"], c["cip"], c["cop"]
    prev = ops.set_h2d_bnb_persist(form, grid)
    try:
        rows = ops.conv1x1_dgrad_bnbwd_h2_plan(M, cip, cop)[3]
        nchunk = -(-M // rows)
        out = {}
        gr = [torch.zeros(cip, device=device) for _ in range(3)]
        sl = ops.amax_slots(3, device)
        k1dz, bound, aout = (ops.amax_slot(sl, i) for i in range(3))
        d = ops.conv1x1_dgrad_bn_bwd_h2(c["dY2h"], c["hw"], c["wdh"], c["Y1"], c["st"], c["mask"], cip,
                                        *gr, False, amax=(c["ady"], c["aw"]), h2_out=(k1dz, bound),
                                        defer=True)
        out["dA1"], out["coef"], out["dgamma"], out["dbeta"], out["k1dz"] = d.g, d.coef, gr[0], gr[1], k1dz
        gr2 = [torch.zeros(cip, device=device) for _ in range(3)]
        out["dy"] = ops.conv1x1_dgrad_bn_bwd_h2(c["dY2h"], c["hw"], c["wdh"], c["Y1"], c["st"], c["mask"],
                                                cip, *gr2, True, amax=(c["ady"], c["aw"]),
                                                amax_out=aout)
        out["dgamma2"], out["dbeta2"], out["aout"] = gr2[0], gr2[1], aout
        # the stored-dA1 path to its end (nsm_bn_bwd_apply)
        gr3 = [torch.zeros(cip, device=device) for _ in range(3)]
        out["dy1"] = ops.conv1x1_dgrad_bn_bwd_h2(c["dY2h"], c["hw"], c["wdh"], c["Y1"], c["st"], c["mask"],
                                                 cip, *gr3, False, amax=(c["ady"], c["aw"]))
        st = c["st"]
        part = torch.full((nchunk * 2 * cip,), float("nan"), device=device)
        call("nsm_conv1x1_dgrad_bnbwd_h2", ptr(c["dY2h"]), M, cop, ptr(c["wdh"]), cip, ptr(c["Y1"]),
             c["Y1"].stride(0), ptr(st.scale), ptr(st.shift), ptr(st.mean), ptr(st.invstd),
             ptr(c["mask"]), c["hw"], SLOPE, 0, ptr(part), None, None, 0, ptr(c["ady"]), ptr(c["aw"]),
             None, None, stream())
        out["partial"] = part
        torch.cuda.synchronize()
        return out
    finally:
        ops.set_h2d_bnb_persist(*prev)


def _same(a, b, keys, what):
    for k in keys:
        x, y = a[k], b[k]
        if x.dtype.is_floating_point:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), (what, k)


ALL = ("dA1", "dy", "dy1", "partial", "coef", "dgamma", "dbeta", "dgamma2", "dbeta2", "k1dz", "aout")


def _slot_max(s):
    return int(s.view(torch.int32).max().item())


def _tiles(M, N, rows):
    return -(-M // rows) * (N // 128)


def _covered(K):
    return K >= 128


@gpu
@pytest.mark.parametrize("M,N,K", SMALL + [BIG])
def test_grid_independence_bitwise(ops, device, M, N, K):
    c = _case(M, N, K)
    tile, form, grid0, rows = _plan_forced(ops, c)
    assert form == "persistent"
    assert rows == (256 if (M, N, K) == BIG else BM)
    tiles = _tiles(M, N, rows)
    base = _run(ops, c, "persistent", 0)
    assert not torch.isnan(base["partial"]).any()
    for g in sorted({1, 3, max(tiles - 1, 1)}):
        got = _run(ops, c, "persistent", g)
        _same(base, got, ALL, f"grid {g} vs default")


def _plan_forced(ops, c):
    prev = ops.set_h2d_bnb_persist("persistent", 0)
    try:
        return ops.conv1x1_dgrad_bnbwd_h2_plan(c["M"], c["cip"], c["cop"])
    finally:
        ops.set_h2d_bnb_persist(*prev)


@gpu
@pytest.mark.parametrize("M,N,K,hw", [s + (HW,) for s in SMALL + [BIG]] +
                         [(5 * BM + 37, 256, 256, 40)])  # HW < 64: the mask row loaded per pixel row
def test_old_vs_persistent_bitwise(ops, device, M, N, K, hw):
    """Same tile, 32x32x16 MFMA, product order and K order in both forms: every
    output is bit-identical. The operand-maximum slots hold the same maximum
    (the one-tile-per-block kernel picks the slot's line by block index, the
    persistent form by tile, so the lines differ)."""
    c = _case(M, N, K, hw)
    old = _run(ops, c, "old")
    new = _run(ops, c, "persistent")
    assert _plan_forced(ops, c)[1] == "persistent"
    _same(old, new, [k for k in ALL if k not in ("k1dz", "aout")], "old vs persistent")
    for k in ("k1dz", "aout"):
        assert _slot_max(old[k]) == _slot_max(new[k]) > 0, k


@gpu
def test_single_k_tile_stays_on_old_kernel(ops, device):
    """K = 64 is one K-tile: the stream would have to run two tiles ahead, so
    the persistent form does not claim it, however it is forced."""
    prev = ops.set_h2d_bnb_persist("persistent", 0)
    try:
        for M, N in ((5 * BM + 37, 128), (524288, 128)):
            tile, form, grid, rows = ops.conv1x1_dgrad_bnbwd_h2_plan(M, N, 32)
            assert (form, grid) == ("old", 0)
    finally:
        ops.set_h2d_bnb_persist(*prev)


def _errs(a, ref):
    d = (a.double() - ref).abs()
    return d.max().item(), d.pow(2).mean().sqrt().item()


@gpu
@pytest.mark.parametrize("M,N,K", [(5 * BM + 37, 256, 256), (BM - 5, 128, 1024), (5 * BM + 37, 128, 192),
                                   BIG])
def test_fp64_parity(ops, device, M, N, K):
    """The bounds of test_conv1x1_dgrad_bnbwd_h2: against a float64 restatement
    the persistent form's error stays within 1.5x (rms) / 2.0x (max) of the
    exact fp32-MFMA path's on the same inputs, dgamma / dbeta within max(1.5x
    that path's error, 1e-5 relative). The fp32 path takes whole images, so it
    gets HW = 1 and the mask row of every pixel's image."""
    c = _case(M, N, K)
    dY2, w, Y1, gamma, beta, mask = c["f64"]
    mrow = mask.repeat_interleave(HW, 0)[:M]
    mu, var = Y1.mean(0), Y1.var(0, unbiased=False)
    inv = (var + 1e-5).rsqrt()
    xhat = (Y1 - mu) * inv
    z = xhat * gamma + beta
    dz = (dY2 @ w) * torch.where(z > 0, 1.0, 0.2) * mrow
    ref = gamma * inv * (dz - dz.mean(0) - xhat * (dz * xhat).mean(0))
    got = _run(ops, c, "persistent")
    bn_bwd_apply = {}
    for recompute in (False, True):
        gr = [torch.zeros(N, device=device) for _ in range(3)]
        prev = ops.set_f32_split(0)
        try:
            dy0 = ops.conv1x1_dgrad_bn_bwd(c["dY2"], M, 1, 1, c["wd"], c["Y1"], c["st"],
                                           mrow.float().contiguous(), N, *gr, recompute)
        finally:
            ops.set_f32_split(prev)
        bn_bwd_apply[recompute] = (dy0, gr)
    torch.cuda.synchronize()
    # dy of the recompute path (modes 0 + 2) and of the stored-dA1 path (mode 1)
    for name, dy, rec in (("mode 2", got["dy"], True), ("mode 1", got["dy1"], False)):
        (mx, rms), (mx0, rms0) = _errs(dy, ref), _errs(bn_bwd_apply[rec][0], ref)
        print(f"{name}: max {mx:.3e} rms {rms:.3e}; fp32 path max {mx0:.3e} rms {rms0:.3e}")
        assert rms <= 1.5 * rms0 + 1e-12 and mx <= 2.0 * mx0 + 1e-12, (name, mx, rms, mx0, rms0)
    for k, key, rr in ((0, "dgamma", (dz * xhat).sum(0)), (1, "dbeta", dz.sum(0))):
        for rec, kk in ((False, key), (True, key + "2")):
            e = (got[kk].double() - rr).norm().item()
            e0 = (bn_bwd_apply[rec][1][k].double() - rr).norm().item()
            print(f"{kk}: err {e:.3e}; fp32 path {e0:.3e}; norm {rr.norm().item():.3e}")
            assert e <= max(1.5 * e0, 1e-5 * rr.norm().item()), (kk, e, e0)


@gpu
def test_plan(ops, device):
    """The policy sends the B=8 512x512 step's conv6 / conv7 / conv8 to the
    persistent form; what the form does not cover, and shapes with no more
    tiles than resident blocks, stay on the old kernel; the partial rows are
    those of nsm_conv1x1_h2_rows."""
    from nsm_amd._lib import lib
    prev = ops.set_h2d_bnb_persist("policy", 0)
    try:
        cus = torch.cuda.get_device_properties(device).multi_processor_count
        for (M, cip, cop), tile in (((32768, 1024, 512), 2), ((131072, 512, 128), 3),
                                    ((524288, 128, 64), 3)):
            t, form, grid, rows = ops.conv1x1_dgrad_bnbwd_h2_plan(M, cip, cop)
            assert (t, form) == (tile, "persistent")
            assert grid in (cus, 2 * cus) and grid <= _tiles(M, cip, rows)
            assert rows == lib.nsm_conv1x1_h2_rows(M, cip, 2 * cop, 1) == (256 if tile == 2 else 128)
        # conv9 (one K-tile, 64 columns), conv2 / conv3 (narrow N), conv4 / conv5 (one round of blocks)
        for M, cip, cop in ((524288, 64, 32), (524288, 32, 64), (131072, 64, 128), (32768, 128, 512),
                            (8192, 512, 1024)):
            t, form, grid, rows = ops.conv1x1_dgrad_bnbwd_h2_plan(M, cip, cop)
            assert (form, grid) == ("old", 0)
            assert rows == lib.nsm_conv1x1_h2_rows(M, cip, 2 * cop, 1)
        ops.set_h2d_bnb_persist("old", 0)
        assert ops.conv1x1_dgrad_bnbwd_h2_plan(524288, 128, 64)[1] == "old"
        ops.set_h2d_bnb_persist("persistent", 7)
        assert ops.conv1x1_dgrad_bnbwd_h2_plan(524288, 128, 64)[1:3] == ("persistent", 7)
        assert ops.conv1x1_dgrad_bnbwd_h2_plan(123, 128, 64)[1:3] == ("persistent", 1)
        assert ops.set_h2d_bnb_persist() == (2, 7)
    finally:
        ops.set_h2d_bnb_persist(*prev)


def _splits(total):
    return [(total // gy, gy) for gy in (1, 2, 3, 4, 8) if total % gy == 0]


@pytest.mark.parametrize("total", [1, 7, 8, 24, 1024, 4096 + 8])
def test_tile_walk_covers_every_tile_once(total):
    """No GPU: nsm_h2d_tile_walk runs the kernel's decoder on the host."""
    from nsm_amd import ops
    for gx, gy in _splits(total):
        remap = gy > 1 and total % 8 == 0
        for grid in (1, 3, 256, 512):
            seen = {}
            for b in range(grid):
                walk = ops.h2d_tile_walk(gx, gy, grid, b)
                assert len(walk) == len(range(b, total, grid))
                for i, (m, n, lg) in enumerate(walk):
                    L = b + i * grid
                    assert 0 <= m < gx and 0 <= n < gy
                    assert (m, n) not in seen, (gx, gy, grid, m, n)
                    # an M block's N tiles are consecutive in the logical order
                    assert lg == m * gy + n
                    # which is the dispatch order, or XCD-contiguous runs of it
                    assert lg == ((L % 8) * (total // 8) + L // 8 if remap else L)
                    seen[(m, n)] = L
            assert len(seen) == total
