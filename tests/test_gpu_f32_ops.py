"""GPU: the direct implicit GEMMs of the fp32 train step (csrc/nsm_conv.hip:
the convolutions of the 32- and 64-channel layers and their backward) one by
one, in the three arithmetic modes of set_f32_split (0: fp32 MFMA, 1: bf16
three-way split, 2: the f16x2 split with the operands' maxima, the default of
the model path): the forward and the input gradient on every tile of
dispatch_conv_fwd, nsm_conv_wgrad on the nine tiles of dispatch_wgrad, and
nsm_conv1x1_dgrad_bnbwd (EpiBnBwd) on the 128- and 256-row tiles, each against
a float64 restatement on plain torch under the element-wise worst-case bounds
of f32_util.py (derived there; none measured on the kernels). The worst err /
bound of every family goes to parity_margins.json as f32_ops.<family>."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eval_util as E
import f16_util as U16
import f32_util as U
from test_gpu_f16_ops import bn_bwd_ref, bn_vectors, drop_mask
from test_gpu_ops import nchw
from util import record_margin

pytestmark = pytest.mark.gpu
torch.set_num_threads(16)
MODES = [0, 1, 2]


@pytest.fixture(scope="module")
def ops(device):
    from nsm_amd import ops as O
    prev = O.set_f32_split(2)
    yield O
    O.set_f32_split(prev)


# ---- helpers -------------------------------------------------------------------
_WORST = {}


def margin(family, case_id, ratio):
    """Keep the worst error / bound of a kernel family in parity_margins.json."""
    if ratio >= _WORST.get(family, (-1.0, None))[0]:
        _WORST[family] = (float(ratio), case_id)
        record_margin("f32_ops." + family, worst_err_over_bound=float(ratio), case=case_id)


def check(family, case_id, got, ref, bound, keep=None):
    """assert |got - ref| <= bound element-wise (on `keep`), recording the margin."""
    if keep is not None:
        got, ref, bound = got[keep], ref[keep], bound[keep]
    r = U.ratio(got, ref, bound)
    print(f"{family} {case_id}: worst err / bound {r:.3f}")
    margin(family, case_id, r)
    assert r <= 1.0, (family, case_id, r)


_REF = {}


def cached(key, make):
    """One float64 reference at a time, shared by the consecutive tests on it
    (the parametrisations below keep the modes of a shape together)."""
    if key not in _REF:
        _REF.clear()
        _REF[key] = make()
    return _REF[key]


def sid(*s):
    return "x".join(str(v) for v in s)


def slot_value(slot):
    """The maximum an operand-maximum slot holds (its 64 lines reduced)."""
    v = slot.view(torch.int32).cpu().numpy().astype(np.uint32).max()
    return float(np.array(v, dtype=np.uint32).view(np.float32))


def slot_holding(ops, device, value):
    """A slot whose content is `value` (one line set: amax_read takes the maximum)."""
    s = ops.amax_slots(1, device)
    s.view(torch.float32)[0] = value
    return s


def make_case(kind, B, H, W, ci, co, k):
    return U.make_spread_case(B, H, W, ci, co, k) if kind == "spread" else E.make_case(B, H, W, ci, co, k)


def fwd_case(B, H, W, ci, co, k, kind):
    """(case, ref, S) of the forward convolution, [M, co] float64."""
    def make():
        case = make_case(kind, B, H, W, ci, co, k)
        return (case, E.nhwc(U.conv_ref(case.x, case.w, case.b)),
                E.nhwc(U.conv_ref(case.x, case.w, case.b, absval=True)))
    return cached(("fwd", B, H, W, ci, co, k, kind), make)


def dgrad_case(B, H, W, ci, co, k, kind):
    """The input gradient with the forward's GEMM geometry: dy has ci
    channels, dx co (w: [ci, co, k, k]), so N = co and K = taps * ci."""
    def make():
        case = make_case(kind, B, H, W, ci, co, k)
        case.dy, case.wd = case.x, case.w.transpose(0, 1).contiguous()
        return (case, E.nhwc(U.dgrad_ref(case.dy, case.wd)),
                E.nhwc(U.dgrad_ref(case.dy, case.wd, absval=True)))
    return cached(("dgrad", B, H, W, ci, co, k, kind), make)


def run_fwd(ops, device, case, mode, slots=None):
    """conv_fwd of a case in `mode`; mode 2 with the operands' maxima from
    nsm_absmax, or with the given slot pair. Returns (y, (amax_x, amax_w))."""
    ops.set_f32_split(mode)
    xd = E.nhwc(case.x).to(device)
    wp = ops.pack_conv_weight(case.w.to(device), case.co, case.ci, ops.PACK_FWD)
    am = (None, None)
    if mode == 2:
        am = slots if slots is not None else (ops.absmax(xd), ops.absmax(wp))
    y = ops.conv_fwd(xd, case.B, case.H, case.W, wp, case.b.to(device), case.co, case.k, amax=am)
    return y.cpu(), am


def fwd_bound(case, S, mode, am):
    K = case.k * case.k * case.ci
    floor = None
    if mode == 2:
        floor = E.nhwc(U.conv_floor(case.x, case.w, slot_value(am[0]), slot_value(am[1]))
                       .expand(case.B, case.co, case.H, case.W))
    return U.gemm_bound(mode, S, K, floor=floor)


# ---- a. forward and input gradient on every tile of dispatch_conv_fwd --------------
# (B, H, W, cin, cout, k, rows, kind): eval_util.SMALL run the 64-row tiles
# (64x64, 64x32, 64x128), F32_LARGE the 128- and 256-row ones; the last uniform
# shape is the 256x32 tile with the 3x3 im2col loader (conv2.0 at 512^2)
CONV_CASES = ([s + (64, "uniform") for s in E.SMALL] + [s + ("uniform",) for s in E.F32_LARGE]
              + [(1, 723, 725, 32, 32, 3, 256, "uniform"),
                 (2, 9, 11, 32, 64, 3, 64, "spread"), (1, 209, 313, 32, 32, 3, 128, "spread")])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,H,W,ci,co,k,rows,kind", CONV_CASES)
def test_conv_fwd(ops, device, B, H, W, ci, co, k, rows, kind, mode):
    from nsm_amd._lib import lib
    assert lib.nsm_conv_stat_rows(B, H, W, co) == rows
    case, ref, S = fwd_case(B, H, W, ci, co, k, kind)
    y, am = run_fwd(ops, device, case, mode)
    if mode == 2:
        assert slot_value(am[0]) == case.x.abs().max().item()
        assert slot_value(am[1]) == case.w.abs().max().item()
    check("conv_fwd", sid(B, H, W, ci, co, k, kind, "m%d" % mode), y, ref, fwd_bound(case, S, mode, am))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,H,W,ci,co,k,rows,kind", CONV_CASES)
def test_conv_dgrad(ops, device, B, H, W, ci, co, k, rows, kind, mode):
    """conv_fwd with PACK_DGRAD weights and no bias against conv_transpose."""
    from nsm_amd._lib import lib
    assert lib.nsm_conv_stat_rows(B, H, W, co) == rows
    case, ref, S = dgrad_case(B, H, W, ci, co, k, kind)
    ops.set_f32_split(mode)
    dyd = E.nhwc(case.dy).to(device)
    wd = ops.pack_conv_weight(case.wd.to(device), ci, co, ops.PACK_DGRAD)
    am, floor = (None, None), None
    if mode == 2:
        am = (ops.absmax(dyd), ops.absmax(wd))
        floor = E.nhwc(U.dgrad_floor(case.dy, case.wd, slot_value(am[0]), slot_value(am[1]))
                       .expand(B, co, H, W))
    dx = ops.conv_fwd(dyd, B, H, W, wd, None, co, k, amax=am)
    check("conv_dgrad", sid(B, H, W, ci, co, k, kind, "m%d" % mode), dx.cpu(), ref,
          U.gemm_bound(mode, S, k * k * ci, floor=floor))


AMAX_CASES = [(2, 9, 11, 32, 64, 3, "uniform"), (2, 9, 11, 32, 64, 3, "spread"),
              (1, 209, 313, 32, 32, 3, "spread")]


@pytest.mark.parametrize("B,H,W,ci,co,k,kind", AMAX_CASES)
def test_conv_fwd_amax_upper_bound(ops, device, B, H, W, ci, co, k, kind):
    """Mode 2 with slots that hold 8x the true maxima (a producer's bound
    instead of the maximum): a coarser scale, within the bound computed from
    the slot values."""
    case, ref, S = fwd_case(B, H, W, ci, co, k, kind)
    slots = (slot_holding(ops, device, 8 * case.x.abs().max().item()),
             slot_holding(ops, device, 8 * case.w.abs().max().item()))
    assert U.pow2_up(slot_value(slots[0])) == 8 * U.pow2_up(case.x.abs().max().item())
    y, am = run_fwd(ops, device, case, 2, slots=slots)
    check("conv_fwd", sid(B, H, W, ci, co, k, kind, "m2-amax8"), y, ref, fwd_bound(case, S, 2, am))


@pytest.mark.parametrize("B,H,W,ci,co,k", [(2, 9, 11, 32, 64, 3), (1, 209, 313, 32, 32, 3)])
def test_conv_fwd_zero_operand(ops, device, B, H, W, ci, co, k):
    """Mode 2 with an all-zero activation operand: its slot stays 0 (scale 1),
    and the output is the bias exactly, no NaN."""
    case = E.make_case(B, H, W, ci, co, k)
    case.x = torch.zeros_like(case.x)
    y, am = run_fwd(ops, device, case, 2)
    assert slot_value(am[0]) == 0.0
    assert not torch.isnan(y).any()
    assert torch.equal(y, case.b.view(1, co).expand(B * H * W, co))
    margin("conv_fwd", sid(B, H, W, ci, co, k, "zero"), 0.0)


# ---- b. conv_wgrad on the nine tiles of dispatch_wgrad ------------------------------
# plan_wgrad: BM = 128 / 64 / 32 for cout_p >= 128 / 64 / 32; BN = 128 for every
# 3x3 and for 1x1 with cin >= 128, 64 / 32 for 1x1 with cin 64 / 32.
# (B, H, W, cin_p, cout_p, k). K = 198: ragged against the 32-wide K step, one
# split; K = 2146: several splits, the last one short; (2, 64, 64): more than
# 16 splits, splitsum_kernel runs first. 3x3 with cin 32 / 64: the multi-tap N
# tiles (cin 32: N = 288, the last tile ragged).
CH = (32, 64, 128)
WGRAD_CASES = ([(2, 9, 11, ci, co, 1) for ci in CH for co in CH]
               + [(2, 37, 29, ci, co, 1) for ci in CH for co in CH]
               + [(2, 9, 11, ci, co, 3) for ci in CH for co in (32, 128)]
               + [(2, 64, 64, ci, co, 3) for ci in CH for co in (32, 128)])


def wgrad_tile(cin_p, cout_p, k):
    bm = 128 if cout_p >= 128 else (64 if cout_p >= 64 else 32)
    bn = 128 if (cin_p >= 128 or k == 3) else (64 if cin_p >= 64 else 32)
    return bm, bn


def test_wgrad_cases_cover_the_nine_tiles():
    assert {wgrad_tile(ci, co, k) for _, _, _, ci, co, k in WGRAD_CASES} == {
        (bm, bn) for bm in (128, 64, 32) for bn in (128, 64, 32)}


def run_wgrad(ops, device, dyd, xd, B, H, W, k, cin, cout, dw, mode, pro=None, amax=(None, None)):
    """nsm_conv_wgrad with a workspace of exactly nsm_conv_wgrad_ws floats
    followed by a guard that must come back untouched."""
    from nsm_amd._lib import call, lib, ptr, stream
    ops.set_f32_split(mode)
    cout_p, cin_p = dyd.shape[1], xd.shape[1]
    n = int(lib.nsm_conv_wgrad_ws(B, H, W, cin_p, cout_p, k))
    assert n == int(ops.call_ws(B, H, W, cin_p, cout_p, k))
    mn = cout_p * k * k * cin_p
    assert n >= mn and n % mn == 0               # whole [M, N] slabs (and 16-way stage-1 sums)
    guard = 4096
    ws = torch.full((n + guard,), float("nan"), device=device)
    sc, sh, mk = pro if pro is not None else (None, None, None)
    call("nsm_conv_wgrad", ptr(dyd), dyd.stride(0), ptr(xd), xd.stride(0), B, H, W, cin_p, cout_p, k,
         ptr(sc), ptr(sh), ptr(mk), 0.2, ptr(ws), n, cin, cout, ptr(dw),
         ptr(amax[0]), ptr(amax[1]), stream())
    assert torch.isnan(ws[n:]).all()
    return n // mn


def wgrad_operands(B, H, W, cip, cop, k):
    def make():
        g = U.gen(B, H, W, cip, cop, k, 41)
        x = U16.normal_values((B, cip, H, W), g, "f32")
        dy = U16.normal_values((B, cop, H, W), g, "f32")
        return x, dy, U.wgrad_ref(x, dy, k), U.wgrad_ref(x, dy, k, absval=True)
    return cached(("wgrad", B, H, W, cip, cop, k), make)


def wgrad_check(ops, device, case_id, x, dy, xd, dyd, k, ci, co, ref, S, mode, B, H, W):
    """One no-prologue nsm_conv_wgrad run in `mode` (mode 2 with the maxima of
    contiguous copies of the operands) against ref [co, ci, k, k]."""
    am, floor = (None, None), None
    if mode == 2:
        am = (ops.absmax(E.nhwc(dy).to(device)), ops.absmax(E.nhwc(x).to(device)))
        floor = U.wgrad_floor(x, dy, k, slot_value(am[0]), slot_value(am[1]))[:co, :ci]
    dw = torch.full((co, ci, k, k), float("nan"), device=device)
    slabs = run_wgrad(ops, device, dyd, xd, B, H, W, k, ci, co, dw, mode, amax=am)
    check("conv_wgrad", case_id + "-m%d" % mode, dw.cpu(), ref, U.wgrad_bound(mode, S, B * H * W, floor=floor))
    return slabs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,H,W,cip,cop,k", WGRAD_CASES)
def test_conv_wgrad(ops, device, B, H, W, cip, cop, k, mode):
    x, dy, ref, S = wgrad_operands(B, H, W, cip, cop, k)
    slabs = wgrad_check(ops, device, sid(B, H, W, cip, cop, k), x, dy, E.nhwc(x).to(device),
                        E.nhwc(dy).to(device), k, cip, cop, ref, S, mode, B, H, W)
    if (H, W) == (9, 11):
        assert slabs == 1
    elif (H, W) == (64, 64):
        assert slabs > 16 + 1                    # the splits and their 16-way stage-1 sums
    else:
        assert 1 < slabs <= 16


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("B,H,W,cip,cop", [(2, 37, 29, 32, 64), (2, 37, 29, 128, 64)])
def test_conv_wgrad_prologue(ops, device, B, H, W, cip, cop, mode):
    """BN-apply + LeakyReLU + Dropout2d in the activation loader (1x1). The
    loader's four fp32 operations move an operand element by at most
    prologue_ref's d, which joins the bound through |dy|. A prologue GEMM
    ignores the maxima (its operand is transformed after they were recorded):
    mode 2, given them, still meets the mode-1 bound."""
    def make():
        g = U.gen(B, H, W, cip, cop, 1, 42)
        x = U16.normal_values((B, cip, H, W), g, "f32")
        dy = U16.normal_values((B, cop, H, W), g, "f32")
        sc = (torch.rand(cip, generator=g) + 0.5) * torch.where(torch.rand(cip, generator=g) < 0.25, -1.0, 1.0)
        sh = torch.randn(cip, generator=g)
        mask = drop_mask(B, cip, g)
        a, d = U16.prologue_ref(x, sc, sh, mask, "f32")
        return (x, dy, (sc, sh, mask), U.wgrad_ref(a, dy, 1), U.wgrad_ref(a, dy, 1, absval=True),
                U.wgrad_ref(d, dy, 1, absval=True))
    x, dy, pro, ref, S, extra = cached(("wgrad_pro", B, H, W, cip, cop), make)
    xd, dyd = E.nhwc(x).to(device), E.nhwc(dy).to(device)
    am = (ops.absmax(dyd), ops.absmax(xd)) if mode == 2 else (None, None)
    dw = torch.full((cop, cip, 1, 1), float("nan"), device=device)
    run_wgrad(ops, device, dyd, xd, B, H, W, 1, cip, cop, dw, mode, pro=tuple(t.to(device) for t in pro),
              amax=am)
    check("conv_wgrad", sid(B, H, W, cip, cop, 1, "pro") + "-m%d" % mode, dw.cpu(), ref,
          U.wgrad_bound(1, S, B * H * W) + extra)


@pytest.mark.parametrize("mode", MODES)
def test_conv_wgrad_padded_real_dims(ops, device, mode):
    """cin = cout = 7 in 32-wide storage, 3x3: dw comes back fully written at
    its real size [7, 7, 3, 3] and nothing behind it is touched; the pad
    columns of the activation hold non-zero values (times the zero pad columns
    of dy), so a wrong channel index shows in the result."""
    B, H, W, c, cp, k = 2, 9, 11, 7, 32, 3
    g = U.gen(B, H, W, c, k, 43)
    x = U16.normal_values((B, cp, H, W), g, "f32")
    dy = F.pad(U16.normal_values((B, c, H, W), g, "f32"), (0, 0, 0, 0, 0, cp - c))
    assert x[:, c:].abs().min().item() > 0 and dy[:, c:].abs().max().item() == 0
    ref = U.wgrad_ref(x, dy, k)[:c, :c]
    S = U.wgrad_ref(x, dy, k, absval=True)[:c, :c]
    xd, dyd = E.nhwc(x).to(device), E.nhwc(dy).to(device)
    am, floor = (None, None), None
    if mode == 2:
        am = (ops.absmax(dyd), ops.absmax(xd))
        floor = U.wgrad_floor(x, dy, k, slot_value(am[0]), slot_value(am[1]))[:c, :c]
    n = c * c * k * k
    buf = torch.full((n + 256,), -7777.0, device=device)
    run_wgrad(ops, device, dyd, xd, B, H, W, k, c, c, buf, mode, amax=am)
    out = buf.cpu()
    assert (out[n:] == -7777.0).all()
    assert (out[:n] != -7777.0).all()
    check("conv_wgrad", "padded7-m%d" % mode, out[:n].view(c, c, k, k), ref,
          U.wgrad_bound(mode, S, B * H * W, floor=floor))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 3])
def test_conv_wgrad_column_slices(ops, device, k, mode):
    """Both operands as 16-byte aligned column slices of wider buffers (row
    stride c + 4, a sentinel in the other columns that a wrong stride reads)."""
    B, H, W, cip, cop = 2, 37, 29, 64, 64
    x, dy, ref, S = wgrad_operands(B, H, W, cip, cop, k)

    def sliced(t):
        r = E.nhwc(t)
        wide = torch.cat([torch.full((r.shape[0], 4), 1e3), r], 1).to(device)
        v = wide[:, 4:]
        assert v.stride(0) == r.shape[1] + 4 and v.data_ptr() % 16 == 0
        return v

    wgrad_check(ops, device, sid(B, H, W, cip, cop, k, "ld+4"), x, dy, sliced(x), sliced(dy), k, cip, cop,
                ref, S, mode, B, H, W)


# ---- c. conv1x1_dgrad_bn_bwd on the 128- and 256-row tiles ---------------------------
# (B, H, W, cip, cop, rows): the GEMM's N = cip (the channels of Y1 / dY1), K =
# cop. H * W is odd: an image boundary falls inside a tile, where the dropout
# mask row changes.
BNBWD_CASES = [(2, 181, 181, 128, 64, 128),     # 128x128
               (2, 181, 181, 64, 32, 128),      # 128x64
               (2, 511, 513, 64, 32, 256),      # 256x64
               (2, 511, 513, 32, 64, 256)]      # 256x32


def bnbwd_case(ops, device, B, H, W, cip, cop):
    def make():
        g = U.gen(B, H, W, cip, cop, 44)
        y1 = U16.normal_values((B, cip, H, W), g, "f32")
        dy2 = U16.normal_values((B, cop, H, W), g, "f32")
        w2 = torch.randn(cop, cip, 1, 1, generator=g) / cip ** 0.5
        st, v = bn_vectors(cip, g, device, ops)
        mask = drop_mask(B, cip, g)
        dA1, SA = U.dgrad_ref(dy2, w2), U.dgrad_ref(dy2, w2, absval=True)
        dz, xhat, S1, S2, unsure = bn_bwd_ref(dA1, y1, v, mask)
        c = (1, -1, 1, 1)
        z = y1.double() * v.scale.double().view(c) + v.shift.double().view(c)
        f = torch.where(z > 0, 1.0, 0.2) * mask.double()[:, :, None, None]     # dz = dA1 f
        del z, dA1
        ym = y1.double() - v.mean.double().view(c)
        big = {n: t.to(device) for n, t in dict(SA=SA, dz=dz, xhat=xhat, f=f, unsure=unsure, ym=ym).items()}
        return dict(y1=y1, dy2=dy2, w2=w2, st=st, v=v, mask=mask, S1=S1, S2=S2, **big)
    return cached(("bnbwd", B, H, W, cip, cop), make)


@pytest.mark.parametrize("with_amax", [False, True])
@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("B,H,W,cip,cop,rows", BNBWD_CASES)
def test_conv1x1_dgrad_bn_bwd(ops, device, B, H, W, cip, cop, rows, recompute, with_amax):
    """dY1 element-wise, dgamma / dbeta / the previous conv's bias gradient
    against float64 sums, the partial-row count and the recorded max|dY1|.
    In the default mode the GEMM runs the f16x2 split with the maxima and the
    bf16 split without them. The float64 reference is computed once per shape
    on the CPU; its large tensors are kept on the device, where the
    comparisons run (plain float64 torch)."""
    from nsm_amd._lib import lib
    M = B * H * W
    assert lib.nsm_conv_stat_rows(B, H, W, cip) == rows
    assert lib.nsm_conv1x1_bnbwd_chunks(B, H, W, cip, cop, ops.NSM_F32) == -(-M // rows)
    assert (H * W) % rows != 0
    r = bnbwd_case(ops, device, B, H, W, cip, cop)
    v, f, dz, xhat, unsure, ym = r["v"], r["f"], r["dz"], r["xhat"], r["unsure"], r["ym"]
    ops.set_f32_split(2)
    yd, dyd = E.nhwc(r["y1"]).to(device), E.nhwc(r["dy2"]).to(device)
    wd = ops.pack_conv_weight(r["w2"].to(device), cop, cip, ops.PACK_DGRAD)
    am, mode, floor = (None, None), 1, None
    if with_amax:
        am, mode = (ops.absmax(dyd), ops.absmax(wd)), 2
        assert slot_value(am[0]) == r["dy2"].abs().max().item()
        floor = U.dgrad_floor(r["dy2"], r["w2"], slot_value(am[0]), slot_value(am[1])).to(device)
    out_slot = ops.amax_slots(1, device)
    dg, db, dbias = (torch.full((cip,), float("nan"), device=device) for _ in range(3))
    dy1 = ops.conv1x1_dgrad_bn_bwd(dyd, B, H, W, wd, yd, r["st"], r["mask"].to(device), cip, dg, db, dbias,
                                   recompute, amax=am, amax_out=out_slot)
    case_id = sid(B, H, W, cip, cop, "rc%d" % recompute, "amax%d" % with_amax)
    # the recorded maximum is that of the stored tensor, bit for bit
    assert slot_value(out_slot) == dy1.abs().max().item()

    bz = f.abs() * U.gemm_bound(mode, r["SA"], cop, floor=floor)       # the bound of dz
    dg, db, dbias = dg.cpu().double(), db.cpu().double(), dbias.cpu().double()
    for name, got, ref, bound in (("dbeta", db, r["S1"], U.sum_bound(bz, dz, unsure)),
                                  ("dgamma", dg, r["S2"], U.sum_bound(bz * xhat.abs(), dz * xhat, unsure))):
        check("bn_param_grads", case_id + "-" + name, got, ref, bound.cpu())
    c = (1, -1, 1, 1)
    k1 = (v.gamma * v.invstd).double()                                  # the fp32 product of the finalize
    k2 = -v.gamma.double() * v.invstd.double() ** 2 * dg / M
    k3 = -k1 * db / M
    # the bias of the conv before a train-mode BN has no gradient: k1 S1 + k3 M
    # cancels up to the rounding of k3 (and of the stored float)
    check("bn_param_grads", case_id + "-dbias_prev", dbias, torch.zeros(cip, dtype=torch.float64),
          2 * U.E32 * (k1.abs() * db.abs() + k3.abs() * M) + 1e-300)
    k1d, k2d, k3d = (t.to(device).view(c) for t in (k1, k2, k3))
    t1, t2 = k1d * dz, k2d * ym
    ref = t1 + t2 + k3d
    bound = k1d.abs() * bz + U16.OPS["bn_bwd_apply"] * U.E32 * (t1.abs() + t2.abs() + k3d.abs())
    assert unsure.double().mean().item() <= 1e-3
    check("conv1x1_dgrad_bnbwd", case_id, nchw(dy1, B, H, W), ref, bound, keep=~unsure)
