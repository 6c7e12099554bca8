"""GPU: the kernels of the 16-bit train step one by one, in f16 storage (the
fp16-autocast mode) and, where it costs nothing, in bf16: the train forward
with its fused BN partials on every tile of dispatch_conv_fwd_b, the prologue
1x1, the input gradients, nsm_conv_wgrad_f16 / _bf16 on every tile of
wgrad_dma_tile / dispatch_wgrad_b, nsm_conv1x1_dgrad_bnbwd with f16 storage,
the elementwise ops, and the f16-only edges (ties to even, gradual underflow,
overflow to +-Inf), each against the float64 restatement of f16_util.py under
its element-wise worst-case bounds (stated there; none measured on the
kernels). The worst err / bound of every family goes to parity_margins.json as
f16_ops.<family>."""
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.nn.functional as F

import eval_util as E
import f16_util as U
from test_gpu_eval_ops import check_partials, storage
from test_gpu_ops import nchw, rel
from util import record_margin

pytestmark = pytest.mark.gpu
torch.set_num_threads(16)
FMTS = ["f16", "bf16"]
# NSM_RESIZE_SEP=2 (read once per process): the separable resize forms in 16-bit
# storage too; test_separable_forms_in_a_child_process runs the resize tests so
SEP16 = os.environ.get("NSM_RESIZE_SEP") == "2"
MARGIN_KEY = "f16_ops_sep." if SEP16 else "f16_ops."


@pytest.fixture(scope="module")
def ops(device):
    from nsm_amd import ops as O
    return O


# ---- helpers -------------------------------------------------------------------
_WORST = {}


def margin(family, case_id, ratio):
    """Keep the worst error / bound of a kernel family in parity_margins.json."""
    if ratio >= _WORST.get(family, (-1.0, None))[0]:
        _WORST[family] = (float(ratio), case_id)
        record_margin(MARGIN_KEY + family, worst_err_over_bound=float(ratio), case=case_id)


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
    """One float64 reference at a time, shared by the consecutive tests on it."""
    if key not in _REF:
        _REF.clear()
        _REF[key] = make()
    return _REF[key]


def conv_case(B, H, W, ci, co, k, fmt, regime="normal"):
    """(case, ref [M, co], S [M, co]) float64 of the forward convolution."""
    def make():
        if regime == "normal":
            case = E.make_case(B, H, W, ci, co, k, fmt=fmt)
        elif regime == "grad":
            case = U.make_grad_case(B, H, W, ci, co, k, fmt)
            case.b = None
        elif regime == "tiny":
            case = U.make_tiny_case(B, H, W, ci, co, k)
        else:
            case = U.make_overflow_case(B, H, W, ci, co, k)
        return (case, E.nhwc(U.conv_ref(case.x, case.w, case.b)),
                E.nhwc(U.conv_ref(case.x, case.w, case.b, absval=True)))
    return cached(("conv", B, H, W, ci, co, k, fmt, regime), make)


def run_conv_fwd_bn(ops, device, case, fmt, stats=True):
    sdt, store, load = storage(ops, fmt, device)
    wp = ops.pack_conv_weight(case.w.to(device), case.co, case.ci, ops.PACK_FWD, sdt)
    y, part = ops.conv_fwd_bn(store(E.nhwc(case.x)), case.B, case.H, case.W, wp,
                              None if case.b is None else case.b.to(device), case.co, case.k,
                              stats=stats)
    assert y.dtype == sdt
    return load(y), part


def sid(*s):
    return "x".join(str(v) for v in s)


def to_dev(ops, fmt, device, t):
    """NCHW float32 (representable) -> device NHWC storage."""
    return storage(ops, fmt, device)[1](E.nhwc(t))


def from_dev(ops, fmt, device, t, B, H, W):
    """device NHWC storage -> float64 NCHW."""
    return nchw(storage(ops, fmt, device)[2](t), B, H, W)


def values(shape, g, fmt, regime="normal"):
    if regime == "grad" and fmt == "f16":
        return U.grad_values(shape, g, fmt)
    return U.normal_values(shape, g, fmt)


def bn_vectors(C, g, device, ops):
    """A BNState with consistent vectors (scale = gamma invstd, shift = beta -
    mean scale, mixed-sign gamma) and their CPU copies."""
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    beta, mean = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5
    invstd = torch.pow(2.0, torch.rand(C, generator=g) * 2 - 1)
    scale = gamma * invstd
    shift = beta - mean * scale
    st = ops.BNState(C, device)
    for name, v in (("scale", scale), ("shift", shift), ("mean", mean), ("invstd", invstd)):
        getattr(st, name).copy_(v)
    st.gamma = gamma.to(device)
    return st, types.SimpleNamespace(gamma=gamma, beta=beta, mean=mean, invstd=invstd, scale=scale,
                                     shift=shift)


def drop_mask(B, C, g):
    return (torch.rand(B, C, generator=g) > 0.2).float() / 0.8


# ---- a. conv_fwd_bn: the train forward and its fused BN partials -------------------
FWD_SHAPES = ([s + (64,) for s in E.SMALL] + E.S16_LARGE
              + [(1, 239, 257, 64, 256, 3, 256),     # 3x3 on the 256x256 LDS-DMA tile (cm walk)
                 (1, 351, 350, 128, 128, 3, 256)])   # 3x3 on the 512x128 tile, two 64-channel chunks


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,H,W,ci,co,k,rows", FWD_SHAPES)
def test_conv_fwd_bn(ops, device, B, H, W, ci, co, k, rows, fmt):
    from nsm_amd._lib import lib
    assert lib.nsm_conv_stat_rows_bf16(B, H, W, co) == rows
    case, ref, S = conv_case(B, H, W, ci, co, k, fmt)
    y, part = run_conv_fwd_bn(ops, device, case, fmt)
    assert part.rpc == rows and part.nchunk == -(-(B * H * W) // rows)
    check(f"conv_fwd_bn_{fmt}", sid(B, H, W, ci, co, k), y, ref, U.gemm_bound(ref, S, k * k * ci, fmt))
    check_partials(part, y, co)


# ---- b. the prologue 1x1 ------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,H,W,ci,co", [(2, 6, 7, 32, 64), (2, 16, 16, 128, 64),
                                         (1, 511, 513, 32, 64)])   # 256x64 register tile
def test_conv1x1_prologue(ops, device, B, H, W, ci, co, fmt):
    """BN-apply + LeakyReLU + Dropout2d in the operand loader: the reference
    rounds the activated operand to storage as the loader does; where the
    loader's fp32 arithmetic may round an operand element to the neighbouring
    storage value (prologue_ref's d), that step times |w| joins the bound."""
    sdt, store, load = storage(ops, fmt, device)
    g = U.gen(B, H, W, ci, co, 21)
    y1 = U.normal_values((B, ci, H, W), g, fmt)
    sc = (torch.rand(ci, generator=g) + 0.5) * torch.where(torch.rand(ci, generator=g) < 0.25, -1.0, 1.0)
    sh = torch.randn(ci, generator=g)
    mask = drop_mask(B, ci, g)
    w = E.rounder(fmt)(torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5)
    a, d = U.prologue_ref(y1, sc, sh, mask, fmt)
    ref, S = E.nhwc(U.conv_ref(a, w, None)), E.nhwc(U.conv_ref(a, w, None, absval=True))
    bound = U.gemm_bound(ref, S, ci, fmt) + E.nhwc(U.conv_ref(d, w, None, absval=True))
    wp = ops.pack_conv_weight(w.to(device), co, ci, ops.PACK_FWD, sdt)
    y = ops.conv_fwd(store(E.nhwc(y1)), B, H, W, wp, None, co, 1,
                     pro=(sc.to(device), sh.to(device), mask.to(device)))
    check(f"conv1x1_prologue_{fmt}", sid(B, H, W, ci, co), load(y), ref, bound)


# ---- c. the input gradients ---------------------------------------------------------
DGRAD_SHAPES = E.SMALL + [(1, 239, 257, 256, 64, 3),   # dx with 256 channels from 64
                          (1, 209, 313, 32, 32, 3)]    # 128x32 LDS-DMA tiles


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,H,W,ci,co,k", DGRAD_SHAPES)
def test_conv_dgrad(ops, device, B, H, W, ci, co, k, fmt):
    """PACK_DGRAD, bias None: dx = conv_transpose(dy, w); dy in the grad regime for f16."""
    sdt, store, load = storage(ops, fmt, device)
    g = U.gen(B, H, W, ci, co, k, 31)
    w = E.rounder(fmt)(torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5)
    dy = values((B, co, H, W), g, fmt, "grad")
    ref, S = E.nhwc(U.dgrad_ref(dy, w)), E.nhwc(U.dgrad_ref(dy, w, absval=True))
    wd = ops.pack_conv_weight(w.to(device), co, ci, ops.PACK_DGRAD, sdt)
    dx = ops.conv_fwd(store(E.nhwc(dy)), B, H, W, wd, None, ci, k)
    check(f"conv_dgrad_{fmt}", sid(B, H, W, ci, co, k), load(dx), ref,
          U.gemm_bound(ref, S, k * k * co, fmt))


# ---- d. conv_wgrad on every tile ----------------------------------------------------
# (B, H, W, cin, cout, k, pro, cin_real, cout_real)
WGRAD_CASES = [(2, 37, 41, ci, co, k, pro, ci, co) for ci, co, k, pro in [
    (32, 32, 3, False),      # 32x128 multi-tap
    (64, 64, 3, False),      # 64x256
    (128, 128, 3, False),    # 128x384
    (256, 256, 3, False),    # 256x256
    (128, 256, 1, False),    # 256x128
    (128, 128, 1, False),    # 128x128
    (64, 128, 1, False),     # 64x64
    (32, 64, 3, False),      # register, shifted loader
    (32, 64, 1, True),       # register, prologue
    (128, 512, 1, True)]]    # register, prologue
WGRAD_CASES.insert(8, (2, 37, 41, 96, 64, 3, False, 90, 60))   # register, cin no multiple of 64; pads
WGRAD_CASES.append((1, 133, 135, 64, 64, 3, False, 64, 64))    # > 16 splits: two-level slab sum
# 96 input channels of a 1x1 (the planned 64-column tile fits neither way: 32 columns), plain and prologue
WGRAD_CASES += [(2, 37, 41, 96, 64, 1, False, 96, 64), (2, 37, 41, 96, 64, 1, True, 96, 64)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,H,W,cip,cop,k,pro,ci,co", WGRAD_CASES)
def test_conv_wgrad(ops, device, B, H, W, cip, cop, k, pro, ci, co, fmt):
    """dw [co, ci, k, k] in fp32 against float64, per element; dy in the grad
    regime for f16. ops.conv_wgrad passes exactly nsm_conv_wgrad_bf16_ws
    floats of workspace, so a query below the call's need fails the call."""
    from nsm_amd._lib import lib
    sdt, store, load = storage(ops, fmt, device)
    g = U.gen(B, H, W, cip, cop, k, 41)
    x = F.pad(U.normal_values((B, ci, H, W), g, fmt), (0, 0, 0, 0, 0, cip - ci))
    dy = F.pad(values((B, co, H, W), g, fmt, "grad"), (0, 0, 0, 0, 0, cop - co))
    extra = 0.0
    if pro:
        sc = (torch.rand(cip, generator=g) + 0.5) * torch.where(torch.rand(cip, generator=g) < 0.25, -1.0, 1.0)
        sh = torch.randn(cip, generator=g)
        mask = drop_mask(B, cip, g)
        a, d = U.prologue_ref(x, sc, sh, mask, fmt)
        extra = U.wgrad_ref(d, dy, k, absval=True)[:co, :ci]
    else:
        a = x
    ref = U.wgrad_ref(a, dy, k)[:co, :ci]
    S = U.wgrad_ref(a, dy, k, absval=True)[:co, :ci]
    if (B, H, W) == (1, 133, 135):
        assert lib.nsm_conv_wgrad_bf16_ws(B, H, W, cip, cop, k) // (cop * k * k * cip) > 16
    dw = torch.full((co, ci, k, k), float("nan"), device=device)
    ops.conv_wgrad(store(E.nhwc(dy)), store(E.nhwc(x)), B, H, W, k, ci, co, dw,
                   pro=(sc.to(device), sh.to(device), mask.to(device)) if pro else None)
    check(f"conv_wgrad_{fmt}", sid(B, H, W, cip, cop, k, int(pro)), dw.cpu(), ref,
          U.wgrad_bound(S, B * H * W) + extra + 1e-300)


# ---- e. conv1x1_dgrad_bn_bwd, f16 storage --------------------------------------------
@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("B,H,W,cip,cop,drop", [(2, 9, 11, 32, 64, True), (2, 16, 16, 64, 32, False),
                                                (2, 16, 16, 128, 64, True), (1, 32, 32, 512, 128, True)])
def test_conv1x1_dgrad_bn_bwd_f16(ops, device, B, H, W, cip, cop, drop, recompute):
    """Against float64 autograd of conv1x1(lrelu(BN(y1)) * mask); the bf16
    tolerances of test_gpu_ops.test_conv1x1_dgrad_bn_bwd times 2^-3, the ratio
    of the unit roundoffs (the same two storage roundings)."""
    _, store, load = storage(ops, "f16", device)
    rnd = E.rounder("f16")
    g = torch.Generator().manual_seed(B * H + cip + cop)
    y1 = rnd(torch.randn(B, cip, H, W, generator=g) * 1.5 + 0.3)
    w2 = rnd(torch.randn(cop, cip, 1, 1, generator=g) / cip ** 0.5)
    dy2 = rnd(torch.randn(B, cop, H, W, generator=g))
    gamma = torch.rand(cip, generator=g) + 0.5
    beta = torch.randn(cip, generator=g) * 0.2
    mask = drop_mask(B, cip, g) if drop else None
    yr = y1.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    a = F.leaky_relu(F.batch_norm(yr, None, None, gr, br, training=True), 0.2)
    if drop:
        a = a * mask.double()[:, :, None, None]
    F.conv2d(a, w2.double()).backward(dy2.double())

    bn = torch.nn.BatchNorm2d(cip).to(device)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    yd = store(E.nhwc(y1))
    st = ops.bn_train(yd, bn, cip, 0.1, 1e-5)
    wd = ops.pack_conv_weight(w2.to(device), cop, cip, ops.PACK_DGRAD, ops.F16S)
    dyd = store(E.nhwc(dy2))
    md = mask.to(device) if drop else None
    outs = {}
    for fused in (True, False):
        dg, db, dbias = (torch.empty(cip, device=device) for _ in range(3))
        if fused:
            dy1 = ops.conv1x1_dgrad_bn_bwd(dyd, B, H, W, wd, yd, st, md, cip, dg, db, dbias, recompute)
        else:
            dA1 = ops.conv_fwd(dyd, B, H, W, wd, None, cip, 1)
            dy1 = ops.bn_bwd(dA1, yd, st, H * W, md, cip, dg, db, dbias)
        assert dy1.dtype == ops.F16S
        outs[fused] = (nchw(load(dy1), B, H, W), dg.cpu(), db.cpu(), dbias.cpu())
    tol, worst = 2.5e-3, 0.0
    for fused in (True, False):
        dy1, dg, db, dbias = outs[fused]
        rs = (rel(dy1, yr.grad), rel(dg, gr.grad), rel(db, br.grad))
        print(f"fused {fused}: rel dy1 {rs[0]:.2e} dgamma {rs[1]:.2e} dbeta {rs[2]:.2e}")
        worst = max(worst, max(rs) / tol)
        assert max(rs) <= tol, (fused, rs)
        assert dbias.abs().max().item() <= 1e-3 * max(1.0, br.grad.abs().max().item())
    d = rel(outs[True][0], outs[False][0])
    margin("conv1x1_dgrad_bn_bwd_f16", sid(B, H, W, cip, cop, int(recompute)), max(worst, d / 5e-4))
    assert d <= 5e-4
    assert rel(outs[True][1], outs[False][1]) <= 1e-5
    assert rel(outs[True][2], outs[False][2]) <= 1e-5


# ---- f. the elementwise ops ------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M,C", [(7, 32), (1000, 64), (4096 * 8 + 3, 128)])
def test_bn_partials_and_train(ops, device, M, C, fmt):
    """bn_stats partials (check_partials on the stored values) and the
    finalized batch statistics against float64 (test_bn_train_stats' bounds)."""
    _, store, _ = storage(ops, fmt, device)
    y = E.rounder(fmt)(torch.randn(M, C, generator=U.gen(M, C)) * 3 + 5)
    yd = store(y)
    check_partials(ops.bn_partials(yd), y.double(), C)
    bn = torch.nn.BatchNorm2d(C).to(device)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.1, 0.1)
    st = ops.bn_train(yd, bn, C, 0.1, 1e-5)
    mean, var_b = y.double().mean(0), y.double().var(0, unbiased=False)
    inv = 1 / (var_b + 1e-5).sqrt()
    assert (st.mean.cpu().double() - mean).abs().max() <= 1e-5 * 5
    assert (st.invstd.cpu().double() - inv).abs().max() <= 1e-5
    sc = bn.weight.detach().cpu().double() * inv
    assert (st.scale.cpu().double() - sc).abs().max() <= 2e-5
    assert (st.shift.cpu().double() - (bn.bias.detach().cpu().double() - mean * sc)).abs().max() <= 2e-4
    assert (bn.running_mean.cpu().double() - 0.1 * mean).abs().max() <= 1e-5
    if M > 1:
        var_u = y.double().var(0, unbiased=True)
        assert (bn.running_var.cpu().double() - (0.9 + 0.1 * var_u)).abs().max() <= 1e-4


# C = 40: C / 8 = 5 does not divide 256, so pix_launch picks a 255-thread block
ACT_SHAPES = [(2, 6, 5, 64), (1, 9, 7, 128), (2, 33, 35, 32), (2, 5, 7, 40)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,H,W,C", ACT_SHAPES)
def test_bn_act(ops, device, B, H, W, C, fmt):
    g = U.gen(B, H, W, C, 51)
    y, res = U.normal_values((B, C, H, W), g, fmt), U.normal_values((B, C, H, W), g, fmt)
    st, v = bn_vectors(C, g, device, ops)
    mask = drop_mask(B, C, g)
    yd, rd = to_dev(ops, fmt, device, y), to_dev(ops, fmt, device, res)
    for tag, kw, rkw in (("plain", {}, {}), ("skip", dict(res=rd), dict(res=res)),
                         ("mask", dict(mask=mask.to(device), HW=H * W), dict(mask=mask)),
                         ("skip_mask", dict(res=rd, mask=mask.to(device), HW=H * W),
                          dict(res=res, mask=mask))):
        z, _, bound = U.bn_act_ref(y, v.scale, v.shift, fmt, **rkw)
        out = ops.bn_act(yd, st, 0.2, **kw)
        check(f"bn_act_{fmt}", sid(B, H, W, C) + "-" + tag, from_dev(ops, fmt, device, out, B, H, W),
              z, bound)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,H,W,C", [(2, 16, 18, 64), (1, 9, 7, 128), (2, 5, 9, 512), (2, 5, 7, 40)])
def test_bn_act_pool(ops, device, B, H, W, C, fmt):
    """z as bn_act; the pooled output is the mean of the stored z: its bound
    carries the propagated bound of z."""
    g = U.gen(B, H, W, C, 52)
    y = U.normal_values((B, C, H, W), g, fmt)
    st, v = bn_vectors(C, g, device, ops)
    z, _, bz = U.bn_act_ref(y, v.scale, v.shift, fmt)
    zd, pd = ops.bn_act_pool(to_dev(ops, fmt, device, y), st, B, H, W, 0.2)
    check(f"bn_act_pool_{fmt}", sid(B, H, W, C) + "-z", from_dev(ops, fmt, device, zd, B, H, W), z, bz)
    p = U.avgpool_ref(z)
    bound = U.elem_bound(p, U.avgpool_ref(z, absval=True), "avgpool2", fmt, extra=U.avgpool_ref(bz))
    check(f"bn_act_pool_{fmt}", sid(B, H, W, C) + "-pooled",
          from_dev(ops, fmt, device, pd, B, H // 2, W // 2), p, bound)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("H,W", [(8, 8), (7, 9), (135, 240)])
def test_avgpool(ops, device, H, W, fmt):
    B, C = 2, 16
    g = U.gen(H, W, 53)
    x = U.normal_values((B, C, H, W), g, fmt)
    p = U.avgpool_ref(x)
    got = ops.avgpool2(to_dev(ops, fmt, device, x), B, H, W)
    check(f"avgpool2_{fmt}", sid(H, W), from_dev(ops, fmt, device, got, B, H // 2, W // 2), p,
          U.elem_bound(p, U.avgpool_ref(x, absval=True), "avgpool2", fmt))
    dy = values((B, C, H // 2, W // 2), g, fmt, "grad")
    skip = values((B, C, H, W), g, fmt, "grad")
    ref = U.avgpool_bwd(dy, H, W) + skip.double()
    A = U.avgpool_bwd(dy.abs(), H, W) + skip.double().abs()
    dx = ops.avgpool2_bwd_add(to_dev(ops, fmt, device, dy), B, H, W, to_dev(ops, fmt, device, skip))
    check(f"avgpool2_bwd_add_{fmt}", sid(H, W), from_dev(ops, fmt, device, dx, B, H, W), ref,
          U.elem_bound(ref, A, "avgpool2_bwd_add", fmt))


def _resample_pair(ops, device, fmt, kind, B, C, hi, wi, ho, wo, g, fam):
    """forward and backward of one resampler against the weight matrices."""
    wy, wx = U.resize_mats(hi, wi, ho, wo) if kind == "resize" else U.up2_mats(hi, wi, ho, wo)
    fwd, bwd = ((ops.resize, ops.resize_bwd) if kind == "resize"
                else (ops.up2_resize, ops.up2_resize_bwd))
    x = U.normal_values((B, C, hi, wi), g, fmt)
    ref = U.resample(x, wy, wx)
    got = fwd(to_dev(ops, fmt, device, x), B, hi, wi, ho, wo)
    check(f"{fam}_{fmt}", sid(B, C, hi, wi, ho, wo), from_dev(ops, fmt, device, got, B, ho, wo), ref,
          U.elem_bound(ref, U.resample(x, wy, wx, absval=True), fam, fmt))
    dy = values((B, C, ho, wo), g, fmt, "grad")
    ref = U.resample(dy, wy.t(), wx.t())
    dx = bwd(to_dev(ops, fmt, device, dy), B, hi, wi, ho, wo)
    check(f"{fam}_bwd_{fmt}", sid(B, C, hi, wi, ho, wo), from_dev(ops, fmt, device, dx, B, hi, wi), ref,
          U.elem_bound(ref, U.resample(dy, wy.t(), wx.t(), absval=True), fam + "_bwd", fmt))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("Hi,Wi,Ho,Wo", [(4, 5, 8, 10), (8, 10, 4, 5), (67, 120, 134, 240)])
def test_resize(ops, device, Hi, Wi, Ho, Wo, fmt):
    _resample_pair(ops, device, fmt, "resize", 2, 8, Hi, Wi, Ho, Wo, U.gen(Hi, Wi, Ho, Wo, 54), "resize")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,C,Hi,Wi,Ho,Wo", [
    (6, 1, 5, 7, 4, 6),          # C % 8 != 0: the scalar kernels (ld1 / st1), the odd-size input guard
    (1, 8, 2, 2050, 4, 4100)])   # rows wider than the row-blocked backward's LDS tables: the gather
def test_resize_other_kernels(ops, device, B, C, Hi, Wi, Ho, Wo, fmt):
    """The 16-bit instantiations no shape of the fp32 lists reaches."""
    _resample_pair(ops, device, fmt, "resize", B, C, Hi, Wi, Ho, Wo, U.gen(Hi, Wi, Ho, Wo, 54), "resize")


# (8, 10, 7, 9): the second step shrinks below the source grid, so the forward
# takes the per-element kernel; (2, 2050, 4, 4100): the gather backward
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,h,w,th,tw", [(2, 2, 4, 5, 9), (2, 5, 7, 5, 7), (2, 67, 120, 135, 240),
                                         (2, 8, 10, 7, 9), (1, 2, 2050, 4, 4100)])
def test_up2_resize(ops, device, B, h, w, th, tw, fmt):
    _resample_pair(ops, device, fmt, "up2", B, 8, h, w, th, tw, U.gen(h, w, th, tw, 55), "up2_resize")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,H,W,C", [(2, 16, 18, 64), (1, 9, 7, 128)])
def test_resize_act(ops, device, B, H, W, C, fmt):
    """The lazy resamplers: every tap is z = r(lrelu(y scale + shift) + res),
    rounded as bn_act stores it, so the bound carries z's bound through the
    (non-negative) resampling weights."""
    g = U.gen(B, H, W, C, 56)
    y, res = U.normal_values((B, C, H, W), g, fmt), U.normal_values((B, C, H, W), g, fmt)
    st, v = bn_vectors(C, g, device, ops)
    z, _, bz = U.bn_act_ref(y, v.scale, v.shift, fmt, res=res)
    lazy = ops.Lazy(to_dev(ops, fmt, device, y), st, to_dev(ops, fmt, device, res))
    for fam, (wy, wx), (ho, wo), fn in (
            ("resize", U.resize_mats(H, W, 2 * H, 2 * W), (2 * H, 2 * W), ops.resize_act),
            ("up2_resize", U.up2_mats(H, W, 2 * H - 1, 2 * W - 1), (2 * H - 1, 2 * W - 1),
             ops.up2_resize_act)):
        got = fn(lazy, B, H, W, ho, wo, 0.2)
        assert got is not None
        ref = U.resample(z, wy, wx)
        bound = U.elem_bound(ref, U.resample(z, wy, wx, absval=True), fam, fmt,
                             extra=U.resample(bz, wy, wx, absval=True))
        check(f"{fam}_act_{fmt}", sid(B, H, W, C), from_dev(ops, fmt, device, got, B, ho, wo), ref, bound)


def test_separable_forms_in_a_child_process():
    """By default only fp32 takes the separable resize kernels; the knob that
    gives them to 16-bit storage is read once per process. A child process
    with NSM_RESIZE_SEP=2 runs the resize tests of this file (resize, the
    composite, the Lazy forms, the fused BN reduction; f16 and bf16) against
    their own float64 references and bounds, which hold for either form."""
    if SEP16:
        return                                   # the child itself
    tests = ["test_resize", "test_up2_resize", "test_resize_act", "test_grad_producer_bnred"]
    env = dict(os.environ, NSM_RESIZE_SEP="2")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider"]
                       + [f"{__file__}::{t}" for t in tests], env=env, capture_output=True,
                       text=True, timeout=600, cwd=os.path.dirname(os.path.dirname(__file__)))
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout


def bn_bwd_ref(g_, y, v, mask):
    """float64 (dz, xhat, S1, S2, unsure) of the BN + LeakyReLU (+ mask)
    backward's reduction, NCHW; unsure: the elements whose pre-activation lies
    within its fp32 error of 0 (the derivative's branch is not determined)."""
    c = (1, -1, 1, 1)
    t = y.double() * v.scale.double().view(c)
    z = t + v.shift.double().view(c)
    unsure = z.abs() <= 4 * U.E32 * (t.abs() + v.shift.double().abs().view(c))
    dz = g_.double() * torch.where(z > 0, 1.0, 0.2)
    if mask is not None:
        dz = dz * mask.double()[:, :, None, None]
    xhat = (y.double() - v.mean.double().view(c)) * v.invstd.double().view(c)
    return dz, xhat, dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3)), unsure


def close_sums(got, ref, second):
    """check_partials' tolerances (sum: rtol 1e-4, centred / weighted sum: 1e-3; atol 1e-2)."""
    torch.testing.assert_close(got.double(), ref, rtol=1e-3 if second else 1e-4, atol=1e-2)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,H,W,C", ACT_SHAPES)
def test_bn_bwd(ops, device, B, H, W, C, fmt):
    """reduce + finalize: dgamma / dbeta against the float64 sums; apply: dy
    element-wise, its coefficients from the dgamma / dbeta the device wrote (the
    reduction has its own check), the undetermined-branch elements left out."""
    g = U.gen(B, H, W, C, 57)
    y = U.normal_values((B, C, H, W), g, fmt)
    gz = values((B, C, H, W), g, fmt, "grad")
    st, v = bn_vectors(C, g, device, ops)
    mask = drop_mask(B, C, g)
    dz, xhat, S1, S2, unsure = bn_bwd_ref(gz, y, v, mask)
    dg, db, dbias = (torch.empty(C, device=device) for _ in range(3))
    dy = ops.bn_bwd(to_dev(ops, fmt, device, gz), to_dev(ops, fmt, device, y), st, H * W,
                    mask.to(device), C, dg, db, dbias)
    close_sums(db.cpu(), S1, False)
    close_sums(dg.cpu(), S2, True)
    assert dbias.abs().max().item() <= 1e-3 * max(1.0, S1.abs().max().item())
    M = B * H * W
    c = (1, -1, 1, 1)
    k1 = (v.gamma.double() * v.invstd.double()).view(c)
    k2 = (-v.gamma.double() * v.invstd.double() ** 2 * dg.cpu().double() / M).view(c)
    k3 = (-k1.view(-1) * db.cpu().double() / M).view(c)
    ym = y.double() - v.mean.double().view(c)
    ref = k1 * dz + k2 * ym + k3
    A = (k1 * dz).abs() + (k2 * ym).abs() + k3.abs()
    assert unsure.double().mean().item() <= 1e-3
    check(f"bn_bwd_apply_{fmt}", sid(B, H, W, C), from_dev(ops, fmt, device, dy, B, H, W), ref,
          U.elem_bound(ref, A, "bn_bwd_apply", fmt), keep=~unsure)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind,B,h,w,C", [("pool", 2, 16, 18, 64), ("pool", 3, 9, 7, 1024),
                                          ("resize", 2, 8, 10, 128), ("resize", 1, 33, 20, 512),
                                          ("up2", 2, 16, 16, 64), ("up2", 1, 67, 120, 32)])
def test_grad_producer_bnred(ops, device, kind, B, h, w, C, fmt):
    """The three gradient producers with the next BN's backward reduction
    fused: the gradient against float64, and the partials' totals against the
    float64 sums over the stored gradient."""
    g = U.gen(B, h, w, C, 58)
    y2 = U.normal_values((B, C, h, w), g, fmt)
    st, v = bn_vectors(C, g, device, ops)
    bnred = (to_dev(ops, fmt, device, y2), st)
    if kind == "pool":
        dy, skip = values((B, C, h // 2, w // 2), g, fmt, "grad"), values((B, C, h, w), g, fmt, "grad")
        ref = U.avgpool_bwd(dy, h, w) + skip.double()
        A, fam = U.avgpool_bwd(dy.abs(), h, w) + skip.double().abs(), "avgpool2_bwd_add"
        G, part = ops.avgpool2_bwd_add(to_dev(ops, fmt, device, dy), B, h, w,
                                       to_dev(ops, fmt, device, skip), bnred=bnred)
    else:
        th, tw = (2 * h, 2 * w) if kind == "resize" else (2 * h - 1, 2 * w + 3)
        wy, wx = U.resize_mats(h, w, th, tw) if kind == "resize" else U.up2_mats(h, w, th, tw)
        dy = values((B, C, th, tw), g, fmt, "grad")
        ref, A = U.resample(dy, wy.t(), wx.t()), U.resample(dy, wy.t(), wx.t(), absval=True)
        fam = "resize_bwd" if kind == "resize" else "up2_resize_bwd"
        fn = ops.resize_bwd if kind == "resize" else ops.up2_resize_bwd
        G, part = fn(to_dev(ops, fmt, device, dy), B, h, w, th, tw, bnred=bnred)
    assert part is not None
    Gs = from_dev(ops, fmt, device, G, B, h, w)
    check(f"{fam}_bnred_{fmt}", sid(B, h, w, C), Gs, ref, U.elem_bound(ref, A, fam, fmt))
    _, _, S1, S2, _ = bn_bwd_ref(Gs, y2, v, None)
    buf, n = part
    tot = buf.view(n, 2, C).cpu().double().sum(0)
    close_sums(tot[0], S1, False)
    close_sums(tot[1], S2, True)


@pytest.mark.parametrize("fmt", FMTS)
def test_boundary_converters(ops, device, fmt):
    """input_prep / input_grad and the NCHW <-> NHWC converters in 16-bit
    storage: one rounding to nearest even of each fp32 value, nothing else
    (bitwise), the pad channels zero."""
    from nsm_amd.unet import _nchw, _nhwc
    sdt, _, load = storage(ops, fmt, device)
    rnd = E.rounder(fmt)
    B, C, H, W = 2, 7, 6, 10
    g = U.gen(B, C, H, W, 59)
    x = torch.randn(B, C, H, W, generator=g) * torch.pow(2.0, torch.rand(B, C, H, W, generator=g) * 30 - 26)
    X = ops.input_prep(x.to(device), 32, dtype=sdt)
    assert X.dtype == sdt
    want = E.nhwc(F.pixel_unshuffle(rnd(x), 2)).double()
    assert torch.equal(load(X)[:, :28], want) and load(X)[:, 28:].abs().max().item() == 0
    assert torch.equal(ops.input_grad(X, B, C, H, W).cpu(), rnd(x))
    for cp in (32, 64):
        Z = _nhwc(x.to(device), cp, sdt)
        assert Z.dtype == sdt and Z.shape == (B * H * W, cp)
        assert torch.equal(load(Z)[:, :C], E.nhwc(rnd(x)).double())
        assert load(Z)[:, C:].abs().max().item() == 0
        assert torch.equal(_nchw(Z, B, C, H, W).cpu(), rnd(x))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,Rh,Rw", [(2, 5, 6), (1, 67, 120)])
def test_head(ops, device, B, Rh, Rw, fmt):
    """conv10 + pixel_shuffle + sigmoid on a 16-bit z (fp32 out: 18 fp32
    operations on the logit through sigmoid' <= 1/4, plus 8 e32 for expf and
    the division); head_bwd's dz (stored 16-bit) from the out the device
    wrote, dw10 / db10 (fp32 sums) to test_head's 1e-5."""
    sdt, store, load = storage(ops, fmt, device)
    g = U.gen(B, Rh, Rw, 60)
    z = U.normal_values((B, 16, Rh, Rw), g, fmt)
    w = torch.randn(4, 16, 1, 1, generator=g) * 0.3
    b = torch.randn(4, generator=g)
    zp = store(F.pad(E.nhwc(z), (0, 16)))
    logit = F.conv2d(z.double(), w.double(), b.double())
    A = F.conv2d(z.double().abs(), w.double().abs(), b.double().abs())
    ref = torch.sigmoid(F.pixel_shuffle(logit, 2))
    o = ops.head_fwd(zp, B, Rh, Rw, w.to(device), b.to(device))
    check(f"head_fwd_{fmt}", sid(B, Rh, Rw), o.cpu(), ref,
          0.25 * 18 * U.E32 * F.pixel_shuffle(A, 2) + 8 * U.E32)
    go = torch.randn(B, 1, 2 * Rh, 2 * Rw, generator=g)
    dw, db = torch.empty(4, 16, 1, 1, device=device), torch.empty(4, device=device)
    dz = ops.head_bwd(go.to(device), o, zp, B, Rh, Rw, w.to(device), dw, db)
    assert dz.dtype == sdt
    oc = o.cpu().double()
    d = F.pixel_unshuffle(go.double() * (1 - oc) * oc, 2)          # [B, 4, Rh, Rw]
    ref = torch.einsum("bjhw,jc->bchw", d, w.double().view(4, 16))
    A = torch.einsum("bjhw,jc->bchw", d.abs(), w.double().abs().view(4, 16))
    dzl = load(dz)
    check(f"head_bwd_{fmt}", sid(B, Rh, Rw), nchw(dzl[:, :16], B, Rh, Rw), ref,
          U.elem_bound(ref, A, "head_bwd", fmt))
    assert dzl[:, 16:].abs().max().item() == 0
    assert rel(dw.cpu().view(4, 16), torch.einsum("bjhw,bchw->jc", d, z.double())) <= 1e-5
    assert rel(db.cpu(), d.sum((0, 2, 3))) <= 1e-5


# ---- g. f16-only edges -------------------------------------------------------------------
def test_avgpool_ties_to_even(ops, device):
    """Windows {a, a, a, a + 2 ulp} for every positive and negative f16 a from
    the smallest subnormal up to 2^15 and beyond: the mean is exact in fp32 and
    lies halfway between two halves (three quarters across a binade edge), so
    the stored result is ref64.to(float16) bit for bit."""
    n = 0x7C00 - 8                               # bit patterns 0 .. n - 1; a + 2 ulp stays finite
    bits = torch.arange(n, dtype=torch.int16)
    a = bits.view(torch.float16)
    hi = (bits + 2).view(torch.float16)
    x = a.view(1, n, 1, 1).repeat(2, 1, 2, 2).clone()
    pos = torch.arange(n) % 4
    x[:, torch.arange(n), pos // 2, pos % 2] = hi
    x[1] = -x[1]
    ref = F.avg_pool2d(x.double(), 2)
    assert torch.equal(ref.float().double(), ref)
    want = ref.to(torch.float16)
    ties = (ref - want.double()).abs() == (hi.double() - a.double()).view(1, n, 1, 1) / 4
    assert ties.double().mean().item() >= 0.9
    xd = E.nhwc(x).to(device).view(torch.int16)
    got = ops.avgpool2(xd, 2, 2, 2).view(torch.float16).cpu()
    assert torch.equal(got.view(torch.int16), E.nhwc(want).view(torch.int16))
    margin("ties_to_even", "avgpool2", 0.0)


def test_conv_fwd_ties_to_even(ops, device):
    """A 32 -> 32 identity 1x1 with x over the whole f16 grid of [1, 2) and
    bias 2^-11: every acc + bias is a tie; bitwise ref64.to(float16)."""
    x = (torch.arange(1024, dtype=torch.int16) + 0x3C00).view(torch.float16).float().view(1, 4, 8, 32)
    x = x.permute(0, 3, 1, 2).contiguous()          # [1, 32, 4, 8]
    assert x.min().item() == 1.0 and x.max().item() < 2.0
    w = torch.eye(32).view(32, 32, 1, 1)
    b = torch.full((32,), 2.0 ** -11)
    ref = U.conv_ref(x, w, b)
    want = E.nhwc(ref.to(torch.float16))
    assert ((E.nhwc(ref) - want.double()).abs() == 2.0 ** -11).all()
    wp = ops.pack_conv_weight(w.to(device), 32, 32, ops.PACK_FWD, ops.F16S)
    y = ops.conv_fwd(E.nhwc(x).to(device).half().view(torch.int16), 1, 4, 8, wp, b.to(device), 32, 1)
    assert torch.equal(y.cpu(), want.view(torch.int16))
    margin("ties_to_even", "conv_fwd", 0.0)


@pytest.mark.parametrize("B,H,W,ci,co,k", [(2, 9, 11, 32, 64, 3), (3, 7, 5, 32, 128, 1),
                                           (1, 239, 257, 64, 256, 1)])
def test_tiny_out_conv_fwd_bn(ops, device, B, H, W, ci, co, k):
    """Gradual underflow of the store: outputs in f16's subnormal range, the
    bound's tiny term (2^-25) all the rounding allowed (a flush is off by up
    to 2^-14)."""
    case, ref, S = conv_case(B, H, W, ci, co, k, "f16", "tiny")
    y, part = run_conv_fwd_bn(ops, device, case, "f16")
    check("tiny_out_f16", sid(B, H, W, ci, co, k), y, ref, U.gemm_bound(ref, S, k * k * ci, "f16"))
    assert ((y != 0) & (y.abs() < U.F16_MIN_NORMAL)).double().mean().item() >= 0.25
    check_partials(part, y, co)


def test_tiny_out_bn_act(ops, device):
    B, C, H, W = 2, 64, 6, 5
    g = U.gen(B, C, H, W, 61)
    y = E.rounder("f16")(torch.randn(B, C, H, W, generator=g) * 2.0 ** -17)
    st, v = bn_vectors(C, g, device, ops)
    st.shift.zero_()
    v.shift = torch.zeros(C)
    z, _, bound = U.bn_act_ref(y, v.scale, v.shift, "f16")
    assert ((z != 0) & (z.abs() < U.F16_MIN_NORMAL)).double().mean().item() >= 0.25
    out = ops.bn_act(to_dev(ops, "f16", device, y), st, 0.2)
    check("tiny_out_f16", "bn_act", from_dev(ops, "f16", device, out, B, H, W), z, bound)


@pytest.mark.parametrize("B,H,W,ci,co,k", [(3, 7, 5, 32, 128, 1), (1, 351, 350, 64, 128, 1)])
def test_grad_operands_conv_fwd(ops, device, B, H, W, ci, co, k):
    """Subnormal f16 operands through the matrix core: whole pixels of x hold
    subnormal values only, so flushing them zeroes outputs the bound pins."""
    case, ref, S = conv_case(B, H, W, ci, co, k, "f16", "grad")
    assert U.subnormal_share(case.x) >= 0.25
    y, _ = run_conv_fwd_bn(ops, device, case, "f16", stats=False)
    check("grad_operands_f16", sid(B, H, W, ci, co, k), y, ref, U.gemm_bound(ref, S, k * k * ci, "f16"))


@pytest.mark.parametrize("B,H,W,ci,co,k", [(2, 9, 11, 32, 64, 3), (1, 351, 350, 64, 128, 1)])
def test_overflow_conv_fwd_bn(ops, device, B, H, W, ci, co, k):
    """Beyond 65504 the store gives +-Inf (no saturation), the other channels
    are untouched, and a partial row that holds a stored Inf has a non-finite
    sum: what lets GradScaler see the overflow."""
    case, ref, S = conv_case(B, H, W, ci, co, k, "f16", "overflow")
    K = k * k * ci
    inf, amb = U.overflow_classes(ref, S, K)
    y, part = run_conv_fwd_bn(ops, device, case, "f16")
    ok = ~amb
    assert not torch.isnan(y).any()
    assert torch.equal(torch.isinf(y)[ok], inf[ok])
    assert torch.equal(torch.sign(y)[ok & inf], torch.sign(ref)[ok & inf])
    check("overflow_f16", sid(B, H, W, ci, co, k), y, ref, U.gemm_bound(ref, S, K, "f16"), keep=ok & ~inf)
    cold = ~case.hot
    n, rpc, M = part.nchunk, part.rpc, B * H * W
    pb = part.buf.view(n, 2, co)
    check_partials(types.SimpleNamespace(buf=pb[:, :, cold.to(device)].contiguous(), nchunk=n, rpc=rpc),
                   y[:, cold], int(cold.sum()))
    has_inf = F.pad(torch.isinf(y), (0, 0, 0, n * rpc - M)).view(n, rpc, co).any(1)
    assert has_inf.any()
    assert not torch.isfinite(pb[:, 0].cpu())[has_inf].any()
