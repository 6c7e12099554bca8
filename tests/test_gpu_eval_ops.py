"""GPU: the eval-mode fused epilogues op by op (nsm_bn_finalize_eval,
nsm_conv_fwd_act in fp32 / bf16 / f16 storage on every tile of its dispatch,
nsm_wino_output_act, nsm_wino_output_bf16m_act, the lazy resamplers in f16
storage) against the float64 restatement of eval_util.py on calibrated-looking
running statistics (mixed-sign gamma, variances 2^U(-4,4), means of order 1).

Bounds (none measured on the kernels):
  fp32   |got - z| <= 2e-5 max(1, max|c|) max(1, max|scale|) + 2^-22 max|z|
         (test_conv_fwd's bound on the convolution c, through the affine map)
  16-bit y = r(lrelu(r(acc + bias) scale + shift) (+ res)), u = 2^-8 / 2^-11:
         |got - z| <= 1.1 u (|scale_c| |c| + |z|) + |scale_c| 1e-5 max|c|
         (intermediate rounding through a 1-Lipschitz LeakyReLU, final
         rounding, fp32 accumulation), per element
  Winograd fp32: WINO_TOL[tile]["fwd"] max(1, max|c|) max(1, max|scale|)."""
import pytest
import torch
import torch.nn.functional as F

import eval_util as E
from test_gpu_ops import WINO_TOL, rel
from util import record_margin

pytestmark = pytest.mark.gpu
torch.set_num_threads(16)
BF = torch.bfloat16


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
        record_margin("eval_ops." + family, worst_err_over_bound=float(ratio), case=case_id)


_REF = {}


def cached(key, make):
    """The float64 reference of one case, computed once and shared by the
    tests that run consecutively on it (one entry: the large ones are big)."""
    if key not in _REF:
        _REF.clear()
        _REF[key] = make()
    return _REF[key]


def conv_ref(B, H, W, ci, co, k, fmt):
    """(case, c [M, co], z [M, co]) float64, no skip."""
    def make():
        case = E.make_case(B, H, W, ci, co, k, fmt=fmt)
        c, z = E.reference(case)
        return case, E.nhwc(c), E.nhwc(z)
    return cached(("conv", B, H, W, ci, co, k, fmt), make)


def bn_module(case, device):
    bn = torch.nn.BatchNorm2d(case.co, eps=case.eps)
    with torch.no_grad():
        bn.weight.copy_(case.gamma)
        bn.bias.copy_(case.beta)
        bn.running_mean.copy_(case.rmean)
        bn.running_var.copy_(case.rvar)
    return bn.to(device).eval()


def bn_state(ops, case, device, C=None):
    """The eval BNState through nsm_bn_finalize_eval, as the model builds it."""
    return ops.bn_eval(bn_module(case, device), C or case.co, case.co, case.eps, device)


def storage(ops, fmt, device):
    """(storage dtype, host fp32 -> device storage, device storage -> host fp64)."""
    if fmt == "f16":
        return (ops.F16S, lambda t: t.to(device).half().view(torch.int16),
                lambda t: t.view(torch.float16).cpu().double())
    if fmt == "bf16":
        return BF, lambda t: t.to(device, BF), lambda t: t.cpu().double()
    return torch.float32, lambda t: t.to(device), lambda t: t.cpu().double()


def skip_arg(case, variant, store, sentinel=1e3):
    """The skip operand of a variant: None, a dense [M, co] tensor, or a
    column slice of a wider buffer (row stride co + pad; the columns outside
    the slice hold a sentinel that a wrong stride would read)."""
    if variant == "plain":
        return None
    r = E.nhwc(case.res)
    if variant == "res":
        return store(r)
    pad = int(variant.rsplit("ld", 1)[1])
    wide = store(torch.cat([torch.full((r.shape[0], pad), sentinel), r], 1))
    view = wide[:, pad:]
    assert view.stride(0) == case.co + pad and view.shape == r.shape
    return view


def check_partials(part, yr, co):
    """BN partials [nchunk][2][co] == float64 per-chunk sums and centred squares
    of the stored rows (the last chunk ragged), as test_conv_fwd_bf16 checks them."""
    M = yr.shape[0]
    rpc, n = part.rpc, part.nchunk
    assert n == -(-M // rpc)
    pb = part.buf.view(n, 2, co).cpu().double()
    yd = F.pad(yr, (0, 0, 0, n * rpc - M)).view(n, rpc, co)
    cnt = torch.clamp(M - torch.arange(n) * rpc, max=rpc).double()[:, None]
    s1 = yd.sum(1)
    mu = s1 / cnt
    valid = (torch.arange(rpc)[None, :] < cnt)[:, :, None]
    m2 = (((yd - mu[:, None, :]) ** 2) * valid).sum(1)
    torch.testing.assert_close(pb[:, 0], s1, rtol=1e-4, atol=1e-2)
    torch.testing.assert_close(pb[:, 1], m2, rtol=1e-3, atol=1e-2)


def ulp32(t):
    """Spacing of float32 at |t| (t float64)."""
    a = t.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


# ---- nsm_bn_finalize_eval ------------------------------------------------------
def test_bn_eval_vectors(ops, device):
    """scale / shift / mean / invstd of bn_eval against the float64 formulas to
    4 fp32 ulps (shift: of |beta| + |mean * scale|, the terms it cancels), with
    variance 0 and 1e4 and negative gamma; the 24 pad channels follow the
    kernel's rule (mean 0, variance 1); bn_eval_into recomputes in place."""
    C, cr, eps = 64, 40, 1e-5
    g = torch.Generator().manual_seed(40)
    bn = torch.nn.BatchNorm2d(cr, eps=eps)
    with torch.no_grad():
        bn.weight.copy_((torch.rand(cr, generator=g) + 0.5)
                        * torch.where(torch.rand(cr, generator=g) < 0.25, -1.0, 1.0))
        bn.weight[3] = -1.25
        bn.bias.copy_(torch.randn(cr, generator=g))
        bn.running_mean.copy_(torch.randn(cr, generator=g) * 2)
        bn.running_var.copy_(torch.pow(2.0, torch.rand(cr, generator=g) * 8 - 4))
        bn.running_var[0], bn.running_var[3], bn.running_var[7] = 0.0, 1e4, 0.0
    bn = bn.to(device).eval()
    # pad entries that are not zero, so the pad channels' rule shows
    gam = torch.cat([bn.weight.detach().cpu(), torch.rand(C - cr, generator=g) + 0.5]).to(device)
    bet = torch.cat([bn.bias.detach().cpu(), torch.randn(C - cr, generator=g)]).to(device)

    def check(st, tag):
        pad = torch.zeros(C - cr, dtype=torch.float64)
        rm = torch.cat([bn.running_mean.cpu().double(), pad])
        rv = torch.cat([bn.running_var.cpu().double(), pad + 1])
        scale, shift, mean, inv = E.bn_vectors(gam.cpu(), bet.cpu(), rm, rv, eps)
        got = {k: getattr(st, k).cpu().double() for k in ("scale", "shift", "mean", "invstd")}
        assert torch.equal(got["mean"], mean)
        worst = 0.0
        for k, ref, tol in (("invstd", inv, 4 * ulp32(inv)), ("scale", scale, 4 * ulp32(scale)),
                            ("shift", shift, 4 * ulp32(bet.cpu().double().abs() + (mean * scale).abs()))):
            r = ((got[k] - ref).abs() / tol).max().item()
            print(f"bn_eval {tag} {k}: {r * 4:.2f} ulps")
            worst = max(worst, r)
            assert r <= 1.0, (k, r)
        margin("bn_eval", tag, worst)

    st = ops.bn_eval(bn, C, cr, eps, device, gamma=gam, beta=bet)
    check(st, "first")
    ptrs = [getattr(st, k).data_ptr() for k in ("scale", "shift", "mean", "invstd")]
    with torch.no_grad():
        bn.running_mean.mul_(-0.5).add_(0.25)
        bn.running_var.add_(0.75)
    ops.bn_eval_into(st, bn, C, cr, eps)
    assert ptrs == [getattr(st, k).data_ptr() for k in ("scale", "shift", "mean", "invstd")]
    check(st, "recomputed")
    # the padding the model uses (pad_vec: zeros) gives inert pad channels
    st0 = ops.bn_eval(bn, C, cr, eps, device)
    assert st0.scale[cr:].abs().max().item() == 0 and st0.shift[cr:].abs().max().item() == 0


# ---- nsm_conv_fwd_act, fp32 ------------------------------------------------------
# the small shapes run the 64-row tiles; eval_util.F32_LARGE names the tile of each large one
F32_SHAPES = [s + (64,) for s in E.SMALL] + E.F32_LARGE


def f32_bound(c, z, scale):
    return (2e-5 * max(1.0, c.abs().max().item()) * max(1.0, scale.abs().max().item())
            + 2.0 ** -22 * z.abs().max().item())


# res_ld4: a 16-byte aligned slice, row stride cout_p + 4 (the vector path);
# res_ld1: row stride cout_p + 1 (EpiStore's scalar fallback)
@pytest.mark.parametrize("variant", ["plain", "res", "res_ld4", "res_ld1"])
@pytest.mark.parametrize("B,H,W,ci,co,k,rows", F32_SHAPES)
def test_conv_fwd_act_f32(ops, device, B, H, W, ci, co, k, rows, variant):
    from nsm_amd._lib import lib
    assert lib.nsm_conv_stat_rows(B, H, W, co) == rows
    case, c, z = conv_ref(B, H, W, ci, co, k, "f32")
    st = bn_state(ops, case, device)
    wp = ops.pack_conv_weight(case.w.to(device), co, ci, ops.PACK_FWD)
    res = skip_arg(case, variant, lambda t: t.to(device))
    got = ops.conv_fwd_act(E.nhwc(case.x).to(device), B, H, W, wp, case.b.to(device), co, k, st,
                           res=res, slope=case.slope)
    want = z if res is None else z + E.nhwc(case.res).double()
    scale = E.bn_vectors(case.gamma, case.beta, case.rmean, case.rvar, case.eps)[0]
    err = (got.cpu().double() - want).abs().max().item()
    bound = f32_bound(c, want, scale)
    print(f"conv_fwd_act f32 {variant}: err {err:.3e} bound {bound:.3e}")
    margin("conv_fwd_act_f32", f"{B}x{H}x{W}x{ci}x{co}k{k}-{variant}", err / bound)
    assert err <= bound


@pytest.mark.parametrize("B,H,W,ci,co,k,rows", F32_SHAPES)
def test_conv_fwd_bn_f32_tiles(ops, device, B, H, W, ci, co, k, rows):
    """conv_fwd_bn at the same shapes: y under test_conv_fwd's bound and the BN
    partials of every fp32 tile (128 and 256 rows included) against float64."""
    case, c, _ = conv_ref(B, H, W, ci, co, k, "f32")
    wp = ops.pack_conv_weight(case.w.to(device), co, ci, ops.PACK_FWD)
    y, part = ops.conv_fwd_bn(E.nhwc(case.x).to(device), B, H, W, wp, case.b.to(device), co, k)
    assert part.rpc == rows
    yr = y.cpu().double()
    err, bound = (yr - c).abs().max().item(), 2e-5 * max(1.0, c.abs().max().item())
    margin("conv_fwd_bn_f32", f"{B}x{H}x{W}x{ci}x{co}k{k}", err / bound)
    assert err <= bound
    check_partials(part, yr, co)


@pytest.mark.parametrize("k", [3, 1])
def test_conv_fwd_act_padded_channels(ops, device, k):
    """40 real output channels packed to 64 (gamma, beta, bias, skip pads zero):
    the real columns within the fp32 bound, the pad columns exactly 0."""
    B, H, W, ci, co, cop = 2, 9, 11, 32, 40, 64
    case = E.make_case(B, H, W, ci, co, k, seed=1)
    c, z = (E.nhwc(t) for t in E.reference(case, res=True))
    st = bn_state(ops, case, device, C=cop)
    wp = ops.pack_conv_weight(case.w.to(device), cop, ci, ops.PACK_FWD)
    res = F.pad(E.nhwc(case.res), (0, cop - co)).to(device)
    got = ops.conv_fwd_act(E.nhwc(case.x).to(device), B, H, W, wp,
                           ops.pad_vec(case.b.to(device), cop), cop, k, st, res=res).cpu().double()
    scale = E.bn_vectors(case.gamma, case.beta, case.rmean, case.rvar, case.eps)[0]
    err, bound = (got[:, :co] - z).abs().max().item(), f32_bound(c, z, scale)
    margin("conv_fwd_act_f32", f"padded40k{k}", err / bound)
    assert err <= bound
    assert got[:, co:].abs().max().item() == 0


# ---- nsm_wino_output_act (fp32, tiles 2 / 4 / 6) ---------------------------------
WINO_ALL = [(B, None, None, H, W, ci, co) for B, H, W, ci, co in E.WINO] + E.WINO_SRC


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("tile", [2, 4, 6])
@pytest.mark.parametrize("B,hi,wi,H,W,ci,co", WINO_ALL)
def test_conv3x3_wino_act(ops, device, B, hi, wi, H, W, ci, co, tile, with_res):
    """The output transform's BN + LeakyReLU (+ skip) form (with act, F(6x6)
    runs the generic kernel, not the buffered one of the training step) against
    float64, ragged tile edges and the fused upsample included, and against the
    unfused device chain conv3x3_wino -> bn_act."""
    src_hw = None if hi is None else (hi, wi)

    def make():
        case = E.make_case(B, H, W, ci, co, 3, src_hw=src_hw)
        c, z = E.reference(case)
        return case, E.nhwc(c), E.nhwc(z)
    case, c, z = cached(("wino", B, hi, wi, H, W, ci, co), make)
    st = bn_state(ops, case, device)
    U = ops.wino_weight(case.w.to(device), co, ci, flip=False, tile=tile)
    xd, bd = E.nhwc(case.x).to(device), case.b.to(device)
    res = E.nhwc(case.res).to(device) if with_res else None
    got = ops.conv3x3_wino(xd, B, H, W, U, bd, co, tile=tile, src_hw=src_hw, act=(st, res))
    y = ops.conv3x3_wino(xd, B, H, W, U, bd, co, tile=tile, src_hw=src_hw)
    chain = ops.bn_act(y, st, case.slope, res=res)
    want = z + E.nhwc(case.res).double() if with_res else z
    scale = E.bn_vectors(case.gamma, case.beta, case.rmean, case.rvar, case.eps)[0]
    bound = WINO_TOL[tile]["fwd"] * max(1.0, c.abs().max().item()) * max(1.0, scale.abs().max().item())
    err = (got.cpu().double() - want).abs().max().item()
    d = rel(got.cpu(), chain.cpu())
    print(f"wino F({tile}) act: err {err:.3e} bound {bound:.3e}; vs unfused chain rel-l2 {d:.2e}")
    margin(f"wino_output_act_f{tile}", f"{B}x{hi}x{wi}->{H}x{W}x{ci}x{co}-res{int(with_res)}",
           max(err / bound, d / 1e-5))
    assert err <= bound
    assert d <= 1e-5   # FMA-contraction differences only (test_wino_input_fused_resize)


# ---- nsm_conv_fwd_act, bf16 and f16 storage --------------------------------------
S16_SHAPES = [s + (64,) for s in E.SMALL] + E.S16_LARGE
UNIT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}


# res_ld8: a 16-byte aligned slice of a wider buffer, row stride cout_p + 8
@pytest.mark.parametrize("variant", ["plain", "res", "res_ld8"])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("B,H,W,ci,co,k,rows", S16_SHAPES)
def test_conv_fwd_act_s16(ops, device, B, H, W, ci, co, k, rows, fmt, variant):
    from nsm_amd._lib import lib
    assert lib.nsm_conv_stat_rows_bf16(B, H, W, co) == rows
    sdt, store, load = storage(ops, fmt, device)
    case, c, z = conv_ref(B, H, W, ci, co, k, fmt)
    st = bn_state(ops, case, device)
    wp = ops.pack_conv_weight(case.w.to(device), co, ci, ops.PACK_FWD, sdt)
    res = skip_arg(case, variant, store)
    got = ops.conv_fwd_act(store(E.nhwc(case.x)), B, H, W, wp, case.b.to(device), co, k, st,
                           res=res, slope=case.slope)
    assert got.dtype == sdt
    want = z if res is None else z + E.nhwc(case.res).double()
    sc = E.bn_vectors(case.gamma, case.beta, case.rmean, case.rvar, case.eps)[0].abs()[None, :]
    bound = 1.1 * UNIT[fmt] * (sc * c.abs() + want.abs()) + sc * (1e-5 * c.abs().max().item())
    ratio = ((load(got) - want).abs() / bound).max().item()
    print(f"conv_fwd_act {fmt} {variant}: worst err / bound {ratio:.3f}")
    margin(f"conv_fwd_act_{fmt}", f"{B}x{H}x{W}x{ci}x{co}k{k}-{variant}", ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_conv_fwd_act_s16_rejects_unaligned_skip_stride(ops, device, fmt):
    """A skip row stride of cout_p + 4 elements (8 bytes off the 16-byte
    chunks) is refused by the host check before any launch."""
    from nsm_amd._lib import NsmError
    B, H, W, ci, co = 1, 4, 4, 32, 32
    sdt, store, _ = storage(ops, fmt, device)
    case = E.make_case(B, H, W, ci, co, 1, fmt=fmt)
    st = bn_state(ops, case, device)
    wp = ops.pack_conv_weight(case.w.to(device), co, ci, ops.PACK_FWD, sdt)
    wide = store(torch.zeros(B * H * W, co + 4))
    with pytest.raises(NsmError, match="leading dims"):
        ops.conv_fwd_act(store(E.nhwc(case.x)), B, H, W, wp, case.b.to(device), co, 1, st,
                         res=wide[:, :co])


# ---- nsm_wino_output_bf16m_act ---------------------------------------------------
WINO_F16_ALL = [(B, None, None, H, W, ci, co) for B, H, W, ci, co in E.WINO_F16] + E.WINO_F16_SRC


@pytest.mark.parametrize("B,hi,wi,H,W,ci,co", WINO_F16_ALL)
def test_conv3x3_wino_f16_act(ops, device, B, hi, wi, H, W, ci, co):
    """conv3x3_wino_f16(act=bn) against float64 of the bf16 input, relative to
    the unfused chain of the same run (f16-M conv stored as bf16, then bn_act):
    the fused form skips one bf16 rounding and must not be worse (the margins
    test_conv3x3_wino_f16_vs_direct_bf16 grants the same kernels)."""
    from test_gpu_wino_f16 import _prep_u
    src_hw = None if hi is None else (hi, wi)
    case = E.make_case(B, H, W, ci, co, 3, fmt="bf16", src_hw=src_hw, round_w=False)
    z = E.nhwc(E.reference(case)[1])
    st = bn_state(ops, case, device)
    xd, bd = E.nhwc(case.x).to(device, BF), case.b.to(device)
    ax = ops.amax_slots(1, device)
    ops.absmax(xd, ax)
    U, au = _prep_u(ops, case.w.to(device).contiguous(), ci, co, device)
    fused = ops.conv3x3_wino_f16(xd, B, H, W, U, bd, co, amax=(ax, au), stats=False, act=st,
                                 src_hw=src_hw)[0]
    y0 = ops.conv3x3_wino_f16(xd, B, H, W, U, bd, co, amax=(ax, au), stats=False, m16=True,
                              src_hw=src_hw)[0]
    chain = ops.bn_act(y0, st, case.slope)
    assert fused.dtype == BF
    e1, e0 = fused.cpu().double() - z, chain.cpu().double() - z
    rms1, rms0 = e1.pow(2).mean().sqrt().item(), e0.pow(2).mean().sqrt().item()
    mx1, mx0 = e1.abs().max().item(), e0.abs().max().item()
    print(f"wino f16 act rms {rms1:.3e} max {mx1:.3e} | unfused rms {rms0:.3e} max {mx0:.3e} | "
          f"of z rms {z.pow(2).mean().sqrt().item():.3e}")
    margin("wino_output_bf16m_act", f"{B}x{hi}x{wi}->{H}x{W}x{ci}x{co}",
           max(rms1 / (1.5 * rms0), mx1 / (2.0 * mx0)))
    assert rms1 <= 1.5 * rms0 and mx1 <= 2.0 * mx0, (rms1, rms0, mx1, mx0)


# ---- the lazy resamplers in f16 storage ------------------------------------------
@pytest.mark.parametrize("B,H,W,C", [(2, 16, 18, 64), (1, 9, 7, 128)])
def test_lazy_resize_f16_storage(ops, device, B, H, W, C):
    """resize / up2_resize of a Lazy block output in f16 storage == bn_act(+res)
    then the resize, bitwise (test_bn_act_pool_and_lazy_resize covers f32 and
    bf16); a geometry the row-blocked kernel does not take returns None."""
    _, store, load = storage(ops, "f16", device)
    g = torch.Generator().manual_seed(H * W + C)
    y = store(torch.randn(B * H * W, C, generator=g) * 2)
    res = store(torch.randn(B * H * W, C, generator=g))
    st = ops.BNState(C, device)
    st.scale.copy_((torch.rand(C, generator=g) + 0.5)
                   * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0))
    st.shift.copy_(torch.randn(C, generator=g))
    zr = ops.bn_act(y, st, 0.2, res=res)
    assert zr.dtype == ops.F16S
    lazy = ops.Lazy(y, st, res)
    up = ops.resize(zr, B, H, W, 2 * H, 2 * W)
    assert torch.equal(up, ops.resize_act(lazy, B, H, W, 2 * H, 2 * W, 0.2))
    th, tw = 2 * H - 1, 2 * W - 1
    a = ops.up2_resize_act(lazy, B, H, W, th, tw, 0.2)
    assert a is not None and torch.equal(ops.up2_resize(zr, B, H, W, th, tw), a)
    assert load(up).abs().max().item() > 0 and load(a).abs().max().item() > 0
    assert th * 2 >= 2 * H - 1 and (H - 1) * 2 < 2 * H - 1
    assert ops.up2_resize_act(lazy, B, H, W, H - 1, 2 * W, 0.2) is None
