"""The fused BN-act 1x1 forward of the fp32 train step (csrc/nsm_conv_h2d.inc
gemm_h2a_kernel, behind nsm_bn_act_conv1x1_h2): one kernel applies BN1 +
LeakyReLU (+ Dropout2d mask) to its tile of Y1, writes the h2 operand A1 for
the weight gradient and feeds the same words to the 1x1 GEMM through LDS,
instead of nsm_bn_act_h2 writing A1 and nsm_conv1x1_h2 reading it back.

GPU: A1, Y2 and the BN2 partials are bitwise those of the two kernels and do
not depend on the grid; Y2 and the statistics meet the float64 bounds of
tests/test_gpu_h2d.py::test_conv1x1_h2_fwd_wgrad; a B=2 train step is bitwise
the same with the knob on and off. The shapes are the smallest at which a tile
walk, a mask row or a K-tile count can go wrong: ragged last tile, fewer tiles
than blocks, 1 / 2 / 3 / 4 / 16 K-tiles, every block tile, a Dropout2d mask row
that changes inside a tile (two and three images per tile), Y1 as a column
slice of a wider tensor.

CPU: the plan query (no data)."""
import functools

import pytest
import torch

gpu = pytest.mark.gpu

SLOPE = 0.2
BM = 128  # rows of the tile h2d_tile gives every SMALL shape (asserted in _case)
HW = 100
CH = [(32, 64), (64, 128), (128, 64), (64, 32), (512, 128), (96, 64)]
SMALL = [(M, ci, co) for ci, co in CH for M in (5 * BM + 37, BM - 5)]
# the 256-row tiles the B=8 step runs (256x128: >= 256 M blocks, 256x64: >= 512),
# ragged last tile; (.., 32, 64): the single-stage kernel of one K-tile
BIG = [(256 * 256 + 37, 64, 128, 256), (512 * 256 + 37, 128, 64, 256), (512 * 256 + 37, 32, 64, 256)]


@pytest.fixture(scope="module")
def ops(device):
    from nsm_amd import ops as O
    prev = O.set_f32_split(2)
    form = O.set_h2d_act_fuse()
    yield O
    O.set_h2d_act_fuse(*form)
    O.set_f32_split(prev)


def _spread(g, n, lo, hi):
    return torch.pow(2.0, torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo)


@functools.lru_cache(maxsize=None)
def _case(M, cin_p, cout_p, masked=True, wide=False, hw=HW, bm=BM):
    """Y1 with channel scales spread 2^U(-6, 0) and a few outlier rows, gamma
    spread, the BN state with the A1 bound, the h2 weight pack; once per shape."""
    from nsm_amd import ops
    device = torch.device("cuda:0")
    g = torch.Generator().manual_seed(M + 3 * cin_p + cout_p)
    B = -(-M // hw)
    Y1 = torch.randn(M, cin_p, generator=g, dtype=torch.float64) * _spread(g, cin_p, -6, 0)
    Y1[torch.randint(0, M, (3,), generator=g)] *= 40.0
    gamma = torch.randn(cin_p, generator=g, dtype=torch.float64) * _spread(g, cin_p, -4, 0)
    beta = torch.randn(cin_p, generator=g, dtype=torch.float64) * 0.1
    w = torch.randn(cout_p, cin_p, generator=g, dtype=torch.float64) / cin_p ** 0.5
    b = torch.randn(cout_p, generator=g, dtype=torch.float64) * 0.1
    mask = ((torch.rand(B, cin_p, generator=g) > 0.2).float() / 0.8).to(device) if masked else None
    Y1s = Y1.float().to(device).contiguous()
    bn = torch.nn.BatchNorm2d(cin_p).to(device)
    with torch.no_grad():
        bn.weight.copy_(gamma.float())
        bn.bias.copy_(beta.float())
    am = ops.amax_slots(2, device)
    bound, aw = ops.amax_slot(am, 0), ops.amax_slot(am, 1)
    st = ops.bn_train(Y1s, bn, cin_p, 0.1, 1e-5, bound=(bound, 1.0 / 0.8 if masked else 1.0))
    ws = w.float().to(device).contiguous()
    ops.absmax(ws, aw)
    wh = ops.to_h2(ws, aw)
    if wide:  # ldy > C
        buf = torch.zeros(M, cin_p + 32, device=device)
        buf[:, :cin_p] = Y1s
        Y1v = buf[:, :cin_p]
    else:
        Y1v = Y1s
    rows = ops.bn_act_conv1x1_h2_plan(M, cin_p, cout_p)[3]
    assert rows == bm, (rows, bm)
    torch.cuda.synchronize()
    return dict(M=M, cin_p=cin_p, cout_p=cout_p, Y1=Y1v, Y1c=Y1s, st=st, mask=mask, wh=wh, ws=ws,
                w64=w.to(device), bs=b.float().to(device), b64=b.to(device), bound=bound, aw=aw,
                hw=hw, am=am, bn=bn)


def _run(ops, c, form, grid=0):
    prev = ops.set_h2d_act_fuse(form, grid)
    try:
        plan = ops.bn_act_conv1x1_h2_plan(c["M"], c["cin_p"], c["cout_p"])
        a1, y, part = ops.bn_act_conv1x1_h2(c["Y1"], c["st"], c["wh"], c["bs"], c["cout_p"], SLOPE,
                                            mask=c["mask"], HW=c["hw"], bound=c["bound"],
                                            amax_w=c["aw"])
        torch.cuda.synchronize()
    finally:
        ops.set_h2d_act_fuse(*prev)
    return dict(a1=a1, y=y, part=part, plan=plan)


def _same(a, b):
    assert torch.equal(a["a1"].view(torch.int16), b["a1"].view(torch.int16)), "A1"
    assert torch.equal(a["y"].view(torch.int32), b["y"].view(torch.int32)), "Y2"
    assert a["part"].nchunk == b["part"].nchunk and a["part"].rpc == b["part"].rpc
    assert torch.equal(a["part"].buf.view(torch.int32), b["part"].buf.view(torch.int32)), "partials"


def _check_bitwise(ops, c):
    two = _run(ops, c, "two kernels")
    assert two["plan"][1:3] == ("two kernels", 0)
    tiles = -(-c["M"] // two["plan"][3])
    for grid in (0, 1, 3):
        f = _run(ops, c, "fused", grid)
        assert f["plan"][1] == "fused" and f["plan"][2] == (min(grid, tiles) if grid else tiles)
        assert f["plan"][0] == two["plan"][0] and f["plan"][3] == two["plan"][3]
        _same(f, two)


@gpu
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("M,cin_p,cout_p", SMALL)
def test_bitwise_and_grid_independent(ops, device, M, cin_p, cout_p, masked):
    """Fused == two kernels on the raw words of A1, Y2 and the partials, for
    forced grids of 1 and 3 blocks and the default; HW = 100: a 128-row tile
    holds two or three images."""
    _check_bitwise(ops, _case(M, cin_p, cout_p, masked))


@gpu
def test_bitwise_wide_y1_and_two_image_tiles(ops, device):
    """Y1 as a column slice of a wider tensor (ldy > C); HW = 200: tiles inside
    one image beside tiles spanning two, HW = 100000: one image for all."""
    _check_bitwise(ops, _case(5 * BM + 37, 128, 64, True, True))
    _check_bitwise(ops, _case(5 * BM + 37, 64, 128, True, False, 200))
    _check_bitwise(ops, _case(5 * BM + 37, 64, 32, True, True, 100000))


@gpu
@pytest.mark.parametrize("M,cin_p,cout_p,bm", BIG)
def test_bitwise_256_row_tiles(ops, device, M, cin_p, cout_p, bm):
    c = _case(M, cin_p, cout_p, True, False, 4096, bm)
    two = _run(ops, c, "two kernels")
    for grid in (0, 3):
        _same(_run(ops, c, "fused", grid), two)


def _errs(a, ref):
    d = (a.double() - ref).abs()
    return d.max().item(), d.pow(2).mean().sqrt().item()


@gpu
@pytest.mark.parametrize("M,cin_p,cout_p", [(5 * BM + 37, ci, co) for ci, co in CH] + [(BM - 5, 512, 128)])
def test_fp64_parity(ops, device, M, cin_p, cout_p):
    """The bounds of test_conv1x1_h2_fwd_wgrad: against float64 on the same
    operands (the fp32 A1 of nsm_bn_act) Y2's error stays within 1.5x (rms) /
    2x (max) of the exact fp32-MFMA path's, and the BN statistics from the
    partials meet its assert_close limits."""
    c = _case(M, cin_p, cout_p, True)
    f = _run(ops, c, "fused")
    a32 = ops.bn_act(c["Y1c"], c["st"], SLOPE, mask=c["mask"], HW=c["hw"])
    ref = a32.double() @ c["w64"].T + c["b64"]
    prev = ops.set_f32_split(0)
    try:
        wpk = ops.pack_conv_weight(c["ws"].view(cout_p, cin_p, 1, 1), cout_p, cin_p, ops.PACK_FWD)
        y0, _ = ops.conv_fwd_bn(a32, 1, 1, M, wpk, c["bs"], cout_p, 1, stats=True)
    finally:
        ops.set_f32_split(prev)
    torch.cuda.synchronize()
    (mx, rms), (mx0, rms0) = _errs(f["y"], ref), _errs(y0, ref)
    print(f"Y2: max {mx:.3e} rms {rms:.3e}; fp32 path max {mx0:.3e} rms {rms0:.3e}")
    assert rms <= 1.5 * rms0 + 1e-12 and mx <= 2.0 * mx0 + 1e-12, (mx, rms, mx0, rms0)
    # the same bound against a reference that shares no kernel with the code
    # under test: lrelu(BN(Y1)) * mask restated in float64 from the fp32 Y1 (the
    # fp32 path's error then holds the fp32 BN arithmetic too, as the fused one's)
    Y1d = c["Y1c"].double()
    inv = (Y1d.var(0, unbiased=False) + 1e-5).rsqrt()
    z = (Y1d - Y1d.mean(0)) * inv * c["bn"].weight.double() + c["bn"].bias.double()
    a64 = torch.where(z > 0, z, SLOPE * z) * c["mask"].double().repeat_interleave(c["hw"], 0)[:M]
    ref2 = a64 @ c["w64"].T + c["b64"]
    (mx, rms), (mx0, rms0) = _errs(f["y"], ref2), _errs(y0, ref2)
    print(f"Y2 vs float64 BN: max {mx:.3e} rms {rms:.3e}; fp32 path max {mx0:.3e} rms {rms0:.3e}")
    assert rms <= 1.5 * rms0 + 1e-12 and mx <= 2.0 * mx0 + 1e-12, (mx, rms, mx0, rms0)
    bn2 = torch.nn.BatchNorm2d(cout_p).to(device)
    st = ops.bn_train(f["y"], bn2, cout_p, 0.1, 1e-5, part=f["part"])
    torch.testing.assert_close(st.mean.double(), ref.mean(0), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(st.invstd.double(), (ref.var(0, unbiased=False) + 1e-5).rsqrt(),
                               rtol=1e-4, atol=0)


def test_plan():
    """No GPU, no data: the policy fuses the 1x1 forwards of the B=8 512x512
    step whose N is one block tile (conv2, conv3, conv7, conv8, conv9) and
    leaves conv4 / conv5 / conv6 (several N tiles) on the two kernels; the
    knob forces either form where the fused kernel covers the shape."""
    from nsm_amd import ops
    from nsm_amd._lib import lib
    prev = ops.set_h2d_act_fuse("policy", 0)
    try:
        for (M, ci, co), tile in (((524288, 32, 64), 4), ((131072, 64, 128), 2), ((131072, 512, 128), 2),
                                  ((524288, 128, 64), 4), ((524288, 64, 32), 6)):
            t, form, grid, rows = ops.bn_act_conv1x1_h2_plan(M, ci, co)
            assert (t, form) == (tile, "fused")
            assert rows == lib.nsm_conv1x1_h2_rows(M, co, 2 * ci, 0) == (128 if tile == 6 else 256)
            assert grid == -(-M // rows)
        # conv4 = DoubleConv(128, 512), conv5 = (512, 1024), conv6 = (1024, 512) at B=8
        for M, ci, co in ((32768, 128, 512), (8192, 512, 1024), (32768, 1024, 512)):
            t, form, grid, rows = ops.bn_act_conv1x1_h2_plan(M, ci, co)
            assert (form, grid) == ("two kernels", 0)
            assert rows == lib.nsm_conv1x1_h2_rows(M, co, 2 * ci, 0)
        ops.set_h2d_act_fuse("two kernels", 0)
        assert ops.bn_act_conv1x1_h2_plan(524288, 128, 64)[1:3] == ("two kernels", 0)
        ops.set_h2d_act_fuse("fused", 7)
        assert ops.bn_act_conv1x1_h2_plan(524288, 128, 64)[1:3] == ("fused", 7)
        assert ops.bn_act_conv1x1_h2_plan(123, 128, 64)[1:3] == ("fused", 1)
        assert ops.bn_act_conv1x1_h2_plan(8192, 512, 1024)[1:3] == ("two kernels", 0)   # not covered
        assert ops.set_h2d_act_fuse() == (2, 7)
    finally:
        ops.set_h2d_act_fuse(*prev)


@gpu
def test_train_step_bitwise(ops, device):
    """B=2, 7x64x64 train step (forward, CustomLoss, backward) with the fused
    form on and off: output, loss, every parameter gradient and x.grad bitwise
    equal (same seed: same initial weights and Dropout2d masks)."""
    import nsm_amd
    gx = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, 7, 64, 64, generator=gx).to(device)
    y = (torch.randint(0, 256, (2, 1, 64, 64), generator=gx).float() / 255.0).to(device)

    def step(form):
        prev = ops.set_h2d_act_fuse(form, 0)
        try:
            torch.manual_seed(5)
            m = nsm_amd.Unet(in_ch=7, dropout_rate=0.2).to(device).train()
            x = x0.clone().requires_grad_(True)
            out = m(x)
            blocks = out.grad_fn.saved_blocks
            assert all(s.A1 is not None and s.A1.dtype == ops.H2 for s in blocks.values())
            # what each DoubleConv's 1x1 forward of THIS step ran (the form is still in force)
            forms[form] = {k: ops.bn_act_conv1x1_h2_plan(s.B * s.H * s.W, s.cip, s.cop)[1]
                           for k, s in blocks.items()}
            narrow[form] = {k for k, s in blocks.items() if s.cop <= 128}
            loss = nsm_amd.CustomLoss(device, 0.9, vgg_weights=False)(out, y, x)
            loss.backward()
            torch.cuda.synchronize()
            return out.detach(), loss.detach(), x.grad, {k: p.grad for k, p in m.named_parameters()}
        finally:
            ops.set_h2d_act_fuse(*prev)

    forms, narrow = {}, {}
    on, off = step("fused"), step("two kernels")
    # the layers of this step whose N is one block tile took the fused kernel
    # (conv2, conv3, conv7, conv8, conv9), the others and the off arm did not
    assert len(narrow["fused"]) == 5 and len(forms["fused"]) > 5
    assert {k for k, f in forms["fused"].items() if f == "fused"} == narrow["fused"]
    assert set(forms["two kernels"].values()) == {"two kernels"}
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]) and torch.equal(on[2], off[2])
    assert on[3].keys() == off[3].keys()
    for k in on[3]:
        assert torch.equal(on[3][k], off[3][k]), k


@gpu
def test_bn_bwd_apply_h2_partial_wave(ops, device):
    """nsm_bn_bwd_apply_h2 at C = 96 (blocks of 252 threads before the whole-wave
    launch: the h2 scale's wave reduction ran short in the last wave): the bound
    dominates max|dY|, and every row of the h2 tensor decodes to the fp32
    nsm_bn_bwd_apply values within the f16x2 bound at the ONE scale of the
    slot (tests/test_gpu_h2d.py::test_bn_bwd_h2_bound's check)."""
    import math

    import numpy as np
    g = torch.Generator().manual_seed(96)
    B, H, W, C = 4, 32, 32, 96
    M = B * H * W
    sp = lambda: _spread(g, C, -12, 0).float()  # noqa: E731
    yd = (torch.randn(M, C, generator=g) * sp() + torch.randn(C, generator=g)).to(device)
    gg = (torch.randn(M, C, generator=g) * sp()).to(device)
    bn = torch.nn.BatchNorm2d(C).to(device)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g) * sp())
        bn.bias.copy_(torch.randn(C, generator=g) * 0.1)
    st = ops.bn_train(yd, bn, C, 0.1, 1e-5)
    d32 = ops.bn_bwd(gg, yd, st, H * W, None, C, *[torch.zeros(C, device=device) for _ in range(3)])
    slots = ops.amax_slots(2, device)
    k1dz, bnd = ops.amax_slot(slots, 0), ops.amax_slot(slots, 1)
    dh = ops.bn_bwd(gg, yd, st, H * W, None, C, *[torch.zeros(C, device=device) for _ in range(3)],
                    h2=(k1dz, bnd))
    torch.cuda.synchronize()
    v = bnd.view(torch.int32).cpu().numpy().astype(np.uint32).max()
    bound = float(np.array(v, dtype=np.uint32).view(np.float32))
    d32 = d32.double()
    assert bound >= d32.abs().max().item()
    e = max(-126, min(126, 15 - math.ceil(math.log2(bound))))
    h = dh.view(M, C // 8, 2, 8).double()
    dec = (h[:, :, 0, :] + h[:, :, 1, :]).reshape(M, C) * 2.0 ** (-e)
    err = (dec - d32).abs()
    assert (err <= d32.abs() * 2.0 ** -21 + 2.0 ** (-25 - e)).all()
