"""GPU: the learned feature extraction (nsm_amd/extract.py, csrc/nsm_extract.hip)
against extract_util.reference (float64): bit for bit on the integer case, whose
every fp32 evaluation order is exact, and within the derived worst-case bounds
on the real-valued one; views, dx off, determinism, the module, and the cascade
ExtractedUnet through autograd, GraphedTrainStep, GraphedUnet, FramePipeline and
feature_sensitivity.

Worst observed |error| / bound over the three fixed shapes (gaussian_case,
seed 0) on MI355X: y 0.038, dx 0.088, dw1 0.027, db1 0.0061, dw2 0.0031, db2 0.012
("Learned feature extraction"); the test prints them."""
import numpy as np
import pytest
import torch

import extract_util as E

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def on(device, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def run(device, case, need_dx=True):
    """{"y", "dx", "dw1", ...} as numpy from the two ops."""
    from nsm_amd.extract import extract_backward, extract_forward
    x, dy, w1, b1, w2, b2, slope = case
    t = [on(device, a) for a in (x, dy, w1, b1, w2, b2)]
    y = extract_forward(t[0], t[2], t[3], t[4], t[5], slope)
    out = extract_backward(t[0], t[1], t[2], t[3], t[4], t[5], slope, need_dx=need_dx)
    res = {"y": y.cpu().numpy()}
    for k, v in zip(E.GRADS, out):
        res[k] = None if v is None else v.cpu().numpy()
    return res


def capped_shape():
    """A shape whose tiles exceed one pass of the capped grid by one tile and a
    ragged one, from the library's own plan."""
    from nsm_amd.extract import extract_bwd_plan
    plan = extract_bwd_plan(1, 3, 4096, 4096, 5, 2)
    cap, tu, up = plan["grid_cap"], plan["tile_units"], plan["unit_pixels"]
    W = 1019                                  # 255 units a row, the last one of 3 columns
    q = -(-W // up)
    H = -(-(cap * tu + tu + tu // 3) // q)
    shape = ((1, H, W), 3, 5, 2)
    got = extract_bwd_plan(1, 3, H, W, 5, 2)
    assert got["grid"] == cap and cap < got["tiles"] < 2 * cap
    assert (H * q) % tu != 0                  # the last tile is ragged
    return shape


@pytest.fixture(scope="module")
def int_cases():
    shapes = dict(E.SHAPES, capped=capped_shape())
    out = {}
    for name, (shape, Cin, Hd, Cout) in shapes.items():
        case = E.integer_case(shape, Cin, Hd, Cout, seed=1)
        out[name] = (case, E.reference(*case, sums=False))
    return out


@pytest.fixture(scope="module")
def real_cases():
    out = {}
    for name, (shape, Cin, Hd, Cout) in E.SHAPES.items():
        case = E.gaussian_case(shape, Cin, Hd, Cout, seed=0)
        out[name] = (case, E.reference(*case))
    return out


@pytest.mark.parametrize("name", ["w73", "w72", "tiny", "capped"])
def test_integer_case_is_bit_exact(device, int_cases, name):
    case, ref = int_cases[name]
    if name == "capped":   # the claim test_extract_ref makes for the fixed shapes
        for k in ("y",) + E.GRADS:
            v = getattr(ref, k)
            assert np.array_equal(v * 16, np.round(v * 16)) and np.abs(v).max() < 2 ** 24, k
    assert (ref.pre == 0).any()
    got = run(device, case)
    for k in ("y",) + E.GRADS:
        assert E.same_bits(got[k], getattr(ref, k)), (name, k)


@pytest.mark.parametrize("name", list(E.SHAPES))
def test_real_case_within_the_worst_case_bound(device, real_cases, name):
    case, ref = real_cases[name]
    got = run(device, case)
    worst = {}
    for k in ("y",) + E.GRADS:
        err = np.abs(got[k].astype(np.float64) - getattr(ref, k))
        bound = getattr(ref, "bound_" + k)
        assert (bound > 0).all(), k
        worst[k] = float((err / bound).max())
    print(f"extract {name}: worst |error| / bound " +
          " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (name, k, v)


def test_views_inside_larger_buffers(device, int_cases, real_cases):
    """x, dy, y and dx one float inside larger buffers: the bits of the contiguous
    call, and the sentinels around the outputs untouched."""
    from nsm_amd._lib import call, lib, ptr, stream
    for cases, name in ((real_cases, "w73"), (real_cases, "w72"), (int_cases, "tiny")):
        case = cases[name][0]
        x, dy, w1, b1, w2, b2, slope = case
        want = run(device, case)
        B, Cin, H, W = x.shape
        Hd, Cout = w1.shape[0], w2.shape[0]

        def inside(a, pad=4):
            buf = torch.full((a.size + 2 * pad + 1,), SENTINEL, dtype=torch.float32, device=device)
            view = buf[pad + 1:pad + 1 + a.size].view(a.shape)
            view.copy_(on(device, a))
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            return buf, view, pad

        xb, xv, _ = inside(x)
        dyb, dyv, _ = inside(dy)
        yb, yv, pad = inside(np.full(want["y"].shape, SENTINEL, np.float32))
        dxb, dxv, _ = inside(np.full(x.shape, SENTINEL, np.float32))
        p = [on(device, a) for a in (w1, b1, w2, b2)]
        call("nsm_extract_fwd", ptr(xv), B, Cin, H, W, ptr(p[0]), ptr(p[1]), Hd, ptr(p[2]),
             ptr(p[3]), Cout, slope, ptr(yv), stream())
        g = [torch.full_like(t, SENTINEL) for t in p]
        ws = torch.empty(lib.nsm_extract_bwd_ws(B, Cin, H, W, Hd, Cout) // 4, device=device)
        call("nsm_extract_bwd", ptr(xv), ptr(dyv), B, Cin, H, W, ptr(p[0]), ptr(p[1]), Hd,
             ptr(p[2]), ptr(p[3]), Cout, slope, ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]),
             ptr(dxv), ptr(ws), stream())
        assert E.same_bits(yv.cpu().numpy(), want["y"]), name
        assert E.same_bits(dxv.cpu().numpy(), want["dx"]), name
        for k, t in zip(("dw1", "db1", "dw2", "db2"), g):
            assert E.same_bits(t.cpu().numpy(), want[k]), (name, k)
        for buf, n in ((yb, yv.numel()), (dxb, dxv.numel())):
            assert (buf[:pad + 1] == SENTINEL).all() and (buf[pad + 1 + n:] == SENTINEL).all()
        # the inputs are read only
        assert torch.equal(xv, on(device, x)) and torch.equal(dyv, on(device, dy))


@pytest.mark.parametrize("name", ["w73", "tiny"])
def test_dx_off_gives_the_same_parameter_gradients(device, real_cases, name):
    case = real_cases[name][0]
    a, b = run(device, case, need_dx=True), run(device, case, need_dx=False)
    assert b["dx"] is None
    for k in ("dw1", "db1", "dw2", "db2"):
        assert E.same_bits(b[k], a[k]), k


def test_backward_is_deterministic(device, real_cases):
    case = real_cases["w73"][0]
    a, b = run(device, case), run(device, case)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run(device, case)
    torch.cuda.current_stream().wait_stream(side)
    for k in E.GRADS:
        assert E.same_bits(b[k], a[k]) and E.same_bits(c[k], a[k]), k


def test_module_against_its_cpu_path(device, real_cases):
    """FeatureExtractor on the GPU against the plain module on the CPU, at the
    real-valued bounds (both are fp32 evaluations of the same terms: twice the
    bound apart at most)."""
    from nsm_amd import FeatureExtractor
    (x, dy, w1, b1, w2, b2, slope), ref = real_cases["w73"]
    m = FeatureExtractor(15, 4, 16, slope)
    with torch.no_grad():
        for p, a in zip(m.net.parameters(), (w1[:, :, None, None], b1, w2[:, :, None, None], b2)):
            p.copy_(torch.from_numpy(a))
    xc = torch.from_numpy(x).requires_grad_(True)
    yc = m(xc)
    yc.backward(torch.from_numpy(dy))
    cpu = {"y": yc.detach().numpy(), "dx": xc.grad.numpy()}
    cpu.update(zip(("dw1", "db1", "dw2", "db2"), (p.grad.numpy().copy() for p in m.net.parameters())))
    m.zero_grad()
    m = m.to(device)
    xg = on(device, x).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):   # fp32 inside any autocast region
        yg = m(xg)
    assert yg.dtype == torch.float32
    yg.backward(on(device, dy))
    gpu = {"y": yg.detach().cpu().numpy(), "dx": xg.grad.cpu().numpy()}
    gpu.update(zip(("dw1", "db1", "dw2", "db2"), (p.grad.cpu().numpy() for p in m.net.parameters())))
    ops = run(device, real_cases["w73"][0])
    for k in ("y",) + E.GRADS:
        bound = getattr(ref, "bound_" + k)
        got = gpu[k].reshape(bound.shape)
        assert E.same_bits(got, ops[k]), k        # the module is the two ops
        assert (np.abs(got.astype(np.float64) - cpu[k].reshape(bound.shape)) <= 2 * bound).all(), k
    assert m(xg[0]).shape == (1, 4, 41, 73)
    with pytest.raises(ValueError, match="float32"):
        m(xg.half())


# ---- the cascade --------------------------------------------------------------------------
def cascade(device, seed=3, dropout=0.0):
    import nsm_amd
    torch.manual_seed(seed)
    m = nsm_amd.ExtractedUnet(nsm_amd.FeatureExtractor(15, 4),
                              nsm_amd.Unet(in_ch=4, dropout_rate=dropout)).to(device).train()
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(2, 15, 32, 32, device=device, generator=g)
    y = torch.rand(2, 1, 32, 32, device=device, generator=g)
    return m, x, y


def test_cascade_backward(device):
    import nsm_amd
    from nsm_amd.extract import extract_backward
    m, x, y = cascade(device)
    crit = nsm_amd.CustomLoss(device, 0.9, vgg_weights=False)
    crit(m(x), y, x).backward()
    params = list(m.parameters())
    assert len(params) == 4 + len(list(m.unet.parameters())) == 70
    for p in params:
        assert p.grad is not None and torch.isfinite(p.grad).all() and (p.grad != 0).any()
    # the op alone, fed the x.grad the U-Net yields for the detached extractor output
    with torch.no_grad():
        z = m.extractor(x)
    z.requires_grad_(True)
    crit(m.unet(z), y, z).backward()
    c1, c2 = m.extractor.net[0], m.extractor.net[2]
    dx, *grads = extract_backward(x, z.grad, c1.weight, c1.bias, c2.weight, c2.bias,
                                  m.extractor.negative_slope, need_dx=False)
    assert dx is None
    for got, p in zip(grads, (c1.weight, c1.bias, c2.weight, c2.bias)):
        assert got.shape == p.grad.shape and torch.equal(got, p.grad)


def test_cascade_graphed_step_equals_eager_steps(device):
    import nsm_amd

    def setup():
        m, x, y = cascade(device)
        opt = nsm_amd.make_optimizer(m.parameters(), "adamw", 1e-3, max_grad_norm=1.0,
                                     sanitize=True, seed=11)
        return m, opt, nsm_amd.CustomLoss(device, 0.9, vgg_weights=False), x, y

    def state(m, opt):
        return [t.detach().clone() for t in [opt.flat, opt.exp_avg, opt.exp_avg_sq]
                + list(m.buffers())]

    m, opt, crit, x, y = setup()
    m2, opt2, crit2, _, _ = setup()
    # the extractor's parameters are re-homed into the flat buffer like the others
    lo, hi = opt.flat.data_ptr(), opt.flat.data_ptr() + opt.flat.numel() * 4
    assert all(lo <= p.data_ptr() < hi for p in m.parameters())
    assert opt.flat.numel() >= sum(p.numel() for p in m.parameters())
    step = nsm_amd.GraphedTrainStep(m, crit, opt, x, y, warmup=2)
    losses = [step().item() for _ in range(3)]
    assert step.captures == 1
    ref = []
    for _ in range(3):
        loss = crit2(m2(x), y, x)
        loss.backward()
        opt2.step()
        opt2.zero_grad()
        ref.append(loss.item())
    assert losses == ref, (losses, ref)
    for a, b in zip(state(m, opt), state(m2, opt2)):
        assert torch.equal(a, b)
    for a, b in zip(m.parameters(), m2.parameters()):
        assert torch.equal(a, b)
    moved = cascade(device)[0]
    assert not torch.equal(m.extractor.net[0].weight, moved.extractor.net[0].weight)


def test_cascade_perturbation_criterion(device):
    """The non-fused perturbation criterion only calls model(x); the fused one
    finds the U-Net's prepared layouts through `.unet` and gives the same step."""
    import nsm_amd
    res = []
    for fused in (False, True):
        m, x, y = cascade(device)
        crit = nsm_amd.EnhancedCustomLoss(device, alpha=0.9, perturb_weight=0.1, vgg=None,
                                          perturbation_count=2, vgg_weights=False, fused=fused).train()
        g = torch.Generator(device=device).manual_seed(9)
        noises = [0.01 * torch.randn(x.shape, device=device, generator=g) for _ in range(2)]
        total, parts = crit(m, m(x), y, x, noises=noises)
        total.backward()
        assert torch.isfinite(total) and float(parts["perturbation_loss"].detach()) > 0
        gw = m.extractor.net[0].weight.grad
        assert torch.isfinite(gw).all() and (gw != 0).any()
        res.append((total.item(), gw.clone()))
    assert abs(res[0][0] - res[1][0]) <= 1e-5 * abs(res[0][0])


def recipe15():
    from nsm_amd import FeatureRecipe
    layout = {"d": 0, "n": 1, "z": 4, "ne": 5, "zf": 8, "ce": 9, "cc": 10}
    raw = ["d", "n", "z", "ne", "zf", "ce", "cc"]
    terms = [("raw", i) for i in range(11)]
    r = FeatureRecipe.parse(["z-zf", "z/zf", "cc/d", "n.ne"], layout, in_channels=11)
    return FeatureRecipe(terms + list(r.terms), 11), raw


def test_cascade_inference(device):
    import nsm_amd
    m, x, y = cascade(device, dropout=0.2)
    opt = nsm_amd.FlatAdamW(m.parameters(), lr=1e-2, weight_decay=0.0, sanitize=True, seed=1)
    crit = nsm_amd.CustomLoss(device, 0.9, vgg_weights=False)
    g = nsm_amd.GraphedUnet(m, x)
    assert m.training

    def eager(inp):
        m.eval()
        with torch.no_grad():
            o = m(inp)
        m.train()
        return o

    assert torch.equal(g(x), eager(x))
    before = g(x).clone()
    w_ext, w_unet = m.extractor.net[2].weight.clone(), m.unet.conv10.weight.clone()
    crit(m(x), y, x).backward()
    opt.step()
    opt.zero_grad()
    assert not torch.equal(w_ext, m.extractor.net[2].weight)
    assert not torch.equal(w_unet, m.unet.conv10.weight)
    after = g(x)
    assert torch.equal(after, eager(x)) and not torch.equal(after, before)
    # new extractor weights alone reach the replay too (read live, at fixed addresses)
    with torch.no_grad():
        m.extractor.net[2].bias.add_(0.25)
    assert torch.equal(g(x), eager(x))

    # raw buffers -> the 15 channels of U -> extractor -> U-Net -> 8-bit frame, one graph
    r, _ = recipe15()
    gen = torch.Generator().manual_seed(4)
    raw = (torch.rand(1, 11, 41, 73, generator=gen) + 0.25).to(device)
    stats = (0.1 * torch.randn(15, generator=gen), torch.rand(15, generator=gen) + 0.5)
    pipe = nsm_amd.FramePipeline(m, raw, recipe=r, stats=stats, crop=True)
    assert pipe.static_in.shape == (1, 15, 48, 80)
    u8 = pipe(raw)
    xin = nsm_amd.compose_features(raw, r, pad_multiple=16, scrub=True, stats=stats)
    o = eager(xin)
    shadow = torch.empty((1, o.shape[1], 41, 73), dtype=torch.float32, device=device)
    want = nsm_amd.finish_frames(o, (41, 73), out_f32=shadow)
    assert torch.equal(pipe.static_in, xin)
    assert torch.equal(u8, want) and torch.equal(pipe.shadow, shadow)


def test_sensitivity_through_the_extractor(device):
    """feature_sensitivity ranks the 15 channels of U through the extractor."""
    import nsm_amd
    m, x, _ = cascade(device)
    s = nsm_amd.feature_sensitivity(m, x, sigma=1.0, repeats=2, chunk=4, seed=3).absolute
    assert s.numel() == 15 and torch.isfinite(s).all() and (s > 0).all()
    # a channel the extractor ignores has no sensitivity
    with torch.no_grad():
        m.extractor.net[0].weight[:, 7] = 0
    s = nsm_amd.feature_sensitivity(m, x, sigma=1.0, repeats=2, chunk=4, seed=3).absolute
    assert float(s[7]) == 0.0 and (s[:7] > 0).all()
