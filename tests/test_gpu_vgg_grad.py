"""GPU: the differentiable VGG19 perceptual loss (MultiLayerVGGLoss(
differentiable=True), CustomLoss(vgg_grad=True)): the three element-wise
backward kernels against ATen on the CPU, features.0's input gradient, the
whole chain against a float64 gradient with the discrete decisions held fixed
and against plain float64 autograd, and the interface (loss scale, CustomLoss,
through the U-Net, inside GraphedTrainStep)."""
import pytest
import torch
import torch.nn.functional as F

import vgg_grad_util as U
from oracle import vgg_ref as V
from oracle.weights import make_state
from util import load

pytestmark = pytest.mark.gpu
torch.set_num_threads(16)

ELEM = dict(rtol=1e-6, atol=0)   # the tolerance of test_l1_loss for the same arithmetic
# sum of the per-convolution input-gradient tolerances along the chain: the 11
# Winograd F(4x4) convs at WINO_TOL[4]["dgrad"] = 1e-4 (test_gpu_ops.py) and the
# 3 direct convs at test_conv_dgrad's 1e-5
CHAIN_FIXED_REL = 11 * 1e-4 + 3 * 1e-5
# vs plain float64 autograd: above the sign / mask flips that feature rounding
# of relative size 1e-6..1e-5 causes (0.7e-3 .. 1.6e-2 measured on the float64
# reference alone), six times below the smallest structural defect (a missing
# tap: 0.18)
CHAIN_AUTOGRAD_REL = 3e-2


@pytest.fixture(scope="module")
def ops(device):
    from nsm_amd import ops as O
    return O


def vgg_module(device, **kw):
    import nsm_amd
    return nsm_amd.MultiLayerVGGLoss(device, state_dict=V.standin_state(), **kw)


def quantised(shape, gen):
    """Integers in [-2, 2]: ties, all-negative windows and exact zeros are frequent."""
    return torch.randint(-2, 3, shape, generator=gen).float()


# ---- kernels ----------------------------------------------------------------
@pytest.mark.parametrize("tap", [False, True])
@pytest.mark.parametrize("B,H,W,C", [(2, 2, 2, 32), (1, 5, 9, 64), (1, 6, 8, 128)])
def test_maxpool2_bwd(ops, device, B, H, W, C, tap):
    gen = torch.Generator().manual_seed(100 * H + W + C)
    x = quantised((B, C, H, W), gen).requires_grad_(True)
    t = quantised((B, C, H, W), gen)
    gp = torch.randn(B, C, H // 2, W // 2, generator=gen)
    F.max_pool2d(F.relu(x), 2, 2).backward(gp)
    routed = x.grad
    coef, gs = 0.37, torch.tensor(3.0)
    got = ops.maxpool2_bwd(U.nhwc(gp).to(device), U.nhwc(x.detach()).to(device),
                           U.nhwc(t).to(device) if tap else None, B, H, W, coef,
                           gs.to(device))
    got = U.nchw(got.cpu(), B, H, W)
    # the cases the quantisation is there for are present
    m = F.max_pool2d(x.detach(), 2, 2)
    assert H * W < 8 or ((m < 0).any() and (m == 0).any())
    He, We = H // 2 * 2, W // 2 * 2
    if not tap:
        assert torch.equal(got, routed)          # pure routing
        assert (got[:, :, He:, :] == 0).all() and (got[:, :, :, We:] == 0).all()
        return
    term = (torch.tensor(coef) * gs) * torch.sign(x.detach() - t)
    torch.testing.assert_close(got, routed + term, **ELEM)
    # the odd trailing row / column: no pooled gradient, the tap term alone
    assert torch.equal(got[:, :, He:, :], term[:, :, He:, :])
    assert torch.equal(got[:, :, :, We:], term[:, :, :, We:])


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("tap", [False, True])
def test_tap_relu_bwd(ops, device, relu, tap):
    gen = torch.Generator().manual_seed(5)
    rows, C = 301, 64                         # 19 blocks of 256 lanes x 4 floats
    y = (quantised((rows, C), gen) * 0.5).requires_grad_(True)
    t = quantised((rows, C), gen) * 0.5
    g = torch.randn(rows, C, generator=gen)
    assert (y == t).any() and (y == 0).any() and (y < 0).any()
    coef, gs = 0.25 / (rows * C), torch.tensor(3.0)
    mag = torch.tensor(coef) * gs
    loss = ((F.relu(y) if relu else y) * g).sum()
    if tap:
        loss = loss + mag * (y - t).abs().sum()
    loss.backward()
    got = ops.vgg_tap_relu_bwd(g.to(device), y.detach().to(device), t.to(device) if tap else None,
                               coef, gs.to(device), relu=relu)
    torch.testing.assert_close(got.cpu(), y.grad, **ELEM)


def test_tap_bwd_without_incoming_gradient(ops, device):
    """The last tap: nothing arrives from above, the kernel writes the tap term."""
    gen = torch.Generator().manual_seed(6)
    rows, C = 301, 64
    y, t = quantised((rows, C), gen) * 0.5, quantised((rows, C), gen) * 0.5
    coef, gs = 0.1 / (rows * C), torch.tensor(1024.0)
    got = ops.vgg_tap_relu_bwd(None, y.to(device), t.to(device), coef, gs.to(device), relu=True)
    ref = (torch.tensor(coef) * gs) * torch.sign(y - t)
    torch.testing.assert_close(got.cpu(), ref, **ELEM)
    assert (got.cpu()[y == t] == 0).all()


def test_vgg_prep_bwd(ops, device):
    gen = torch.Generator().manual_seed(7)
    B, H, W = 2, 9, 37                        # 666 pixels: 3 blocks
    o = torch.rand(B, 1, H, W, generator=gen) * 1.4 - 0.2
    flat = o.view(-1)
    flat[:5] = torch.tensor([0.0, 1.0, -0.1, 1.1, float("nan")])
    flat[300:305] = torch.tensor([1.0, 0.0, float("nan"), -0.1, 1.1])
    o.requires_grad_(True)
    # one sign per pixel: the kernel sums the three channels before dividing,
    # ATen divides first; without cancellation the two agree to a few ulp
    g3 = (torch.rand(B, 3, H, W, generator=gen) + 0.5) * torch.sign(
        torch.randn(B, 1, H, W, generator=gen))
    V.prep(o).backward(g3)
    ref = o.grad
    g32 = torch.randn(B * H * W, 32, generator=gen)   # channels 3..31 must be ignored
    g32[:, :3] = U.nhwc(g3)
    base = torch.randn(B, 1, H, W, generator=gen)
    denom = float(torch.tensor(V.STD) + torch.tensor(V.EPS))
    g32d, od = g32.to(device), o.detach().to(device)
    grad = torch.full((B, 1, H, W), float("nan"), device=device)   # written, not read
    ops.vgg_prep_bwd(g32d, od, denom, grad)
    got = grad.cpu()
    torch.testing.assert_close(got, ref, **ELEM)
    # 0.0 and 1.0 pass; -0.1, 1.1 and NaN give exactly 0
    assert (got.view(-1)[[0, 1, 300, 301]] != 0).all()
    assert (got.view(-1)[[2, 3, 4, 302, 303, 304]] == 0).all()
    acc = base.to(device)
    ops.vgg_prep_bwd(g32d, od, denom, acc, accumulate=True)
    assert torch.equal(acc.cpu(), base + got)
    half = torch.full((B, 1, H, W), float("nan"), device=device)
    ops.vgg_prep_bwd(g32d, od, denom, half, scale=0.5)
    assert torch.equal(half.cpu(), 0.5 * got)


def test_features0_input_gradient(ops, device):
    """conv 3 -> 64 with the input padded to 32 channels (the PACK_DGRAD pack
    through the implicit-GEMM conv)."""
    gen = torch.Generator().manual_seed(8)
    B, H, W = 1, 5, 7
    w = V.standin_state()["0.weight"]
    x = torch.randn(B, 3, H, W, generator=gen, requires_grad=True)
    dy = torch.randn(B, 64, H, W, generator=gen)
    F.conv2d(x, w, padding=1).backward(dy)
    wd = ops.pack_conv_weight(w.to(device), 64, 32, ops.PACK_DGRAD)
    dx = ops.conv_fwd(U.nhwc(dy).to(device), B, H, W, wd, None, 32, 3).cpu()
    assert dx.shape == (B * H * W, 32)
    assert U.rel(U.nchw(dx[:, :3], B, H, W), x.grad) <= 1e-5
    assert (dx[:, 3:] == 0).all()


# ---- the chain --------------------------------------------------------------
_GPU = {}


def gpu_run(device, name):
    """One differentiable forward + backward of a case on the GPU (shared):
    loss, gradient and the kept activations as [2B, C, h, w] on the CPU."""
    if name not in _GPU:
        o, t = U.inputs(name)
        B, _, H, W = o.shape
        m = vgg_module(device, differentiable=True, keep_acts=True)
        od = o.to(device).requires_grad_(True)
        loss = m(od, t.to(device))
        loss.backward()
        acts = {}
        pools = [i for i, kind, _, _ in V.layers() if kind == "pool"]
        for idx, a in m.last_acts.items():
            d = 2 ** sum(p < idx for p in pools)
            assert a.shape[0] == 2 * B * (H // d) * (W // d)
            acts[idx] = U.nchw(a.cpu(), 2 * B, H // d, W // d)
        plain = vgg_module(device)
        _GPU[name] = (loss.detach().cpu(), od.grad.cpu(), acts, plain(od.detach(), t.to(device)).cpu(),
                      plain.last_acts)
    return _GPU[name]


@pytest.mark.parametrize("name", ["b1_40x72", "b2_96x128"])
def test_chain_with_decisions_fixed(device, name):
    """Every discrete decision (sign(y - t) at the taps, y > 0, the argmax of
    each window) taken from the GPU forward's own activations: the remaining
    map is linear, and only the rounding of the input-gradient GEMMs is left.
    At 40x72 the pools see 5x9 -> 2x4 (the odd edge); 96x128 has whole and
    partial Winograd tiles."""
    o, _ = U.inputs(name)
    _, grad, acts, _, _ = gpu_run(device, name)
    assert sorted(acts) == list(U.CONV_IDX)
    ref = U.fixed_decision_grad(o, acts)
    err = U.rel(grad, ref)
    print(f"{name}: chain vs fixed-decision float64 rel-L2 {err:.3e} (bound {CHAIN_FIXED_REL:.1e})")
    assert ref.abs().max() > 0
    assert err <= CHAIN_FIXED_REL


@pytest.mark.parametrize("name", ["b1_40x72", "b2_96x128", "b1_32x48"])
def test_chain_vs_float64_autograd(device, name):
    loss, grad, _, plain_loss, plain_acts = gpu_run(device, name)
    ref_loss, ref, _ = U.autograd64(name)
    err = U.rel(grad, ref)
    print(f"{name}: chain vs float64 autograd rel-L2 {err:.3e} (bound {CHAIN_AUTOGRAD_REL:.0e}); "
          f"loss {loss.item():.8e} ref {ref_loss.item():.8e}")
    assert err <= CHAIN_AUTOGRAD_REL
    # the differentiable forward is the default one: the same value bitwise
    assert torch.equal(loss, plain_loss)
    assert plain_acts is None
    assert abs(loss.item() - ref_loss.item()) <= 2e-5 * abs(ref_loss.item())


# ---- interface --------------------------------------------------------------
def test_loss_scale_is_exact(device):
    """The upstream gradient is read on the device at the taps; a power-of-two
    seed scales every later pass exactly."""
    o, t = U.inputs("b1_32x48")
    m = vgg_module(device, differentiable=True)
    grads = []
    for seed in (None, torch.tensor(1024.0, device=device)):
        od = o.to(device).requires_grad_(True)
        m(od, t.to(device)).backward(seed)
        grads.append(od.grad)
    assert grads[0].abs().max() > 0
    assert torch.equal(grads[1], 1024.0 * grads[0])
    assert m.last_acts is None


def test_custom_loss_vgg_grad(device):
    import nsm_amd
    o, t = U.inputs("b1_32x48")
    sd = V.standin_state()
    od = o.to(device).requires_grad_(True)
    crit = nsm_amd.CustomLoss(device, alpha=0.9, vgg_weights=sd, vgg_grad=True)
    loss = crit(od, t.to(device), None)
    loss.backward()
    o2 = o.to(device).requires_grad_(True)
    vgg_module(device, differentiable=True)(o2, t.to(device)).backward()
    # the reference is formed on the CPU: there `/ N` is an IEEE division, as in
    # nsm_l1_loss_bwd, while ATen's device kernel multiplies by 1/N (one ulp of
    # the L1 term, which the near-cancelling elements of the sum would magnify)
    ref = 0.9 * torch.sign(o - t) / o.numel() + 0.1 * o2.grad.cpu()
    torch.testing.assert_close(od.grad.cpu(), ref, **ELEM)
    assert (0.1 * o2.grad).abs().max() > 1e-3 * (0.9 / o.numel())   # the VGG part is not noise
    # the value is the default CustomLoss's
    plain = nsm_amd.CustomLoss(device, alpha=0.9, vgg_weights=sd)(od.detach(), t.to(device), None)
    assert torch.equal(loss.detach(), plain)


def test_enhanced_custom_loss_vgg_grad(device):
    import nsm_amd
    o, t = U.inputs("b1_32x48")
    od = o.to(device).requires_grad_(True)
    crit = nsm_amd.EnhancedCustomLoss(device, alpha=0.9, vgg_weights=V.standin_state(),
                                      vgg_grad=True).eval()
    total, _ = crit(None, od, t.to(device), None)
    total.backward()
    o2 = o.to(device).requires_grad_(True)
    vgg_module(device, differentiable=True)(o2, t.to(device)).backward()
    # two autograd nodes here: the L1 part is exact, and the VGG chain ran with
    # the upstream 0.1 applied at the taps instead of after it. Same forward,
    # same decisions, so both are the same linear map, each within the chain's
    # GEMM-rounding allowance of the exact one
    l1 = 0.9 * torch.sign(o - t) / o.numel()      # on the CPU: an IEEE division, as the kernel's
    err = U.rel(od.grad.cpu() - l1, 0.1 * o2.grad.cpu())
    print(f"EnhancedCustomLoss VGG part vs standalone rel-L2 {err:.3e}")
    assert err <= 2 * CHAIN_FIXED_REL


def _unet_step(device, vgg_grad):
    import nsm_amd
    fx = load("train_c7_p0_b2_64")
    in_ch = int(fx["meta/in_ch"])
    m = nsm_amd.Unet(in_ch=in_ch, dropout_rate=0.0)
    m.load_state_dict({k: torch.from_numpy(v.copy())
                       for k, v in make_state(in_ch, int(fx["meta/seed_w"])).items()})
    m = m.to(device).train()
    crit = nsm_amd.CustomLoss(device, alpha=0.9, vgg_weights=V.standin_state(), vgg_grad=vgg_grad)
    x, y = torch.from_numpy(fx["x"]).to(device), torch.from_numpy(fx["y"]).to(device)
    out = m(x)
    out.retain_grad()
    crit(out, y, x).backward()
    return m, crit, out, y


def test_vgg_grad_through_unet(device):
    m, crit, out, y = _unet_step(device, True)
    leaf = out.detach().clone().requires_grad_(True)
    crit(leaf, y, None).backward()
    assert torch.equal(out.grad, leaf.grad)
    m1, _, out1, _ = _unet_step(device, False)
    assert torch.equal(out1, out)
    differ = [k for (k, a), (_, b) in zip(m.named_parameters(), m1.named_parameters())
              if not torch.equal(a.grad, b.grad)]
    assert len(differ) > len(list(m.parameters())) // 2, differ


def _setup(device, p, seed=3, B=2, C=7, H=64):
    import nsm_amd
    torch.manual_seed(seed)
    m = nsm_amd.Unet(in_ch=C, dropout_rate=p).to(device).train()
    opt = nsm_amd.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-3, max_grad_norm=1.0,
                            sanitize=True, seed=11)
    crit = nsm_amd.CustomLoss(device, 0.9, vgg_weights=V.standin_state(), vgg_grad=True)
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(B, C, H, H, device=device, generator=g)
    y = torch.rand(B, 1, H, H, device=device, generator=g)
    return m, opt, crit, x, y


def _state(m, opt):
    return [t.detach().clone() for t in [opt.flat, opt.exp_avg, opt.exp_avg_sq]
            + list(m.buffers())]


def test_graphed_step_with_vgg_grad_equals_eager_steps(device):
    """The model, size and assertions of test_graphed_step_equals_eager_steps,
    with the VGG term carrying its gradient: three replays equal three eager
    steps bitwise, and building the step leaves the training state untouched."""
    import nsm_amd
    m, opt, crit, x, y = _setup(device, 0.0)
    m2, opt2, crit2, _, _ = _setup(device, 0.0)
    before = _state(m, opt)
    step = nsm_amd.GraphedTrainStep(m, crit, opt, x, y, warmup=2)
    for a, b in zip(before, _state(m, opt)):
        assert torch.equal(a, b)
    losses = [step().item() for _ in range(3)]
    ref = []
    for _ in range(3):
        loss = crit2(m2(x), y, x)
        loss.backward()
        opt2.step()
        opt2.zero_grad()
        ref.append(loss.item())
    assert losses == ref, (losses, ref)
    for a, b in zip(_state(m, opt), _state(m2, opt2)):
        assert torch.equal(a, b)
