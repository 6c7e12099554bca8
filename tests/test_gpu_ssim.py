"""GPU: the opt-in SSIM term and metric (nsm_ssim_fwd/bwd) against the float64
restatement of pytorch_msssim.ssim (ssim_util.py) on the same float32 inputs,
and the interface: per-image values, data_range 255, identical inputs, seed
scaling, determinism, CustomLoss with and without detail weights and the VGG
gradient, the untouched default mode, through the U-Net, inside
GraphedTrainStep, EnhancedCustomLoss and the refusals.

No fixture comes from running the reference: customLoss.py:187-191 is commented
out there (the term never executes) and pytorch_msssim is not installed."""
import pytest
import torch

import detail_util as D
import ssim_util as U
from oracle.weights import make_state
from util import load

pytestmark = pytest.mark.gpu
torch.set_num_threads(16)

ELEM = dict(rtol=1e-6, atol=0)
CASES = [(s, f, r) for f in U.FAMILIES for r in U.RANGES for s in U.SHAPES]
IDS = [f"{f}-R{int(r)}-" + "x".join(map(str, s)) for s, f, r in CASES]

# A kernel error may be at most max(2 x the float32 restatement's own error on
# that case, floor). The floors are 4 x the kernel's worst measured error over
# the random cases (MI355X; the restatement's own worst there in brackets):
GRAD_REL_L2_FLOOR = 7e-7   # measured 1.73e-7 (restatement 6.2e-7)
GRAD_PIXEL_FLOOR = 1.4e-6  # measured 3.52e-7 (restatement 7.7e-7), times max|g|
VALUE_FLOOR = 7.6e-7       # absolute; measured 1.89e-7 per image, 8.1e-8 batch (restatement 2.6e-7)
# Smooth cases, measured worst (kernel | restatement): R = 1: rel-L2 1.2e-5 | 5.6e-5,
# pixel 2.9e-5 | 1.4e-4, value 7.5e-7 | 8.8e-6; R = 255: rel-L2 2.0e-7 | 5.7e-6,
# pixel 2.2e-7 | 4.9e-6: the difference-form moments sit 4 to 25 times below it.


def loss_grad(device, o, t, data_range=1.0, seed=None):
    import nsm_amd
    od = o.to(device).requires_grad_(True)
    loss = nsm_amd.ssim_loss(od, t.to(device), data_range)
    loss.backward(seed)
    return loss.detach(), od.grad


def weighted_grad(device, o, t, w, data_range=1.0):
    """d(w * (1 - ssim))/do from its own kernel call."""
    from nsm_amd.losses import _SsimFn
    od = o.to(device).requires_grad_(True)
    _SsimFn.apply(od, t.to(device), w, data_range)[0].backward()
    return od.grad


# ---- kernels ----------------------------------------------------------------
@pytest.mark.parametrize("shape,family,data_range", CASES, ids=IDS)
def test_accuracy(device, shape, family, data_range):
    """Value, per-image values (leakage between images) and gradient; every
    pixel counts."""
    import nsm_amd
    o, t, (per, val, grad), _ = U.reference(shape, family, data_range)
    f_rel, f_pix, f_val, f_per = U.f32_errors(shape, family, data_range)
    loss, g = loss_grad(device, o, t, data_range)
    od, td = o.to(device), t.to(device)
    got = nsm_amd.ssim(od, td, data_range)
    got_per = nsm_amd.ssim(od, td, data_range, size_average=False)
    assert got.dim() == 0 and got_per.shape == (shape[0],) and not got.requires_grad
    rel, pix = U.grad_errors(-g.cpu(), grad)
    e_val = abs(got.item() - val)
    e_per = (got_per.cpu().double() - per).abs().max().item()
    e_loss = abs(loss.item() - (1 - val))
    print(f"{family} R={data_range} {shape}: ssim {val:.7f} | kernel grad rel-L2 {rel:.2e} "
          f"pixel {pix:.2e} value {e_val:.2e} per-image {e_per:.2e} loss {e_loss:.2e} | float32 "
          f"restatement {f_rel:.2e} {f_pix:.2e} {f_val:.2e} {f_per:.2e}")
    assert grad.abs().max() > 0
    assert rel <= max(2 * f_rel, GRAD_REL_L2_FLOOR)
    assert pix <= max(2 * f_pix, GRAD_PIXEL_FLOOR)
    assert e_val <= max(2 * f_val, VALUE_FLOOR)
    assert e_per <= max(2 * f_per, VALUE_FLOOR)
    assert e_loss <= max(2 * f_val, VALUE_FLOOR)


def test_identical_inputs(device):
    import nsm_amd
    for family in U.FAMILIES:
        o, _ = U.inputs((3, 1, 27, 75), family)
        loss, g = loss_grad(device, o, o.clone())
        assert abs(loss.item()) <= 1e-6
        assert abs(1 - nsm_amd.ssim(o.to(device), o.to(device)).item()) <= 1e-6
        assert torch.isfinite(g).all()


def test_seed_scaling_is_exact(device):
    o, t = U.inputs((3, 1, 27, 75), "random")
    _, g1 = loss_grad(device, o, t)
    _, g2 = loss_grad(device, o, t, seed=torch.tensor(1024.0, device=device))
    assert g1.abs().max() > 0
    assert torch.equal(g2, 1024.0 * g1)


def test_determinism(device):
    import nsm_amd
    o, t = U.inputs((2, 1, 40, 90), "smooth")
    runs = []
    for _ in range(2):
        loss, g = loss_grad(device, o, t)
        runs.append((loss, g, nsm_amd.ssim(o.to(device), t.to(device), size_average=False)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_zero_weight_contributes_zero(device):
    o, t = U.inputs((2, 1, 40, 90), "random")
    assert (weighted_grad(device, o, t, 0.0) == 0).all()


# ---- CustomLoss --------------------------------------------------------------
def _l1_grad(device, o, t):
    import nsm_amd
    od = o.to(device).requires_grad_(True)
    nsm_amd.l1_loss(od, t.to(device), 0.9).backward()
    return od.grad.cpu()


def _detail_grad(device, o, t, dw, gw):
    """The three weighted detail gradients, each from its own kernel call,
    summed in the kernel's order (test_gpu_detail._pieces)."""
    import nsm_amd
    parts = []
    for w in ((dw, 0.0, 0.0), (0.0, dw, 0.0), (0.0, 0.0, gw)):
        od = o.to(device).requires_grad_(True)
        nsm_amd.detail_loss(od, t.to(device), *w).backward()
        parts.append(od.grad.cpu())
    return (parts[0] + parts[1]) + parts[2]


@pytest.mark.parametrize("dw,gw", [(0.0, 0.0), (0.1, 0.2)], ids=["alone", "with-detail"])
def test_custom_loss_ssim(device, dw, gw):
    import nsm_amd
    o, t = D.inputs((2, 1, 40, 90))
    od, td = o.to(device).requires_grad_(True), t.to(device)
    kw = dict(vgg_weights=False, detail_weight=dw, gradient_weight=gw)
    crit = nsm_amd.CustomLoss(device, 0.9, ssim_weight=0.1, **kw)
    loss = crit(od, td, None)
    assert loss.dim() == 0
    loss.backward()
    enhanced = nsm_amd.CustomLoss(device, 0.9, **kw)(od.detach(), td, None).cpu()
    s = nsm_amd.ssim(od.detach(), td).cpu()
    torch.testing.assert_close(loss.detach().cpu(), enhanced + 0.1 * (1 - s), **ELEM)
    want = _l1_grad(device, o, t)
    if dw or gw:
        want = want + _detail_grad(device, o, t, dw, gw)
    part = weighted_grad(device, o, t, 0.1).cpu()
    torch.testing.assert_close(od.grad.cpu(), want + part, **ELEM)
    # the SSIM part is not noise beside alpha/N
    assert part.abs().max() > 1e-2 * (0.9 / o.numel())


def test_custom_loss_ssim_with_vgg_grad(device):
    import nsm_amd
    o, t = D.inputs((2, 1, 32, 48))
    td = t.to(device)
    vgg = nsm_amd.CustomLoss(device, 0.9, vgg_weights="random").vgg_loss
    part = weighted_grad(device, o, t, 0.1).cpu()
    for dw, gw in ((0.0, 0.0), (0.1, 0.1)):
        kw = dict(vgg_weights=vgg, vgg_grad=True, detail_weight=dw, gradient_weight=gw)
        od = o.to(device).requires_grad_(True)
        loss = nsm_amd.CustomLoss(device, 0.9, ssim_weight=0.1, **kw)(od, td, None)
        loss.backward()
        o2 = o.to(device).requires_grad_(True)
        base = nsm_amd.CustomLoss(device, 0.9, **kw)(o2, td, None)
        base.backward()
        s = nsm_amd.ssim(o2.detach(), td).cpu()
        torch.testing.assert_close(loss.detach().cpu(), base.detach().cpu() + 0.1 * (1 - s), **ELEM)
        torch.testing.assert_close(od.grad.cpu(), o2.grad.cpu() + part, **ELEM)
        assert not torch.equal(o2.grad.cpu(), _l1_grad(device, o, t))   # the VGG chain contributed
    # the detached default composes too: the value moves, the gradient is L1 + SSIM
    o3 = o.to(device).requires_grad_(True)
    l3 = nsm_amd.CustomLoss(device, 0.9, vgg_weights=vgg, ssim_weight=0.1)(o3, td, None)
    l3.backward()
    o4 = o.to(device).requires_grad_(True)
    l4 = nsm_amd.CustomLoss(device, 0.9, vgg_weights=vgg, vgg_grad=True, ssim_weight=0.1)(o4, td, None)
    torch.testing.assert_close(l3.detach(), l4.detach(), **ELEM)
    torch.testing.assert_close(o3.grad.cpu(), _l1_grad(device, o, t) + part, **ELEM)


@pytest.mark.parametrize("dw,gw", [(0.0, 0.0), (0.1, 0.2)], ids=["plain", "with-detail"])
def test_default_mode_is_untouched(device, dw, gw):
    import nsm_amd
    o, t = D.inputs((2, 1, 40, 72))
    res = []
    for kw in ({}, dict(ssim_weight=0), dict(ssim_weight=0.0, ssim_data_range=255.0)):
        od = o.to(device).requires_grad_(True)
        loss = nsm_amd.CustomLoss(device, 0.9, vgg_weights=False, detail_weight=dw,
                                  gradient_weight=gw, **kw)(od, t.to(device), None)
        loss.backward()
        res.append((loss.detach(), od.grad, type(loss.grad_fn).__name__))
    for r in res[1:]:
        assert torch.equal(res[0][0], r[0]) and torch.equal(res[0][1], r[1])
        assert r[2] == res[0][2] == ("_CustomDetailFnBackward" if dw else "_L1FnBackward")


# ---- in the training step ------------------------------------------------------
def _crit(device):
    import nsm_amd
    return nsm_amd.CustomLoss(device, 0.9, vgg_weights=False, ssim_weight=0.1)


def test_ssim_through_unet(device):
    import nsm_amd
    fx = load("train_c7_p0_b2_64")
    in_ch = int(fx["meta/in_ch"])
    m = nsm_amd.Unet(in_ch=in_ch, dropout_rate=0.0)
    m.load_state_dict({k: torch.from_numpy(v.copy())
                       for k, v in make_state(in_ch, int(fx["meta/seed_w"])).items()})
    m = m.to(device).train()
    x, y = torch.from_numpy(fx["x"]).to(device), torch.from_numpy(fx["y"]).to(device)
    grads = []
    for crit in (_crit(device), nsm_amd.CustomLoss(device, 0.9, vgg_weights=False)):
        m.zero_grad(set_to_none=True)
        out = m(x)
        out.retain_grad()
        crit(out, y, x).backward()
        leaf = out.detach().clone().requires_grad_(True)
        crit(leaf, y, None).backward()
        assert torch.equal(out.grad, leaf.grad)
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
        grads.append([p.grad.clone() for p in m.parameters()])
    # the parameter gradients differ from the L1-only run
    assert any(not torch.equal(a, b) for a, b in zip(*grads))


def _setup(device, seed=3, B=2, C=7, H=64):
    import nsm_amd
    torch.manual_seed(seed)
    m = nsm_amd.Unet(in_ch=C, dropout_rate=0.0).to(device).train()
    opt = nsm_amd.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-3, max_grad_norm=1.0,
                            sanitize=True, seed=11)
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(B, C, H, H, device=device, generator=g)
    y = torch.rand(B, 1, H, H, device=device, generator=g)
    return m, opt, _crit(device), x, y


def _state(m, opt):
    return [t.detach().clone() for t in [opt.flat, opt.exp_avg, opt.exp_avg_sq]
            + list(m.buffers())]


def test_graphed_step_with_ssim_equals_eager_steps(device):
    import nsm_amd
    m, opt, crit, x, y = _setup(device)
    m2, opt2, crit2, _, _ = _setup(device)
    step = nsm_amd.GraphedTrainStep(m, crit, opt, x, y, warmup=2)
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


# ---- EnhancedCustomLoss, refusals -----------------------------------------------
def test_enhanced_custom_loss_ssim(device):
    import nsm_amd
    o, t = D.inputs((2, 1, 40, 90))
    td = t.to(device)
    od = o.to(device).requires_grad_(True)
    crit = nsm_amd.EnhancedCustomLoss(device, 0.9, vgg_weights=False, ssim_weight=0.1).eval()
    total, losses = crit(None, od, td, None)
    assert set(losses) == {"l1_loss", "vgg_loss", "perturbation_loss", "total_loss", "ssim_loss"}
    term = losses["ssim_loss"]
    assert term.device == od.device and term.dim() == 0 and not term.requires_grad
    # the kernel rounds 1 - ssim from double once; 1 - float32(ssim) rounds twice
    s = nsm_amd.ssim(od.detach(), td)
    assert abs(term.item() - (1 - s.item())) <= 2.0 ** -23
    ref = 0.9 * losses["l1_loss"].detach().cpu() + 0.1 * term.cpu()
    torch.testing.assert_close(total.detach().cpu(), ref, **ELEM)
    total.backward()
    od2 = o.to(device).requires_grad_(True)
    _crit(device)(od2, td, None).backward()
    torch.testing.assert_close(od.grad, od2.grad, **ELEM)
    _, plain = nsm_amd.EnhancedCustomLoss(device, 0.9, vgg_weights=False).eval()(None, od, td, None)
    assert set(plain) == {"l1_loss", "vgg_loss", "perturbation_loss", "total_loss"}


def test_refusals(device):
    import nsm_amd
    crit = _crit(device)
    o3 = torch.rand(2, 3, 16, 16, device=device, requires_grad=True)
    ok = torch.rand(2, 1, 16, 16, device=device)
    low = torch.rand(2, 1, 10, 16, device=device)
    for o, t in ((o3, o3.detach()), (low, low), (low.transpose(2, 3), low.transpose(2, 3)),
                 (ok, ok[:, :, :12]), (ok, o3.detach())):
        with pytest.raises(ValueError):
            nsm_amd.ssim(o, t)
        with pytest.raises(ValueError):
            nsm_amd.ssim_loss(o, t)
        with pytest.raises(ValueError):
            crit(o, t, None)
    with pytest.raises((ValueError, nsm_amd.NsmError)):
        nsm_amd.ssim(ok.cpu(), ok.cpu())
    with pytest.raises((ValueError, nsm_amd.NsmError)):
        nsm_amd.ssim_loss(ok.cpu(), ok.cpu())
    with pytest.raises(ValueError):
        nsm_amd.ssim(ok, ok, data_range=0.0)
    # the default mode still takes any shape
    assert torch.isfinite(nsm_amd.CustomLoss(device, 0.9, vgg_weights=False)(o3, o3.detach(), None))
