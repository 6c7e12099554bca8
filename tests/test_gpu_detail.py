"""GPU: the opt-in detail terms of CustomLoss (detail_weight, gradient_weight):
nsm_detail_loss_fwd/bwd against the float64 restatement of the reference's
formulas (detail_util.py), and the interface: CustomLoss with and without the
VGG gradient, seed scaling, determinism, the untouched default mode, through
the U-Net, inside GraphedTrainStep, EnhancedCustomLoss and the refusals."""
import pytest
import torch

import detail_util as U
from oracle.weights import make_state
from util import load

pytestmark = pytest.mark.gpu
torch.set_num_threads(16)

IDS = dict(ids=lambda s: "x".join(map(str, s)))
WEIGHTS = {"hf": (1.0, 0.0, 0.0), "pen": (0.0, 1.0, 0.0), "sob": (0.0, 0.0, 1.0)}
ELEM = dict(rtol=1e-6, atol=0)


def term_grad(device, o, t, w, seed=None):
    import nsm_amd
    od = o.to(device).requires_grad_(True)
    loss = nsm_amd.detail_loss(od, t.to(device), *w)
    loss.backward(seed)
    return loss.detach(), od.grad


# ---- kernels ----------------------------------------------------------------
@pytest.mark.parametrize("shape", U.SHAPES, **IDS)
def test_values(device, shape):
    import nsm_amd
    o, t, vals, _, _ = U.reference(shape)
    got = [v.item() for v in nsm_amd.detail_terms(o.to(device), t.to(device))]
    for k, g in zip(U.TERMS, got):
        err = abs(g - vals[k]) / abs(vals[k])
        print(f"{shape} {k}: {g:.9e} ref {vals[k]:.9e} rel {err:.2e}")
    for k, g in zip(U.TERMS, got):
        assert abs(g - vals[k]) <= U.VALUE_REL * abs(vals[k]), k


@pytest.mark.parametrize("term", U.TERMS)
@pytest.mark.parametrize("shape", U.SHAPES, **IDS)
def test_gradients(device, shape, term):
    """Each term alone (the other weights 0), outside the float64 near ties."""
    o, t, vals, grads, ties = U.reference(shape)
    loss, grad = term_grad(device, o, t, WEIGHTS[term])
    rel, worst, share = U.grad_errors(grad.cpu(), grads[term], ties[term])
    print(f"{shape} {term}: rel-L2 {rel:.2e} pixel {worst:.2e} excluded {share:.2e}")
    assert share <= U.TIE_SHARE
    assert grads[term].abs().max() > 0
    assert rel <= U.GRAD_REL_L2 and worst <= U.GRAD_PIXEL
    assert abs(loss.item() - vals[term]) <= U.VALUE_REL * abs(vals[term])


def test_no_penumbra(device):
    """t in {0, 1}: the mask is empty, PEN and its gradient are exactly 0. The
    flat regions make sign(r) rounding noise (in the reference too): values and
    finiteness only."""
    import nsm_amd
    o, _ = U.inputs((2, 1, 33, 65))
    t = (U.inputs((2, 1, 33, 65), seed=1)[1] > 0.5).float()
    hf, pen, sob = nsm_amd.detail_terms(o.to(device), t.to(device))
    assert pen.item() == 0.0
    ref = U.terms(o.double(), t.double())
    assert abs(hf.item() - ref["hf"].item()) <= U.VALUE_REL * ref["hf"].item()
    assert abs(sob.item() - ref["sob"].item()) <= U.VALUE_REL * ref["sob"].item()
    _, g = term_grad(device, o, t, WEIGHTS["pen"])
    assert (g == 0).all()
    loss, g = term_grad(device, o, t, (0.1, 0.1, 0.1))
    assert torch.isfinite(loss) and torch.isfinite(g).all() and g.abs().max() > 0
    # a flat pair: every r is 0, sign(0) = 0
    flat = torch.full((2, 1, 20, 70), 0.5)
    loss, g = term_grad(device, flat, flat.clone(), (1.0, 1.0, 1.0))
    assert loss.item() == 0.0 and (g == 0).all()


# ---- CustomLoss --------------------------------------------------------------
def _pieces(device, o, t, dw, gw):
    """alpha*sign/N and the three weighted term gradients, each from its own
    kernel call, summed in the kernel's order."""
    import nsm_amd
    od = o.to(device).requires_grad_(True)
    nsm_amd.l1_loss(od, t.to(device), 0.9).backward()
    parts = [term_grad(device, o, t, w)[1].cpu()
             for w in ((dw, 0.0, 0.0), (0.0, dw, 0.0), (0.0, 0.0, gw))]
    for p in parts:
        assert p.abs().max() > 0
    return od.grad.cpu(), (parts[0] + parts[1]) + parts[2]


def test_custom_loss_detail(device):
    import nsm_amd
    o, t = U.inputs((2, 1, 40, 72))
    od, td = o.to(device).requires_grad_(True), t.to(device)
    crit = nsm_amd.CustomLoss(device, 0.9, vgg_weights=False, detail_weight=0.1,
                              gradient_weight=0.1)
    loss = crit(od, td, None)
    loss.backward()
    base = nsm_amd.CustomLoss(device, 0.9, vgg_weights=False)(od.detach(), td, None).cpu()
    hf, pen, sob = [v.cpu() for v in nsm_amd.detail_terms(od.detach(), td)]
    torch.testing.assert_close(loss.detach().cpu(), base + 0.1 * (hf + pen) + 0.1 * sob, **ELEM)
    l1, detail = _pieces(device, o, t, 0.1, 0.1)
    torch.testing.assert_close(od.grad.cpu(), l1 + detail, **ELEM)
    # the detail part is not noise beside alpha/N
    assert detail.abs().max() > 1e-2 * l1.abs().max()


def test_custom_loss_detail_with_vgg_grad(device):
    import nsm_amd
    o, t = U.inputs((2, 1, 32, 48))
    td = t.to(device)
    vgg = nsm_amd.CustomLoss(device, 0.9, vgg_weights="random").vgg_loss
    od = o.to(device).requires_grad_(True)
    crit = nsm_amd.CustomLoss(device, 0.9, vgg_weights=vgg, vgg_grad=True, detail_weight=0.1,
                              gradient_weight=0.1)
    loss = crit(od, td, None)
    loss.backward()
    o2 = o.to(device).requires_grad_(True)
    base = nsm_amd.CustomLoss(device, 0.9, vgg_weights=vgg, vgg_grad=True)(o2, td, None)
    base.backward()
    hf, pen, sob = [v.cpu() for v in nsm_amd.detail_terms(o2.detach(), td)]
    torch.testing.assert_close(loss.detach().cpu(),
                               base.detach().cpu() + 0.1 * (hf + pen) + 0.1 * sob, **ELEM)
    l1, detail = _pieces(device, o, t, 0.1, 0.1)
    torch.testing.assert_close(od.grad.cpu(), o2.grad.cpu() + detail, **ELEM)
    assert not torch.equal(o2.grad.cpu(), l1)          # the VGG chain contributed
    # the detached default composes too: the value moves, the gradient is L1 + detail
    o3 = o.to(device).requires_grad_(True)
    det = nsm_amd.CustomLoss(device, 0.9, vgg_weights=vgg, detail_weight=0.1, gradient_weight=0.1)
    l3 = det(o3, td, None)
    l3.backward()
    torch.testing.assert_close(l3.detach(), loss.detach(), **ELEM)
    torch.testing.assert_close(o3.grad.cpu(), l1 + detail, **ELEM)


def test_seed_scaling_is_exact(device):
    import nsm_amd
    o, t = U.inputs((3, 1, 33, 65))
    grads = []
    for seed in (None, torch.tensor(1024.0, device=device)):
        od = o.to(device).requires_grad_(True)
        crit = nsm_amd.CustomLoss(device, 0.9, vgg_weights=False, detail_weight=0.1,
                                  gradient_weight=0.1)
        crit(od, t.to(device), None).backward(seed)
        grads.append(od.grad)
    assert grads[0].abs().max() > 0
    assert torch.equal(grads[1], 1024.0 * grads[0])
    assert torch.equal(term_grad(device, o, t, (0.1, 0.1, 0.1), torch.tensor(1024.0, device=device))[1],
                       1024.0 * term_grad(device, o, t, (0.1, 0.1, 0.1))[1])


def test_determinism(device):
    import nsm_amd
    o, t = U.inputs((3, 1, 33, 65))
    runs = []
    for _ in range(2):
        od = o.to(device).requires_grad_(True)
        crit = nsm_amd.CustomLoss(device, 0.9, vgg_weights=False, detail_weight=0.1,
                                  gradient_weight=0.1)
        loss = crit(od, t.to(device), None)
        loss.backward()
        runs.append((loss.detach(), od.grad) + tuple(nsm_amd.detail_terms(od.detach(), t.to(device))))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_default_mode_is_untouched(device):
    import nsm_amd
    o, t = U.inputs((2, 1, 40, 72))
    res = []
    for kw in ({}, dict(detail_weight=0, gradient_weight=0)):
        od = o.to(device).requires_grad_(True)
        loss = nsm_amd.CustomLoss(device, 0.9, vgg_weights=False, **kw)(od, t.to(device), None)
        loss.backward()
        res.append((loss.detach(), od.grad, type(loss.grad_fn).__name__))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2] == "_L1FnBackward"
    ref = 0.9 * torch.sign(o - t) / o.numel()
    torch.testing.assert_close(res[1][1].cpu(), ref, **ELEM)


# ---- in the training step ------------------------------------------------------
def _crit(device):
    import nsm_amd
    return nsm_amd.CustomLoss(device, 0.9, vgg_weights=False, detail_weight=0.1,
                              gradient_weight=0.1)


def test_detail_through_unet(device):
    import nsm_amd
    fx = load("train_c7_p0_b2_64")
    in_ch = int(fx["meta/in_ch"])
    m = nsm_amd.Unet(in_ch=in_ch, dropout_rate=0.0)
    m.load_state_dict({k: torch.from_numpy(v.copy())
                       for k, v in make_state(in_ch, int(fx["meta/seed_w"])).items()})
    m = m.to(device).train()
    crit = _crit(device)
    x, y = torch.from_numpy(fx["x"]).to(device), torch.from_numpy(fx["y"]).to(device)
    out = m(x)
    out.retain_grad()
    crit(out, y, x).backward()
    leaf = out.detach().clone().requires_grad_(True)
    crit(leaf, y, None).backward()
    assert torch.equal(out.grad, leaf.grad)
    l1 = 0.9 * torch.sign(out.detach() - y) / out.numel()
    assert not torch.equal(out.grad, l1)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


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


def test_graphed_step_with_detail_equals_eager_steps(device):
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
def test_enhanced_custom_loss_detail(device):
    import nsm_amd
    o, t = U.inputs((2, 1, 40, 72))
    td = t.to(device)
    od = o.to(device).requires_grad_(True)
    crit = nsm_amd.EnhancedCustomLoss(device, 0.9, vgg_weights=False, detail_weight=0.1,
                                      gradient_weight=0.2).eval()
    total, losses = crit(None, od, td, None)
    assert set(losses) == {"l1_loss", "vgg_loss", "perturbation_loss", "total_loss",
                           "high_freq_loss", "penumbra_loss", "gradient_loss"}
    hf, pen, sob = nsm_amd.detail_terms(od.detach(), td)
    for k, v in (("high_freq_loss", hf), ("penumbra_loss", pen), ("gradient_loss", sob)):
        assert losses[k].device == od.device and losses[k].dim() == 0
        assert not losses[k].requires_grad
        assert torch.equal(losses[k], v)
    ref = 0.9 * losses["l1_loss"].detach().cpu() + 0.1 * (hf.cpu() + pen.cpu()) + 0.2 * sob.cpu()
    torch.testing.assert_close(total.detach().cpu(), ref, **ELEM)
    assert losses["total_loss"] is total
    total.backward()
    od2 = o.to(device).requires_grad_(True)
    nsm_amd.CustomLoss(device, 0.9, vgg_weights=False, detail_weight=0.1,
                       gradient_weight=0.2)(od2, td, None).backward()
    torch.testing.assert_close(od.grad, od2.grad, **ELEM)
    _, plain = nsm_amd.EnhancedCustomLoss(device, 0.9, vgg_weights=False).eval()(None, od, td, None)
    assert set(plain) == {"l1_loss", "vgg_loss", "perturbation_loss", "total_loss"}


def test_refusals(device):
    import nsm_amd
    o = torch.rand(2, 3, 8, 8, device=device, requires_grad=True)
    t = torch.rand(2, 3, 8, 8, device=device)
    with pytest.raises(ValueError):
        nsm_amd.CustomLoss(device, 0.9, vgg_weights=False, detail_weight=0.1)(o, t, None)
    with pytest.raises(ValueError):
        nsm_amd.CustomLoss(device, 0.9, vgg_weights=False, gradient_weight=0.1)(o, t, None)
    with pytest.raises(ValueError):
        nsm_amd.detail_terms(o, t)
    with pytest.raises(ValueError):
        nsm_amd.detail_terms(o[:, :1], t[:, :1, :4])
    # the default mode still takes any shape
    assert torch.isfinite(nsm_amd.CustomLoss(device, 0.9, vgg_weights=False)(o, t, None))
