"""GPU: the perturbation-loss step. Kernel level: nsm_perturb_variants against
nsm_perturb bit for bit and its device noise as a distribution;
nsm_pert_loss_fwd / nsm_pert_loss_bwd against the fp64 restatement
(tests/perturb_util.py, pinned to the oracle by tests/test_perturb_ref.py).
Model level: EnhancedCustomLoss(fused=True, noise="device") on the reference's
fixture and against the unfused path, and GraphedTrainStep with the criterion
against the same eager steps."""
import ctypes

import numpy as np
import pytest
import torch

import perturb_util as PU
from oracle.weights import make_state
from util import RUN_TOL, load

pytestmark = pytest.mark.gpu
torch.set_num_threads(16)


def _lib():
    from nsm_amd import _lib as L
    return L


def _offset(t):
    """The same values at an address 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _std(x):
    L = _lib()
    B, C, H, W = x.shape
    std = torch.empty(C, dtype=torch.float32, device=x.device)
    L.call("nsm_channel_std", L.ptr(x), B, C, H, W, None, L.ptr(std), L.stream())
    return std


def _variants(x, std, P, noises=None, seed=0, seed_dev=None, factor=0.01, out=None):
    L = _lib()
    B, C, H, W = x.shape
    if out is None:
        out = torch.empty((P, B, C, H, W), dtype=torch.float32, device=x.device)
    L.call("nsm_perturb_variants", L.ptr(x), L.ptr(std), L.ptr(noises), seed, L.ptr(seed_dev), P,
           B, C, H, W, factor, L.ptr(out), L.stream())
    return out


# ---- nsm_perturb_variants ------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3, 8])
@pytest.mark.parametrize("shape", [(2, 7, 5, 7), (1, 4, 1, 1), (2, 7, 8, 16)])
def test_variants_with_injected_noise_are_nsm_perturb(device, shape, P):
    """[2,7,5,7] (HW = 35: ragged tail) and [1,4,1,1] take the scalar path,
    [2,7,8,16] the 16-byte one; moved 4 bytes off alignment it must fall back."""
    L = _lib()
    g = torch.Generator().manual_seed(sum(shape) + P)
    x = (torch.randn(shape, generator=g) * 3 + 0.5).to(device)
    z = torch.randn((P,) + shape, generator=g).to(device)
    B, C, H, W = shape
    std = _std(x) if B * H * W > 1 else torch.rand(C, generator=g).to(device) + 0.5
    want = torch.empty_like(z)
    for i in range(P):
        L.call("nsm_perturb", L.ptr(x), L.ptr(z[i]), L.ptr(std), B, C, H, W, 0.01, L.ptr(want[i]),
               L.stream())
    assert torch.equal(_variants(x, std, P, noises=z), want)
    assert not torch.equal(want[0], x)
    # x, the noise and the output each off alignment in turn, then all three
    xo, zo, oo = _offset(x), _offset(z), _offset(torch.zeros_like(z))
    assert torch.equal(_variants(xo, std, P, noises=z), want)
    assert torch.equal(_variants(x, std, P, noises=zo), want)
    assert torch.equal(_variants(x, std, P, noises=z, out=oo), want)
    oo.zero_()
    assert torch.equal(_variants(xo, std, P, noises=zo, out=oo), want)


def test_variants_device_noise(device):
    shape, P = (2, 4, 64, 64), 3
    g = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=g).to(device)
    std = _std(x)
    a = _variants(x, std, P, seed=1234)
    assert torch.equal(a, _variants(x, std, P, seed=1234))            # the same seed: the same bits
    b = _variants(x, std, P, seed=1235)
    assert (a != b).float().mean().item() > 0.99                      # another seed: other values
    two = _variants(x, std, 2, seed=1234)                             # a variant does not depend on P
    assert torch.equal(two[0], a[0]) and torch.equal(two[1], a[1])
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2])
    sd = torch.tensor([1234], dtype=torch.int64, device=device)
    assert torch.equal(_variants(x, std, P, seed=99, seed_dev=sd), a)  # the device word wins
    assert torch.equal(_variants(_offset(x), std, P, seed=1234), a)    # nor on the access width
    # the recovered normals: 4 sigma of the estimators of mean and variance
    s = (std.double().cpu() * 0.01).view(1, 1, 4, 1, 1)
    zr = ((a.double().cpu() - x.double().cpu()) / s).numpy().ravel()
    N = zr.size
    assert N == 98304
    print(f"device noise: mean {zr.mean():.3e} var {zr.var():.6f} max|z| {np.abs(zr).max():.3f}")
    assert abs(zr.mean()) <= 4 / np.sqrt(N)
    assert abs(zr.var() - 1) <= 4 * np.sqrt(2 / N)
    assert np.abs(zr).max() < 6


# ---- nsm_pert_loss_fwd / bwd -----------------------------------------------------------
LENGTHS = [1, 1000, 8 * 64 * 64, 8 * 64 * 64 + 3]    # one element; one block, 16-byte path;
                                                    # 16 blocks; 17 blocks, ragged, scalar path


def _dev(arrs, device):
    return [torch.from_numpy(a).to(device) for a in arrs]


def _table(ps):
    return (ctypes.c_void_p * len(ps))(*[p.data_ptr() for p in ps])


@pytest.mark.parametrize("P", [1, 3, 8])
@pytest.mark.parametrize("n", LENGTHS)
def test_pert_loss_forward(device, n, P):
    L = _lib()
    alpha, w = 0.9, 0.5
    o, t, ps = PU.make_operands(n, P)
    od, td, *pd = _dev([o, t] + ps, device)
    nb = L.lib.nsm_pert_loss_blocks(n)
    assert nb == -(-n // 2048)
    bound = PU.fwd_bound(n)
    for vgg in (None, 0.4321):
        partial = torch.full(((1 + P) * nb,), float("nan"), device=device)
        rec = torch.full((3 + P,), float("nan"), device=device)
        vd = None if vgg is None else torch.tensor(vgg, dtype=torch.float32, device=device)
        L.call("nsm_pert_loss_fwd", L.ptr(od), L.ptr(td), _table(pd), P, n, alpha, w, L.ptr(vd),
               L.ptr(partial), L.ptr(rec), L.stream())
        got = rec.cpu().double().numpy()
        ref = PU.pert_loss_ref(o, t, ps, alpha, w,
                               vgg=0.0 if vgg is None else float(np.float32(vgg)))
        want = np.array([ref["l1"], ref["pert"], ref["total"]] + ref["means"])
        rel = np.abs(got - want) / want
        print(f"n={n} P={P} vgg={vgg}: max rel {rel.max():.3e} bound {bound:.3e}")
        assert np.isfinite(got).all()
        assert (np.abs(got - want) <= bound * want).all(), (got, want)


@pytest.mark.parametrize("P", [1, 3, 8])
@pytest.mark.parametrize("n", LENGTHS)
def test_pert_loss_backward(device, n, P):
    L = _lib()
    alpha, w = 0.9, 0.5
    o, t, ps = PU.make_operands(n, P)
    od, td, *pd = _dev([o, t] + ps, device)
    tab = _table(pd)
    zero = PU.all_tie(n)

    def run(gscale, grad, accumulate):
        gd = None if gscale is None else torch.tensor(gscale, dtype=torch.float32, device=device)
        L.call("nsm_pert_loss_bwd", L.ptr(od), L.ptr(td), tab, P, n, alpha, w, L.ptr(gd),
               L.ptr(grad), accumulate, L.stream())
        return grad.cpu().double().numpy()

    for gs in (None, 65536.0, -0.75):
        g = 1.0 if gs is None else gs
        got = run(gs, torch.full((n,), float("nan"), device=device), 0)
        ref = PU.pert_grad_ref(o, t, ps, alpha, w, g)
        err = np.abs(got - ref).max()
        bound = PU.grad_bound(n, P, alpha, w, g)
        print(f"n={n} P={P} gscale={gs}: max err {err:.3e} bound {bound:.3e}")
        assert err <= bound                      # every element
        assert (got[zero] == 0).all()            # all signs 0: exactly 0
        assert np.abs(got).max() > 0
    # accumulate = 1 adds onto what the buffer holds (one more rounding, of the sum)
    pre = np.random.default_rng(n + P).standard_normal(n).astype(np.float32) * np.float32(1e-4)
    got = run(None, torch.from_numpy(pre).to(device), 1)
    ref = pre.astype(np.float64) + PU.pert_grad_ref(o, t, ps, alpha, w)
    assert (np.abs(got - ref) <= PU.grad_bound(n, P, alpha, w) + PU.U * np.abs(ref)).all()
    assert (got[zero] == pre[zero]).all()
    # and the offset buffers (scalar path) give the bits of the aligned ones
    base = run(None, torch.empty(n, device=device), 0)
    od2, td2 = _offset(od), _offset(td)
    pd2 = [_offset(p) for p in pd]
    g2 = _offset(torch.empty(n, device=device))
    L.call("nsm_pert_loss_bwd", L.ptr(od2), L.ptr(td2), _table(pd2), P, n, alpha, w, None,
           L.ptr(g2), 0, L.stream())
    assert np.array_equal(g2.cpu().double().numpy(), base)


# ---- EnhancedCustomLoss(fused=True, noise="device") ---------------------------------------
def _build(device, fx):
    from nsm_amd import Unet
    m = Unet(in_ch=4, dropout_rate=0.0)
    sd = {k: torch.from_numpy(v.copy()) for k, v in make_state(4, int(fx["meta/seed_w"])).items()}
    sd.update({k[len("run_before/"):]: torch.from_numpy(v.copy()) for k, v in fx.items()
               if k.startswith("run_before/") and "running" in k})
    m.load_state_dict(sd)
    return m.to(device).train()


def _running(fx):
    return {k[4:]: v for k, v in fx.items() if k.startswith("run/") and "running" in k}


def test_enhanced_custom_loss_fused_on_the_fixture(device):
    """The assertions of test_gpu_model.py::test_enhanced_custom_loss (its
    tolerances and its >= 0.99 agreement share) on the fused, device-noise path
    with the fixture's noises injected, then fused against unfused."""
    import nsm_amd
    from oracle import vgg_ref as V
    fx = load("perturb_c4_b1_64")
    x = torch.from_numpy(fx["x"]).to(device)
    y = torch.rand(fx["out"].shape, generator=torch.Generator().manual_seed(4)).to(device)
    noises = [torch.from_numpy(n).to(device) for n in fx["noise"]]

    def run(fused, noise, inject):
        m = _build(device, fx)
        out = torch.from_numpy(fx["out"]).to(device).requires_grad_(True)
        crit = nsm_amd.EnhancedCustomLoss(device, alpha=0.9, perturb_weight=0.5,
                                          vgg_weights=V.standin_state(), fused=fused, noise=noise)
        if inject == "set":
            crit.set_noises(torch.stack(noises))
            total, parts = crit(m, out, y, x)
        else:
            total, parts = crit(m, out, y, x, noises=noises)
        total.backward()
        return m, crit, out, total, parts

    m, crit, out, total, parts = run(True, "device", "arg")
    l1 = (torch.from_numpy(fx["out"]) - y.cpu()).abs().mean().item()
    vgg = V.vgg_loss(V.standin_state(), torch.from_numpy(fx["out"]), y.cpu()).item()
    pert = float(fx["loss"])
    assert abs(parts["l1_loss"].item() - l1) <= 1e-6 * l1
    assert abs(parts["vgg_loss"].item() - vgg) <= 2e-5 * vgg
    assert abs(parts["perturbation_loss"].item() - pert) <= 2e-5 + 1e-2 * pert
    assert abs(total.item() - (0.9 * l1 + 0.1 * vgg + 0.5 * parts["perturbation_loss"].item())) <= 1e-5
    assert parts["total_loss"] is total
    for k in ("l1_loss", "vgg_loss", "perturbation_loss"):
        assert parts[k].is_cuda and parts[k].dim() == 0 and not parts[k].requires_grad
    ref_g = 0.9 * np.sign(fx["out"] - y.cpu().numpy()) / out.numel() + 0.5 * fx["out_grad"]
    agree = np.mean(np.abs(out.grad.cpu().numpy() - ref_g) <= 1e-9 + 1e-5 * np.abs(ref_g))
    assert agree >= 0.99
    sd = m.state_dict()
    for k, v in _running(fx).items():
        assert np.abs(sd[k].cpu().numpy() - v).max() <= RUN_TOL * (1 + np.abs(v).max()), k
    crit.eval()   # no perturbation term outside training: today's path
    total_e, parts_e = crit(m, out.detach(), y, x)
    assert parts_e["perturbation_loss"].item() == 0.0

    # against fused=False on the same inputs (and the noises set once, as one tensor)
    m0, _, out0, total0, parts0 = run(False, "torch", "arg")
    m1, _, out1, total1, parts1 = run(True, "device", "set")
    assert torch.equal(out1.grad, out.grad) and total1.item() == total.item()
    for k in ("l1_loss", "vgg_loss", "perturbation_loss", "total_loss"):
        a, b = parts[k].item(), parts0[k].item()
        print(f"{k}: fused {a!r} unfused {b!r}")
        assert abs(a - b) <= 2e-6 * abs(b), k
    gerr = (out.grad.double() - out0.grad.double()).abs().max().item()
    print(f"gradient fused vs unfused: max err {gerr:.3e}")
    assert gerr <= PU.grad_bound(out.numel(), 3, 0.9, 0.5)
    for (k, a), (_, b) in zip(m.state_dict().items(), m0.state_dict().items()):
        assert torch.equal(a, b), k        # the same perturbed inputs: the same running statistics


# ---- GraphedTrainStep with the perturbation criterion -------------------------------------
def _setup(device, dtype=torch.float32, B=2, C=4, H=64, seed=3, lr=1e-3, wd=1e-3, scaler=None,
           **crit_kw):
    import nsm_amd
    torch.manual_seed(seed)
    m = nsm_amd.Unet(in_ch=C, dropout_rate=0.0).to(device).train()
    if dtype != torch.float32:
        m.set_compute_dtype(dtype)
    opt = nsm_amd.FlatAdamW(m.parameters(), lr=lr, weight_decay=wd, max_grad_norm=1.0,
                            sanitize=True, seed=11, grad_scaler=scaler)
    crit = nsm_amd.EnhancedCustomLoss(device, 0.9, perturb_weight=0.5, vgg_weights=False, **crit_kw)
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(B, C, H, H, device=device, generator=g)
    y = torch.rand(B, 1, H, H, device=device, generator=g)
    z = torch.randn(3, B, C, H, H, device=device, generator=g)
    return m, opt, crit, x, y, z


def _state(m, opt):
    return [t.detach().clone() for t in [opt.flat, opt.exp_avg, opt.exp_avg_sq]
            + list(m.buffers())]


KEYS = {"l1_loss", "vgg_loss", "perturbation_loss", "total_loss"}


@pytest.mark.parametrize("fused,noise", [(False, "torch"), (True, "device")])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graphed_perturbation_step_equals_eager_steps(device, dtype, fused, noise):
    """As test_gpu_graph_step.py::test_graphed_step_equals_eager_steps: three
    replays equal three eager steps bitwise (parameters, AdamW moments, BN
    buffers), with the noises injected into both."""
    import nsm_amd
    m, opt, crit, x, y, z = _setup(device, dtype, fused=fused, noise=noise)
    m2, opt2, crit2, _, _, _ = _setup(device, dtype, fused=fused, noise=noise)
    crit.set_noises(z)
    crit2.set_noises(z)
    before = _state(m, opt)
    step = nsm_amd.GraphedTrainStep(m, crit, opt, x, y, warmup=2)
    for a, b in zip(before, _state(m, opt)):
        assert torch.equal(a, b)
    got, ref = [], []
    for _ in range(3):
        total = step()
        assert set(step.losses) == KEYS
        assert step.losses["total_loss"].item() == total.item()
        got.append({k: v.item() for k, v in step.losses.items()})
    for _ in range(3):
        total, parts = crit2(m2, m2(x), y, x)
        total.backward()
        opt2.step()
        opt2.zero_grad()
        ref.append({k: v.item() for k, v in parts.items()})
    assert got == ref, (got, ref)
    assert got[0]["perturbation_loss"] > 0 and got[0] != got[1]
    for a, b in zip(_state(m, opt), _state(m2, opt2)):
        assert torch.equal(a, b)


def test_graphed_perturbation_step_draws_new_noise_every_replay(device):
    """noise="device", nothing injected, lr = 0: the parameters stay put, so two
    replays on one batch give the same L1 term bit for bit and another
    perturbation term: new noise without a new capture."""
    import nsm_amd
    m, opt, crit, x, y, _ = _setup(device, lr=0.0, wd=0.0, fused=True, noise="device")
    step = nsm_amd.GraphedTrainStep(m, crit, opt, x, y, warmup=1)
    graph = step.graph
    seen = []
    for _ in range(3):
        step()
        seen.append({k: v.item() for k, v in step.losses.items()})
    assert step.graph is graph
    assert seen[0]["l1_loss"] == seen[1]["l1_loss"] == seen[2]["l1_loss"]
    assert len({s["perturbation_loss"] for s in seen}) == 3, seen
    crit.check_range_now()   # sigmoid output: in range, nothing raised


def test_graphed_perturbation_step_with_a_grad_scaler(device):
    """The scaler's scale word seeds the fused backward (gscale) inside the
    graph: the replays equal eager steps seeded the same way."""
    import nsm_amd
    sc = [nsm_amd.GradScaler(init_scale=1024.0, growth_interval=2, device=device)
          for _ in range(2)]
    m, opt, crit, x, y, z = _setup(device, scaler=sc[0], fused=True, noise="device")
    m2, opt2, crit2, _, _, _ = _setup(device, scaler=sc[1], fused=True, noise="device")
    crit.set_noises(z)
    crit2.set_noises(z)
    step = nsm_amd.GraphedTrainStep(m, crit, opt, x, y, warmup=1)
    for _ in range(3):
        step()
        total, _ = crit2(m2, m2(x), y, x)
        total.backward(sc[1].seed)
        opt2.step()
        opt2.zero_grad()
    assert sc[0].last() == sc[1].last() and sc[0].last()["growths"] >= 1
    for a, b in zip(_state(m, opt), _state(m2, opt2)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reuse_prepared_weights_is_bitwise_and_follows_the_weights(device, dtype):
    """A forward that keeps the prepared weight layouts (what the fused
    criterion's perturbed forwards do) equals one that prepares them, output,
    BN buffers and gradients; after an in-place weight change it prepares again."""
    from nsm_amd.unet import reuse_prepared_weights
    m, _, _, x, y, _ = _setup(device, dtype)
    m2, _, _, _, _, _ = _setup(device, dtype)

    def twice(mod, reuse):
        mod(x)
        if reuse:
            with reuse_prepared_weights(mod):
                out = mod(x)
        else:
            out = mod(x)
        (out * y).sum().backward()
        return out.detach()

    for _ in range(2):
        assert torch.equal(twice(m, False), twice(m2, True))
        for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
            assert torch.equal(a, b), k
        for (k, a), (_, b) in zip(m.named_parameters(), m2.named_parameters()):
            assert torch.equal(a.grad, b.grad), k
        with torch.no_grad():   # the version counters move: the kept layouts are stale
            for mod in (m, m2):
                mod.conv6.conv[0].weight.mul_(1.25)
                mod.conv9.conv[4].weight.add_(0.01)
        with reuse_prepared_weights(m2):
            stale = m2(x).detach()
        assert torch.equal(stale, m(x).detach())


def test_eager_device_noise_follows_torch_manual_seed(device):
    """Eager: the kernel's seed is drawn from torch's CPU generator."""
    import nsm_amd
    pl = nsm_amd.PerturbationLoss(noise="device")
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(1)).to(device)
    torch.manual_seed(7)
    a = torch.stack(pl.perturb_input(x))
    b = torch.stack(pl.perturb_input(x))
    torch.manual_seed(7)
    c = torch.stack(pl.perturb_input(x))
    assert torch.equal(a, c) and not torch.equal(a, b)
    own = [nsm_amd.PerturbationLoss(noise="device", seed=5) for _ in range(2)]
    assert torch.equal(torch.stack(own[0].perturb_input(x)), torch.stack(own[1].perturb_input(x)))
    assert a.shape == (3, 2, 4, 16, 16)
