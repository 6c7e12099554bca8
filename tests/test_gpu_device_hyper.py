"""GPU: lr and max_norm as device words (`device_hyper=True`, include/nsm.h
nsm_hyper_set and the *_dev tail entries).

The two paths differ only in where a value is read from (a kernel argument, or
the 16-byte hyper block), so every comparison here is bitwise and no tolerance
appears: the device-hyper tail, eager and replayed from ONE capture across a
schedule, against the argument-path tail; through nsm_amd.GradScaler; queued
with no host wait between uploads and replays; and under GraphedTrainStep, which
must not re-capture for an lr / max_norm change."""
import functools

import numpy as np
import pytest
import torch

from test_tail import tail_fixture

pytestmark = pytest.mark.gpu

# kind -> (flat class name, optimizer keywords)
KINDS = {
    "adamw": ("FlatAdamW", {}),
    "adam": ("FlatAdam", {}),
    "sgd": ("FlatSGD", {"momentum": 0.9}),
    "sgd0": ("FlatSGD", {"momentum": 0.0}),
}


def _snap(opt, extra=()):
    """Everything the tail and the update kernel write (and `extra`), as host
    arrays: parameters, moments, the step counters, the 8 flags, stat."""
    torch.cuda.synchronize()
    ts = [opt.flat] + opt._moments() + [opt._step_dev, opt.flags, opt.stat] + list(extra)
    return [t.detach().cpu().numpy().copy() for t in ts]


def _same(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        # the bytes, so that equal NaNs are equal and -0.0 is not 0.0
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


def _capture(opt, noise=None):
    """ONE capture of the tail (recorded, not run). The hyper block is made
    current first; inside the capture step() uploads nothing."""
    opt.sync_hyper()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step(noise=noise)
    return graph


# ---- 1. the reference's scripted run: 12 steps, 4 epochs, one capture ---------------------
@functools.lru_cache(maxsize=None)
def _fixture():
    return tail_fixture()


def _scripted(device, kind, world, device_hyper, capture):
    import nsm_amd
    from nsm_amd.optim import FLAG_NAMES
    fx, E, P, nparam, steps = _fixture()
    cls, kw = KINDS[kind]
    params = [torch.nn.Parameter(torch.from_numpy(fx[f"init/{i}"].copy()).to(device))
              for i in range(nparam)]
    base = float(fx["meta/base_lr"])
    opt = getattr(nsm_amd, cls)(params, lr=base, weight_decay=float(fx["meta/wd"]),
                                max_grad_norm=1.0, sanitize=True, world_size=world, seed=11,
                                device_hyper=device_hyper, **kw)
    assert len(FLAG_NAMES) == opt.flags.numel()
    gflat = torch.empty(opt.flat.numel(), device=device)
    noise = torch.empty_like(gflat)
    off = 0
    for p in params:
        p.grad = gflat[off:off + p.numel()].view_as(p)
        off += p.numel()
    graph = _capture(opt, noise) if capture else None
    out, norms = [], []
    for b, (epoch, grads, nz) in enumerate(steps):
        gflat.copy_(torch.cat([g.reshape(-1) for g in grads]).to(device) * world)
        noise.copy_(torch.cat([n.reshape(-1) for n in nz]).to(device))
        opt.param_groups[0]["lr"] = base / (1.0 + epoch)
        opt.set_epoch(epoch, E)
        if capture:
            opt.sync_hyper()
            graph.replay()
        else:
            opt.step(noise=noise)
        out.append(_snap(opt))
        norms.append(opt.last_flags()["max_norm"])
    return out, norms, [int(s) for s in fx["skipped"]]


@functools.lru_cache(maxsize=None)
def _scripted_argument_path(kind, world):
    return _scripted(torch.device("cuda", 0), kind, world, False, False)


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("kind", list(KINDS))
def test_scripted_tail_one_capture(device, kind, world):
    """lr = base/(1+epoch) and set_epoch's max_norm (1, 1, 0.5, 0.25) over the
    reference's 12 scripted steps, three of them skipped: the device-hyper tail,
    eager and replayed from one capture with sync_hyper() between replays, is
    the argument-path eager tail on every step, bit for bit (parameters, state,
    step counters, every flag, stat). An argument-path capture would freeze the
    first epoch's values, so this cannot pass without the hyper block."""
    ref, norms, skipped = _scripted_argument_path(kind, world)
    assert norms == [1.0] * 6 + [0.5] * 3 + [0.25] * 3
    assert [int(s[-2][0]) for s in ref] == skipped and sum(skipped) == 3
    for capture in (False, True):
        got, got_norms, _ = _scripted(device, kind, world, True, capture)
        assert got_norms == norms                  # stat[2]: the max_norm read from the block
        for b, (a, r) in enumerate(zip(got, ref)):
            _same(a, r, (kind, world, "replay" if capture else "eager", b))


# ---- 2. / 3. / 4. a ragged block plan ---------------------------------------------------------
SIZES = [5, 8192 + 3, 8192, 1]     # a ragged crossing of TAIL_CHUNK, an exact block, one element
TOTAL = sum(SIZES)
WD = 1e-4
# (lr, max_norm) of each step: lr = 0, no clipping (None), and thresholds below
# the gradient's norm (~0.13), where the clip coefficient is < 1
SCHEDULE = [(1e-2, 1.0), (0.0, 0.5), (3e-3, None), (1e-3, 0.01), (7e-4, 0.1), (2e-2, 1.0)]


def _init():
    g = torch.Generator().manual_seed(0)
    return [torch.randn(n, generator=g) for n in SIZES]


def _clean(seed, amp=1e-3):
    """A flat gradient of norm ~0.13 * amp/1e-3."""
    return torch.randn(TOTAL, generator=torch.Generator().manual_seed(seed)) * amp


def _build(device, kind, **kw):
    import nsm_amd
    cls, okw = KINDS[kind]
    ps = [torch.nn.Parameter(t.clone().to(device)) for t in _init()]
    opt = getattr(nsm_amd, cls)(ps, lr=1e-2, weight_decay=WD, max_grad_norm=1.0, sanitize=True,
                                seed=5, **okw, **kw)
    gflat = torch.zeros(TOTAL, device=device)
    off = 0
    for p in ps:
        p.grad = gflat[off:off + p.numel()].view_as(p)
        off += p.numel()
    return opt, gflat


def _run_schedule(device, kind, device_hyper, capture, scaler=None, grads=None):
    opt, g = _build(device, kind, device_hyper=device_hyper, grad_scaler=scaler)
    extra = [] if scaler is None else [scaler.state_tensor()]
    graph = _capture(opt) if capture else None
    out = []
    for s, (lr, mx) in enumerate(SCHEDULE):
        g.copy_(grads[s] if grads is not None else _clean(50 + s))
        opt.param_groups[0]["lr"] = lr
        opt.max_grad_norm = mx
        if capture:
            opt.sync_hyper()
            graph.replay()
        else:
            opt.step()
        out.append(_snap(opt, extra))
    return out, opt


@pytest.mark.parametrize("kind", list(KINDS))
def test_odd_block_plan_every_step_another_pair(device, kind):
    ref, ropt = _run_schedule(device, kind, False, False)
    clip = [float(s[-1][1]) for s in ref]                  # stat[1], the clip coefficient
    assert clip[2] == 1.0 and clip[3] < 0.1 and clip[4] < 1.0, clip
    assert [float(s[-1][2]) for s in ref] == [float(np.float32(np.inf if m is None else m))
                                              for _, m in SCHEDULE]
    assert ropt.steps_taken() == len(SCHEDULE)
    # lr = 0: AdamW still decays nothing (1 - 0*wd) and moves nothing; the moments advance
    for capture in (False, True):
        got, opt = _run_schedule(device, kind, True, capture)
        for s, (a, r) in enumerate(zip(got, ref)):
            _same(a, r, (kind, capture, s))
        hv = opt.hyper_values()
        assert hv == {"lr": SCHEDULE[-1][0], "max_norm": 1.0}


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_scaled_tail_with_an_overflow_step(device, kind):
    """Through nsm_grad_tail_scaled(_dev): the schedule above at a dynamic loss
    scale, with an Inf in step 2 (skipped; the scale backs off) and a growth
    (interval 2): parameters, state, flags and the scaler's words are bitwise
    those of the argument path."""
    import nsm_amd

    def scaler():
        return nsm_amd.GradScaler(init_scale=1024.0, growth_interval=2, on_overflow="skip",
                                  device=device)

    # the scale every step is taken at: growth after steps 0-1, backoff at step 2, growth after 3-4
    scales = [1024.0, 1024.0, 2048.0, 1024.0, 1024.0, 2048.0]
    grads = []
    for s, sc in enumerate(scales):
        gr = _clean(70 + s) * sc
        if s == 2:
            gr[5 + 4321] = float("inf")
        grads.append(gr)
    sref = scaler()
    ref, ropt = _run_schedule(device, kind, False, False, sref, grads)
    assert [int(s[-3][0]) for s in ref] == [0, 0, 1, 0, 0, 0]          # flags[0]: skip
    assert sref.last() == dict(scale=2048.0, growth_tracker=1, found_inf=0, overflows=1,
                               growths=2)
    for capture in (False, True):
        sc = scaler()
        got, _ = _run_schedule(device, kind, True, capture, sc, grads)
        for s, (a, r) in enumerate(zip(got, ref)):
            _same(a, r, (kind, capture, s))
        assert sc.last() == sref.last()


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_uploads_and_replays_queue_without_a_host_wait(device, kind):
    """set a, replay, set b, replay, set c, set d, replay, with nothing between
    them but the stream's order: every upload carries its own values (they are
    arguments of its launch), so the result is eager steps at a, b and d."""
    a, b, c, d = 1e-2, 3e-3, 0.5, 7e-4
    grad = _clean(90)
    ref, g = _build(device, kind)
    g.copy_(grad)
    for lr in (a, b, d):
        ref.param_groups[0]["lr"] = lr
        ref.step()
    want = _snap(ref)
    opt, g = _build(device, kind, device_hyper=True)
    g.copy_(grad)
    graph = _capture(opt)
    torch.cuda.synchronize()
    for lrs in ((a,), (b,), (c, d)):
        for lr in lrs:
            opt.param_groups[0]["lr"] = lr
            opt.sync_hyper()
        graph.replay()
    _same(_snap(opt), want, kind)
    assert opt.hyper_values()["lr"] == d


def test_nothing_is_uploaded_under_capture(device):
    """The capture rule: with a changed lr pending, step() on a capturing stream
    records no upload and sync_hyper() raises, so the block keeps the old value
    until the next sync_hyper() outside the capture; the replay then steps at
    the new one."""
    a, b = 1e-2, 5e-3
    grad = _clean(91)
    ref, g = _build(device, "adamw")
    g.copy_(grad)
    ref.param_groups[0]["lr"] = b
    ref.step()
    opt, g = _build(device, "adamw", device_hyper=True)
    g.copy_(grad)
    opt.sync_hyper()
    opt.param_groups[0]["lr"] = b
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="capturing"):
            opt.sync_hyper()
        opt.step()
    assert opt.hyper_values()["lr"] == a and opt.steps_taken() == 0
    opt.sync_hyper()
    graph.replay()
    assert opt.hyper_values()["lr"] == b
    _same(_snap(opt), _snap(ref), "replay after the upload")


# ---- 5. GraphedTrainStep ------------------------------------------------------------------------
def _setup(device, device_hyper, perturb=False, B=2, C=7, H=64, seed=3):
    import nsm_amd
    torch.manual_seed(seed)
    m = nsm_amd.Unet(in_ch=C, dropout_rate=0.0).to(device).train()
    opt = nsm_amd.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-3, max_grad_norm=1.0,
                            sanitize=True, seed=11, device_hyper=device_hyper)
    if perturb:
        crit = nsm_amd.EnhancedCustomLoss(device, 0.9, perturb_weight=0.5, vgg_weights=False,
                                          fused=True, noise="device")
    else:
        crit = nsm_amd.CustomLoss(device, 0.9, vgg_weights=False)
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(B, C, H, H, device=device, generator=g)
    y = torch.rand(B, 1, H, H, device=device, generator=g)
    return m, opt, crit, x, y


def _state(m, opt):
    torch.cuda.synchronize()
    return [t.detach().cpu().numpy().copy()
            for t in [opt.flat, opt.exp_avg, opt.exp_avg_sq] + list(m.buffers())]


def test_graphed_step_follows_a_schedule_on_one_capture(device):
    """Four replays with an lr change, a lower max_norm from set_epoch and a
    LambdaLR step between them: one capture, and parameters, moments and BN
    buffers are those of a twin on the argument path, which re-captures for
    each. A change of betas (still a kernel argument) re-captures both."""
    import nsm_amd
    m, opt, crit, x, y = _setup(device, True)
    m2, opt2, crit2, _, _ = _setup(device, False)
    step = nsm_amd.GraphedTrainStep(m, crit, opt, x, y, warmup=1)
    twin = nsm_amd.GraphedTrainStep(m2, crit2, opt2, x, y, warmup=1)
    scheds = [torch.optim.lr_scheduler.LambdaLR(o, lr_lambda=lambda e: 1.0 / (1.0 + e))
              for o in (opt, opt2)]
    assert step.captures == 1 and twin.captures == 1

    def both(n):
        la, lb = step().item(), twin().item()
        assert la == lb, (n, la, lb)
        _same(_state(m, opt), _state(m2, opt2), n)

    both(1)
    for o in (opt, opt2):
        o.param_groups[0]["lr"] = 3e-4
    both(2)
    assert step.captures == 1 and opt.hyper_values() == {"lr": 3e-4, "max_norm": 1.0}
    for o in (opt, opt2):
        o.set_epoch(9, 10)                      # max_norm 0.1
    both(3)
    assert step.captures == 1
    fl = opt.last_flags()
    print(f"replay 3: total norm {fl['total_norm']:.4g}, clip coefficient {fl['clip_coef']:.4g}")
    assert opt.max_grad_norm == 0.1 and fl["max_norm"] == float(np.float32(0.1))
    for s in scheds:
        s.step()                                # lr = 1e-3 / 2
    assert opt.param_groups[0]["lr"] == 5e-4
    both(4)
    assert step.captures == 1 and twin.captures == 4
    # this model's gradient norm is below the schedule's floor of 0.1: one more
    # replay at a threshold that does clip
    for o in (opt, opt2):
        o.max_grad_norm = 1e-3
    both(5)
    assert step.captures == 1 and twin.captures == 5
    assert opt.last_flags()["clip_coef"] < 1.0
    for o in (opt, opt2):
        o.param_groups[0]["betas"] = (0.8, 0.99)
    both(6)
    assert step.captures == 2 and twin.captures == 6
    assert opt.steps_taken() == 6


def test_graphed_perturbation_step_on_one_capture(device):
    """The perturbation criterion (its perturbed forwards inside the graph): an
    lr change between two replays costs no capture."""
    import nsm_amd
    m, opt, crit, x, y = _setup(device, True, perturb=True)
    step = nsm_amd.GraphedTrainStep(m, crit, opt, x, y, warmup=1)
    l1 = step().item()
    opt.param_groups[0]["lr"] = 2e-4
    l2 = step().item()
    assert step.captures == 1
    assert np.isfinite(l1) and np.isfinite(l2)
    assert all(np.isfinite(v.item()) for v in step.losses.values())
    assert opt.hyper_values()["lr"] == 2e-4 and opt.steps_taken() == 2


# ---- 6. checkpoint ------------------------------------------------------------------------------
def test_checkpoint_lr_reaches_a_live_graphed_step(device):
    """load_state_dict of a torch-format checkpoint that holds another lr, under
    a live GraphedTrainStep: no capture, and the next replay is an eager step at
    that lr. The block holds lr as the double and max_norm as the float."""
    import nsm_amd
    lr2, mx = 2.5e-4, 0.3
    assert float(np.float32(lr2)) != lr2 and float(np.float32(mx)) != mx
    m, opt, crit, x, y = _setup(device, True)
    m2, opt2, crit2, _, _ = _setup(device, False)
    step = nsm_amd.GraphedTrainStep(m, crit, opt, x, y, warmup=1)

    def eager():
        loss = crit2(m2(x), y, x)
        loss.backward()
        opt2.step()
        opt2.zero_grad()

    step()
    eager()
    sd = opt.state_dict()
    sd["param_groups"][0]["lr"] = lr2
    torch.optim.AdamW([torch.nn.Parameter(p.detach().cpu().clone()) for p in m.parameters()]
                      ).load_state_dict(sd)                  # torch's own format
    opt.load_state_dict(sd)
    opt.max_grad_norm = mx
    opt2.param_groups[0]["lr"] = lr2
    opt2.max_grad_norm = mx
    step()
    eager()
    assert step.captures == 1
    _same(_state(m, opt), _state(m2, opt2), "after the checkpoint")
    assert opt.hyper_values() == {"lr": lr2, "max_norm": float(np.float32(mx))}
    assert opt.state_dict()["param_groups"][0]["lr"] == lr2     # the host group is the truth


# ---- 7. refusals ----------------------------------------------------------------------------------
def test_device_hyper_needs_the_device_tail(device):
    import nsm_amd
    for make in (nsm_amd.FlatAdamW, nsm_amd.FlatAdam, nsm_amd.FlatSGD,
                 lambda ps, **kw: nsm_amd.make_optimizer(ps, "adamw", 1e-3, **kw)):
        ps = [torch.nn.Parameter(torch.zeros(4, device=device))]
        with pytest.raises(ValueError, match="device_hyper needs sanitize=True"):
            make(ps, device_hyper=True)
