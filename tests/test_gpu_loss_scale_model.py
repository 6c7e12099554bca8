"""GPU, model level: the device-side dynamic loss scaler on the fp16 training
step of the Unet (7 channels, 2 x 64 x 64, the fixtures' size): the scale finds
its level from 2^40, `scaler.scale(loss).backward()` is `loss.backward(scaler.seed)`,
GraphedTrainStep follows the moving scale with one capture, and a disabled
scaler changes nothing.

Observed on the MI355X at this shape (facts, not bounds): see DESIGN.md, "The
dynamic loss scaler"."""
import pytest
import torch

import loss_scale_util as U

pytestmark = pytest.mark.gpu
INIT_SCALE = 2.0 ** 40


def _setup(device, scaler=None, f16=True, seed=3):
    import nsm_amd
    torch.manual_seed(seed)
    m = nsm_amd.Unet(in_ch=7, dropout_rate=0.0).to(device).train()
    if f16:
        m.set_compute_dtype(torch.float16)
    kw = {} if scaler is None else {"grad_scaler": scaler}
    opt = nsm_amd.FlatAdamW(m.parameters(), lr=1e-3, max_grad_norm=1.0, sanitize=True, seed=11,
                            **kw)
    crit = nsm_amd.CustomLoss(device, 0.9, vgg_weights=False)
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(2, 7, 64, 64, device=device, generator=g)
    y = torch.rand(2, 1, 64, 64, device=device, generator=g)
    return m, opt, crit, x, y


def _scaler(device, interval=4, init=INIT_SCALE, **kw):
    import nsm_amd
    return nsm_amd.GradScaler(init_scale=init, growth_interval=interval, on_overflow="skip",
                              device=device, **kw)


def _state(m, opt):
    return [t.detach().clone() for t in opt.step_state() + list(m.buffers())]


def _biteq(a, b):
    """Bitwise equality (equal NaNs, as an overflowed norm in `stat`, are equal)."""
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.dtype == b.dtype and torch.equal(a, b)


def _eager_step(m, opt, crit, x, y, sc):
    loss = crit(m(x), y, x)
    loss.backward(sc.seed)
    sc.step(opt)
    sc.update()
    opt.zero_grad()
    return loss


def test_scale_finds_its_level(device):
    sc = _scaler(device)
    m, opt, crit, x, y = _setup(device, sc)
    before = opt.flat.detach().clone()
    scale, tracker, first_taken, record = INIT_SCALE, 0, None, []
    for s in range(64):
        _eager_step(m, opt, crit, x, y, sc)
        st, fl = sc.last(), opt.last_flags()
        if s == 0:       # 2^40 overflows the f16 activation gradients: skipped, nothing moved
            assert st["found_inf"] == 1 and fl["skip"] == 1, (st, fl)
            assert torch.equal(opt.flat, before) and opt.steps_taken() == 0
        # every scale change is the rule's, replayed from the recorded found_inf
        assert fl["skip"] == 1 if st["found_inf"] else True
        scale, tracker = U.update(scale, tracker, st["found_inf"], 2.0, 0.5, 4,
                                  other_skip=bool(fl["skip"]) and not st["found_inf"])
        assert (st["scale"], st["growth_tracker"]) == (scale, tracker), (s, st)
        record.append((st["found_inf"], fl["skip"], scale))
        if first_taken is None and not fl["skip"]:
            first_taken = s
        if first_taken is not None and s >= first_taken + 8:
            break
    print("loss-scale settling: first step taken at", first_taken, "scale there",
          None if first_taken is None else record[first_taken][2], "steps run", len(record),
          "steps taken", opt.steps_taken(), "final", sc.last())
    print("(found_inf, skip, log2 scale):",
          [(f, k, int(torch.log2(torch.tensor(v)).item())) for f, k, v in record])
    assert first_taken is not None and opt.steps_taken() >= 1      # within the 64-step cap
    assert sc.last()["overflows"] == sum(r[0] for r in record)
    assert not torch.equal(opt.flat, before)
    for t in list(m.parameters()) + list(m.buffers()):
        assert torch.isfinite(t).all()


def test_scale_loss_backward_is_seeded_backward(device):
    from nsm_amd.optim import flat_grad
    sc = _scaler(device, init=2.0 ** 12)
    m, opt, crit, x, y = _setup(device, sc)
    crit(m(x), y, x).backward(sc.seed)
    a = flat_grad(list(m.parameters())).clone()
    opt.zero_grad()
    sc.scale(crit(m(x), y, x)).backward()
    b = flat_grad(list(m.parameters())).clone()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.isfinite(a).all() and a.abs().max().item() > 0
    # and it is the scale's multiple of the unscaled gradient's size
    opt.zero_grad()
    crit(m(x), y, x).backward()
    c = flat_grad(list(m.parameters())).clone()
    assert 0.5 * 2.0 ** 12 < (a.norm() / c.norm()).item() < 2.0 * 2.0 ** 12


def test_graphed_step_follows_the_scale_without_recapture(device):
    """Eight replays from 2^40 equal eight eager steps bitwise (parameters,
    moments, counters, BN buffers, the scaler's state) across several
    backoffs, on one capture; building the step leaves the scaler as it was."""
    import nsm_amd
    sc, sc2 = _scaler(device), _scaler(device)
    m, opt, crit, x, y = _setup(device, sc)
    m2, opt2, crit2, _, _ = _setup(device, sc2)
    before = _state(m, opt)
    step = nsm_amd.GraphedTrainStep(m, crit, opt, x, y, warmup=2, grad_scaler=sc)
    assert step._seed is sc.seed
    for a, b in zip(before, _state(m, opt)):
        assert _biteq(a, b)
    assert sc.last() == dict(scale=INIT_SCALE, growth_tracker=0, found_inf=0, overflows=0,
                             growths=0)
    graph, captures = step.graph, []
    capture = step._capture
    step._capture = lambda *a, **k: (captures.append(1), capture(*a, **k))
    scales = []
    for _ in range(8):
        lg = step()
        le = _eager_step(m2, opt2, crit2, x, y, sc2)
        assert _biteq(lg, le)
        assert step.graph is graph
        for a, b in zip(_state(m, opt), _state(m2, opt2)):
            assert _biteq(a, b)
        assert sc.last() == sc2.last()
        scales.append(sc.last()["scale"])
    assert not captures                                  # the moving scale never re-captured
    assert sc.last()["overflows"] >= 3, sc.last()        # several backoffs
    assert len(set(scales)) >= 4, scales
    # a scale set by hand is written in place: still the same capture, and from
    # 2^10 the steps are taken
    taken = opt.steps_taken()
    for s_ in (sc, sc2):
        s_.update(new_scale=2.0 ** 10)
    for _ in range(3):
        lg = step()
        le = _eager_step(m2, opt2, crit2, x, y, sc2)
        assert _biteq(lg, le) and step.graph is graph and not captures
        for a, b in zip(_state(m, opt), _state(m2, opt2)):
            assert _biteq(a, b)
    assert opt.steps_taken() == opt2.steps_taken() == taken + 3
    assert sc.last()["growth_tracker"] == 3 and sc.last()["scale"] == 2.0 ** 10
    with pytest.raises(ValueError):
        nsm_amd.GraphedTrainStep(m, crit, opt, x, y, loss_scale=2.0, warmup=0, grad_scaler=sc)


def test_disabled_scaler_is_the_step_without_one(device):
    import nsm_amd
    sc = nsm_amd.GradScaler(enabled=False)
    m, opt, crit, x, y = _setup(device, sc, f16=False)
    m2, opt2, crit2, _, _ = _setup(device, None, f16=False)
    assert opt.step_hyper() == opt2.step_hyper()
    assert len(opt.step_state()) == len(opt2.step_state())
    for _ in range(2):
        sc.scale(crit(m(x), y, x)).backward()
        sc.step(opt)
        sc.update()
        opt.zero_grad()
        crit2(m2(x), y, x).backward()
        opt2.step()
        opt2.zero_grad()
    assert opt.steps_taken() == opt2.steps_taken() == 2
    for a, b in zip(_state(m, opt), _state(m2, opt2)):
        assert _biteq(a, b)
