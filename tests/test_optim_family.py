"""CPU: the three optimizers of main.py:952-957 on the flat buffer — the
`make_optimizer` factory, FlatAdam's / FlatSGD's checkpoint formats
(torch.optim.Adam's / torch.optim.SGD's, both directions), the options the
kernels do not implement, and the LambdaLR schedule on the new classes."""
import pytest
import torch


def _params(seed=0):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]


def _clone(ps):
    return [torch.nn.Parameter(p.detach().clone()) for p in ps]


@pytest.mark.parametrize("name,cls,wd,momentum", [
    ("adam", "FlatAdam", 1e-4, None),
    ("adamw", "FlatAdamW", 1e-3, None),
    ("sgd", "FlatSGD", 1e-4, 0.9),
    ("rmsprop", "FlatSGD", 1e-4, 0.9),     # main.py:956 `else:` -> SGD
    ("Adam", "FlatSGD", 1e-4, 0.9),        # the reference compares exactly
])
def test_make_optimizer_mirrors_reference_branches(name, cls, wd, momentum):
    import nsm_amd
    opt = nsm_amd.make_optimizer(_params(), name, 3e-4, max_grad_norm=1.0)
    assert type(opt) is getattr(nsm_amd, cls)
    g = opt.param_groups[0]
    assert g["lr"] == 3e-4 and g["weight_decay"] == wd
    assert g.get("momentum") == momentum
    assert opt.max_grad_norm == 1.0
    if momentum is None:
        assert tuple(g["betas"]) == (0.9, 0.999) and g["eps"] == 1e-8


def test_flat_sgd_allocates_one_buffer_or_none():
    import nsm_amd
    opt = nsm_amd.FlatSGD(_params())
    assert opt.momentum_buffer.shape == opt.flat.shape
    assert [t.data_ptr() for t in opt.step_state()[:2]] == [opt.flat.data_ptr(),
                                                            opt.momentum_buffer.data_ptr()]
    opt0 = nsm_amd.FlatSGD(_params(), momentum=0)
    assert opt0.momentum_buffer is None
    assert len(opt0.step_state()) == 4      # flat, step counters, flags, stat


def test_flat_adam_checkpoint_format_is_torch_adam():
    import nsm_amd
    ps = _params()
    ref_ps = _clone(ps)
    ref = torch.optim.Adam(ref_ps, lr=1e-3, weight_decay=1e-4)
    for _ in range(2):
        for p in ref_ps:
            p.grad = torch.randn_like(p)
        ref.step()
    sd = ref.state_dict()
    opt = nsm_amd.FlatAdam(ps, lr=5.0, weight_decay=0.0)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == 1e-3 and opt.param_groups[0]["weight_decay"] == 1e-4
    assert opt.steps_taken() == 2
    out = opt.state_dict()
    assert set(out["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    for i in range(2):
        assert torch.equal(out["state"][i]["exp_avg"], sd["state"][i]["exp_avg"])
        assert torch.equal(out["state"][i]["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
        assert float(out["state"][i]["step"]) == 2.0
    # torch's group keys and values, and it loads back into torch's Adam
    assert set(out["param_groups"][0]) == set(sd["param_groups"][0])
    back = torch.optim.Adam(_clone(ps))
    back.load_state_dict(out)
    bsd = back.state_dict()
    for k, v in sd["param_groups"][0].items():
        assert bsd["param_groups"][0][k] == v, k
    for i in range(2):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(bsd["state"][i][k], sd["state"][i][k]), (i, k)


def test_flat_sgd_checkpoint_format_is_torch_sgd():
    import nsm_amd
    ps = _params()
    ref_ps = _clone(ps)
    ref = torch.optim.SGD(ref_ps, lr=1e-3, momentum=0.8, weight_decay=1e-4)
    for _ in range(2):
        for p in ref_ps:
            p.grad = torch.randn_like(p)
        ref.step()
    sd = ref.state_dict()
    opt = nsm_amd.FlatSGD(ps, lr=5.0, momentum=0.9, weight_decay=0.0)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert g["lr"] == 1e-3 and g["momentum"] == 0.8 and g["weight_decay"] == 1e-4
    assert opt.steps_taken() >= 1           # buffers present: no re-initialisation
    out = opt.state_dict()
    assert set(out["param_groups"][0]) == set(sd["param_groups"][0])
    for i in range(2):
        assert set(out["state"][i]) == {"momentum_buffer"}
        assert torch.equal(out["state"][i]["momentum_buffer"], sd["state"][i]["momentum_buffer"])
    back = torch.optim.SGD(_clone(ps), lr=7.0)
    back.load_state_dict(out)
    bsd = back.state_dict()
    for k, v in sd["param_groups"][0].items():
        assert bsd["param_groups"][0][k] == v, k
    for i in range(2):
        assert torch.equal(bsd["state"][i]["momentum_buffer"], sd["state"][i]["momentum_buffer"])


@pytest.mark.parametrize("how", ["empty", "none_entries"])
def test_flat_sgd_checkpoint_without_buffers_keeps_first_step_pending(how):
    """A torch SGD that has not stepped has no state; torch versions that keep
    an entry before the buffer exists write {"momentum_buffer": None}. Either
    way the flat optimizer's next step is the initialising one, and what it
    exports has no buffers either."""
    import nsm_amd
    ps = _params()
    ref_ps = _clone(ps)
    ref = torch.optim.SGD(ref_ps, lr=1e-3, momentum=0.9, weight_decay=1e-4)
    sd = ref.state_dict()
    assert sd["state"] == {}
    if how == "none_entries":
        sd["state"] = {i: {"momentum_buffer": None} for i in range(len(ps))}
    # loaded over an optimizer that already holds buffers: they must not survive
    opt = nsm_amd.FlatSGD(ps, lr=5.0, momentum=0.9)
    stepped = torch.optim.SGD(_clone(ps), lr=1e-3, momentum=0.9)
    for p in stepped.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    stepped.step()
    opt.load_state_dict(stepped.state_dict())
    assert opt.steps_taken() == 1
    opt.load_state_dict(sd)
    assert opt.steps_taken() == 0
    out = opt.state_dict()
    assert out["state"] == {}
    back = torch.optim.SGD(_clone(ps), lr=7.0)
    back.load_state_dict(out)
    assert back.state_dict()["state"] == {}
    for k, v in sd["param_groups"][0].items():
        assert back.state_dict()["param_groups"][0][k] == v, k


def test_flat_sgd_rejects_partial_buffers():
    import nsm_amd
    ps = _params()
    ref_ps = _clone(ps)
    ref = torch.optim.SGD(ref_ps, lr=1e-3, momentum=0.9)
    ref_ps[0].grad = torch.ones_like(ref_ps[0])      # the second parameter never steps
    ref.step()
    with pytest.raises(ValueError):
        nsm_amd.FlatSGD(ps).load_state_dict(ref.state_dict())


@pytest.mark.parametrize("cls,kw", [
    ("FlatAdam", dict(amsgrad=True)),
    ("FlatAdam", dict(maximize=True)),
    ("FlatSGD", dict(nesterov=True)),
    ("FlatSGD", dict(dampening=0.1)),
    ("FlatSGD", dict(maximize=True)),
])
def test_unsupported_options_raise(cls, kw):
    import nsm_amd
    with pytest.raises(ValueError):
        getattr(nsm_amd, cls)(_params(), **kw)
    # the same option arriving in a checkpoint is refused too, not ignored
    twin = {"FlatAdam": torch.optim.Adam, "FlatSGD": torch.optim.SGD}[cls]
    tkw = dict(kw, momentum=0.9) if "nesterov" in kw else kw
    sd = twin(_clone(_params()), lr=1e-3, **tkw).state_dict()
    with pytest.raises(ValueError):
        getattr(nsm_amd, cls)(_params()).load_state_dict(sd)


@pytest.mark.parametrize("cls", ["FlatAdam", "FlatSGD"])
def test_more_than_one_param_group_raises(cls):
    import nsm_amd
    a, b = _params()
    with pytest.raises(ValueError):
        getattr(nsm_amd, cls)([{"params": [a]}, {"params": [b], "lr": 1e-2}])


@pytest.mark.parametrize("cls,twin", [("FlatAdam", torch.optim.Adam), ("FlatSGD", torch.optim.SGD)])
def test_lambda_lr_drives_new_optimizers_like_torch(cls, twin):
    import nsm_amd
    from nsm_amd.optim import make_lambda_lr
    warm, epochs, lr0 = 2, 3, 7e-4
    opt = getattr(nsm_amd, cls)(_params(), lr=lr0)
    ref = twin(_clone(_params()), lr=lr0)
    s1, s2 = make_lambda_lr(opt, warm, epochs), make_lambda_lr(ref, warm, epochs)
    got, want = [], []
    for _ in range(epochs):
        got.append(opt.param_groups[0]["lr"])
        want.append(ref.param_groups[0]["lr"])
        s1.step()
        s2.step()
    assert got == want
    assert want[0] == 0.0 and want[1] == lr0 * 0.5 and want[2] == lr0
