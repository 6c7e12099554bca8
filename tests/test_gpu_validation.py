"""GPU: nsm_amd.Validator / validate — the reference's validate_direct
(main.py:583-664) as one captured graph per batch — against an eager
restatement of that loop on the same model, and the image metrics against the
numpy float64 yardstick of val_util.py on the eager outputs.

The totals are compared exactly: the graph's eval forward equals the eager one
bitwise (test_graphed_unet_follows_graphed_train_step), the criterion's kernels
fold in a fixed order, and the accumulator adds the same fp32 values in the
same order in fp64 as Python's float sum of the `.item()`s."""
import contextlib

import numpy as np
import pytest
import torch

import val_util as V

pytestmark = pytest.mark.gpu


def _setup(device, p=0.2, seed=3, B=2, C=7, H=64, batches=3, pert=False):
    import nsm_amd
    torch.manual_seed(seed)
    m = nsm_amd.Unet(in_ch=C, dropout_rate=p).to(device).train()
    opt = nsm_amd.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-3, max_grad_norm=1.0,
                            sanitize=True, seed=11)
    if pert:
        crit = nsm_amd.EnhancedCustomLoss(device, 0.9, vgg_weights=False)
    else:
        crit = nsm_amd.CustomLoss(device, 0.9, vgg_weights=False)
    g = torch.Generator(device=device).manual_seed(seed)
    data = [(torch.randn(B, C, H, H, device=device, generator=g),
             torch.rand(B, 1, H, H, device=device, generator=g)) for _ in range(batches)]
    return m, opt, crit, data


def restate(m, crit, data, ctx=contextlib.nullcontext):
    """validate_direct's loop, eagerly: dict of the means (val_util), the outputs'
    records against the targets, and the per-batch L1 of the yardstick."""
    pert = hasattr(crit, "perturbation_loss")
    was = m.training
    m.eval()
    totals, perts, recs, l1s = [], [], [], []
    with torch.no_grad(), ctx():
        for x, y in data:
            out = m(x)
            if pert:
                loss, parts = crit(m, out, y, x)
                perts.append(parts["perturbation_loss"].item())
            else:
                loss = crit(out, y, x)
            totals.append(loss.item())
            r = V.records(out.float().cpu().numpy(), y.float().cpu().numpy())
            recs.append(r)
            b = V.fold(r)
            l1s.append(b[V.S1] / b[V.COUNT])
    m.train(was)
    means = V.validate_direct_means(totals, l1s, perts if pert else None)
    return means, np.concatenate(recs)


def check(res, means, recs, what):
    assert res.loss == means["loss"], (what, res.loss, means["loss"])
    assert res.batches == means["batches"]
    assert float(res) == res.loss
    l1_err = V.rel(res.l1_loss, means["l1_loss"])
    ref = V.figures(V.fold(recs))
    m = res.metrics
    errs = {k: float(V.rel(getattr(m, k), ref[k])) for k in ("l1", "mse")}
    print(f"{what}: loss {res.loss!r}; l1_loss within {l1_err:.2e}, metrics within {errs}")
    assert l1_err <= V.BOUND and max(errs.values()) <= V.BOUND
    assert (m.count, m.max_abs, m.nonfinite, m.out_of_range) == \
        (ref["count"], ref["max_abs"], ref["nonfinite"], ref["out_of_range"])
    assert abs(m.psnr - ref["psnr"]) <= 4.35 * V.BOUND      # d psnr = (10 / ln 10) d mse / mse


def run(val, data):
    val.reset()
    for x, y in data:
        val.update(x, y)
    return val.compute()


def _training_state(m, opt):
    return [t.detach().clone() for t in list(m.parameters()) + list(m.buffers())
            + [opt.flat, opt.exp_avg, opt.exp_avg_sq]]


def test_validator_equals_the_eager_loop(device):
    """Three batches; and building and running the Validator leaves parameters, BN
    buffers, optimizer state and the model's mode as they were."""
    import nsm_amd
    m, opt, crit, data = _setup(device)
    before = _training_state(m, opt)
    val = nsm_amd.Validator(m, crit, *data[0], log_images=4)
    assert m.training and val.graph is not None and val.frozen is not None
    res = run(val, data)
    assert m.training
    for a, b in zip(before, _training_state(m, opt)):
        assert torch.equal(a, b)
    means, recs = restate(m, crit, data)
    check(res, means, recs, "CustomLoss, 3 batches")
    assert res.perturbation_loss == 0.0 and res.validator is val
    # the log: the first 4 of the 6 images
    p = res.per_image
    assert p.count.tolist() == recs[:4, V.COUNT].tolist()
    assert p.max_abs.tolist() == recs[:4, V.MAX].tolist()
    assert V.rel(p.mse.numpy(), recs[:4, V.S2] / recs[:4, V.COUNT]).max() <= V.BOUND
    # the same call sequence again: the same bits; reset() zeroes the state
    again = run(val, data)
    assert again.loss == res.loss and again.l1_loss == res.l1_loss
    assert again.metrics == res.metrics
    val.reset()
    zero = val.compute()
    assert zero.batches == 0 and zero.loss == float("inf") and zero.metrics.count == 0
    assert not val._acc.any() and not val._state.any() and not val._log.any()
    crit.check_range_now()


def test_perturbation_criterion_in_eval(device):
    """EnhancedCustomLoss in .eval(): no noise is drawn, the perturbation part is 0
    and the dict's parts come back as means over batches."""
    import nsm_amd
    m, _, crit, data = _setup(device, pert=True)
    crit.eval()
    val = nsm_amd.Validator(m, crit, *data[0])
    res = run(val, data)
    means, recs = restate(m, crit, data)
    check(res, means, recs, "EnhancedCustomLoss.eval(), 3 batches")
    assert res.perturbation_loss == 0.0 == means["perturbation_loss"]
    assert set(res.parts) == {"l1_loss", "vgg_loss", "perturbation_loss"}
    assert res.vgg_loss == 0.0
    # the criterion's own fp32 L1 beside the metrics pass's fp64 one
    assert abs(res.parts["l1_loss"] - res.l1_loss) <= 1e-6 * res.l1_loss
    assert not crit.training and m.training


def test_tail_batch_runs_eagerly(device):
    """drop_last=False: a last batch of one image does not fit the graph."""
    import nsm_amd
    m, _, crit, data = _setup(device)
    x, y = data[0]
    data = data + [(x[:1] * 0.5, y[:1])]
    val = nsm_amd.Validator(m, crit, *data[0])
    res = run(val, data)
    means, recs = restate(m, crit, data)
    check(res, means, recs, "3 batches + a tail of one image")
    assert res.batches == 4 and res.metrics.count == 7 * 64 * 64 and m.training
    # graph=False: every batch eagerly, the same figures
    plain = nsm_amd.Validator(m, crit, *data[0], graph=False)
    assert plain.graph is None
    res2 = run(plain, data)
    assert res2.loss == res.loss and res2.metrics == res.metrics


def test_weights_refresh_between_epochs(device):
    """Three GraphedTrainStep replays between two validations: the second follows
    the new weights and BN running statistics."""
    import nsm_amd
    m, opt, crit, data = _setup(device)
    step = nsm_amd.GraphedTrainStep(m, crit, opt, *data[0], warmup=1)
    val = nsm_amd.Validator(m, crit, *data[0])
    first = run(val, data)
    means, recs = restate(m, crit, data)
    check(first, means, recs, "before training")
    for _ in range(3):
        step()
    second = run(val, data)
    means, recs = restate(m, crit, data)
    check(second, means, recs, "after three steps")
    assert second.loss != first.loss and m.training


def test_validate_equals_the_validator_run(device):
    import nsm_amd
    m, _, crit, data = _setup(device)
    x, y = data[0]
    loader = [(a.cpu(), b.cpu()) for a, b in data] + [(x[:1].cpu(), y[:1].cpu())]
    res = nsm_amd.validate(m, loader, crit, log_images=2)
    val = res.validator
    assert isinstance(val, nsm_amd.Validator) and res.batches == 4
    ref = run(nsm_amd.Validator(m, crit, x, y), [(a.to(device), b.to(device)) for a, b in loader])
    assert res.loss == ref.loss and res.l1_loss == ref.l1_loss
    assert res.metrics == ref.metrics
    assert res.per_image.count.tolist() == [64 * 64] * 2 and ref.per_image is None
    # the validator again at the next epoch: it starts from zero
    again = nsm_amd.validate(m, loader, crit, validator=val)
    assert again.validator is val and again.loss == res.loss and again.batches == 4
    assert nsm_amd.validate(m, [], crit).loss == float("inf")
    best = float("inf")
    assert res < best


def test_bf16_autocast(device):
    """Captured inside torch.autocast('cuda', torch.bfloat16): the graph and the
    eager tail run the bf16 forward."""
    import nsm_amd
    m, _, crit, data = _setup(device)
    x, y = data[0]
    data = data + [(x[:1], y[:1])]

    def ctx():
        return torch.autocast("cuda", dtype=torch.bfloat16)

    with ctx():
        val = nsm_amd.Validator(m, crit, *data[0])
    res = run(val, data)          # outside the context: the construction's autocast state holds
    means, recs = restate(m, crit, data, ctx)
    check(res, means, recs, "bf16 autocast")
    fp32, _ = restate(m, crit, data)
    assert fp32["loss"] != means["loss"]
