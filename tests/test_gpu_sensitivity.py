"""GPU: the feature-sensitivity analysis (nsm_amd.feature_sensitivity, the
paper's Eq. 1) and its two kernels against torch constructions and the float64
comparator of sensitivity_util.py."""
import math

import pytest
import torch

import sensitivity_util as U
from oracle.weights import synthetic_batch
from util import OUT_ABS

pytestmark = pytest.mark.gpu

# nsm_sens_reduce sums in a fixed fp32 tree of 11 levels (8 per thread, the
# wave, the 4 waves) over the rounded differences, and nsm_sens_finalize goes on
# in double: the error is below 17 levels x 2^-24 of sum|d|, doubled.
REDUCE_TOL = 2e-6


def _slots(x, sigma, channels, repeats, factor, chunk, noises=None, seed=0):
    """All B * (1 + C' * R) slots of the plan, generated `chunk` at a time, and
    the filler slots of the last chunk."""
    from nsm_amd.sensitivity import sens_variants
    B, C, H, W = x.shape
    N = B * (1 + len(channels) * repeats)
    ch = torch.tensor(channels, dtype=torch.int32, device=x.device)
    parts = []
    for first in range(0, N, chunk):
        out = torch.full((chunk, C, H, W), float("nan"), device=x.device)
        sens_variants(x, sigma, ch, repeats, factor, first, chunk, out, noises, seed)
        parts.append(out)
    full = torch.cat(parts)
    return full[:N], full[N:]


@pytest.mark.parametrize("H,W", [(20, 36), (64, 64), (9, 7)])
def test_variants_injected_noise_bitwise(device, H, W):
    """Every slot equals torch's x[:, i] + z * s bit for bit, untouched planes
    equal x, fillers hold image 0, and the chunking does not matter. (9 x 7 has
    planes that are no multiple of a 16-byte vector.)"""
    B, C, R, factor = 2, 7, 2, 0.1
    channels = [5, 0, 3]
    gen = torch.Generator().manual_seed(H * W)
    x = torch.randn((B, C, H, W), generator=gen).to(device)
    sigma = (0.5 + torch.rand(C, generator=gen)).to(device)
    z = torch.randn((len(channels), R, B, H, W), generator=gen).to(device)
    a, fill_a = _slots(x, sigma, channels, R, factor, 3, z)
    b, fill_b = _slots(x, sigma, channels, R, factor, 16, z)
    assert fill_a.shape[0] == 1 and fill_b.shape[0] == 2
    assert torch.equal(a, b)
    assert torch.equal(a[:B], x)
    for f in (*fill_a, *fill_b):
        assert torch.equal(f, x[0])
    for ii, c in enumerate(channels):
        s = sigma[c] * factor
        for r in range(R):
            for img in range(B):
                want = x[img].clone()
                want[c] = x[img, c] + z[ii, r, img] * s
                got = a[B + (ii * R + r) * B + img]
                assert torch.equal(got, want), (c, r, img)


def test_variants_device_generator(device):
    B, C, H, W, R, factor = 2, 4, 64, 64, 4, 0.1
    channels = list(range(C))
    x = torch.from_numpy(synthetic_batch(B, C, H, W)[0]).to(device)
    sigma = torch.linspace(1, 2, C).to(device)
    N = B * (1 + C * R)
    a, _ = _slots(x, sigma, channels, R, factor, N, seed=1234)
    again, _ = _slots(x, sigma, channels, R, factor, N, seed=1234)
    other, _ = _slots(x, sigma, channels, R, factor, N, seed=1235)
    chunked, _ = _slots(x, sigma, channels, R, factor, 5, seed=1234)
    assert torch.equal(a, again) and torch.equal(a, chunked)
    assert torch.equal(a[:B], x)
    var = a[B:].view(C, R, B, C, H, W)
    delta = var - x.view(1, 1, B, C, H, W)
    zs = []
    for i in range(C):
        for c in range(C):
            if c != i:      # only channel i differs from x in variant (i, .)
                assert torch.equal(var[i, :, :, c], x[:, c].expand(R, B, H, W))
        zs.append(delta[i, :, :, i].double() / (sigma[i] * factor).double())
    z = torch.stack(zs)                                      # [C, R, B, H, W]
    assert not torch.equal(var, other[B:].view_as(var))
    tex = z.view(C * R * B, H * W)
    same = (tex.unsqueeze(0) == tex.unsqueeze(1)).all(-1).sum().item()
    assert same == tex.shape[0]                              # each texture equals only itself
    n = z.numel()
    mean, variance = z.mean().item(), z.var().item()
    print(f"generator: {n} normals, mean {mean:+.5f} (5 sigma {5 / math.sqrt(n):.5f}), "
          f"variance {variance:.5f} (5 sigma {5 * math.sqrt(2 / n):.5f})")
    assert n == 131072
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(variance - 1) <= 5 * math.sqrt(2 / n)


@pytest.mark.parametrize("n", [2 * 31 * 2 * 19, 128 * 128, 1001])
def test_reduce_against_float64(device, n):
    """Five variant slots over three base images (B = 3, one channel, two
    repeats: the sixth variant is not in the chunk and its words stay as they
    were). 1001 takes the path without 16-byte vectors."""
    from nsm_amd import lib
    from nsm_amd.sensitivity import sens_reduce
    B, Cs, R = 3, 1, 2
    gen = torch.Generator().manual_seed(n)
    base = torch.rand((B, n), generator=gen).to(device)
    out = (base[[0, 1, 2, 0, 1]].cpu() + 0.05 * torch.randn((5, n), generator=gen)).to(device)
    per = lib.nsm_sens_blocks(n)
    assert per == -(-n // 2048)
    runs = []
    for _ in range(2):
        psum = torch.full((Cs * R * B, per, 2), -7.0, device=device)
        sens_reduce(out, base, B, B, Cs, R, psum)
        runs.append(psum)
    assert torch.equal(runs[0], runs[1])
    assert (runs[0][5] == -7.0).all()
    got = runs[0][:5].double().sum(1).cpu()
    d = out.double().cpu() - base.double().cpu()[[0, 1, 2, 0, 1]]
    want_abs, want_sum = d.abs().sum(1), d.sum(1)
    err_a = ((got[:, 0] - want_abs).abs() / want_abs).max().item()
    err_s = ((got[:, 1] - want_sum).abs() / want_abs).max().item()
    print(f"reduce n={n}: sum|d| err {err_a:.2e}, sum d err {err_s:.2e} (of sum|d|; bound {REDUCE_TOL})")
    assert err_a <= REDUCE_TOL and err_s <= REDUCE_TOL


@pytest.fixture(scope="module")
def model(device):
    import nsm_amd
    m = nsm_amd.Unet(in_ch=4, dropout_rate=0.0)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in U.sens_model_state().items()})
    return m.to(device).train()


@pytest.mark.parametrize("chunk", [3, 8])
def test_end_to_end_against_cpu_oracle(device, model, chunk):
    """|S_i - S_i^ref| <= 2 * OUT_ABS / (factor * sigma_i): each of the two
    outputs of a difference may be off by the project's eval output bound."""
    import nsm_amd
    x, sigma, noises, (ref_abs, ref_signed, ref_rel, ref_terms) = U.e2e_case()
    bound = 2 * OUT_ABS / (U.E2E_FACTOR * sigma.double())
    assert (ref_abs >= 20 * bound).all()          # on the reference alone
    before = [p.detach().clone() for p in model.parameters()]
    res = nsm_amd.feature_sensitivity(model, x.to(device), sigma, repeats=U.E2E_REPEATS,
                                      factor=U.E2E_FACTOR, chunk=chunk, noises=noises)
    assert model.training
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
    absolute, relative = res.absolute.double().cpu(), res.relative.double().cpu()
    signed, terms = res.signed.double().cpu(), res.terms.double().cpu()
    err = (absolute - ref_abs).abs()
    print(f"chunk {chunk}: S {absolute.tolist()} ref {ref_abs.tolist()} err/bound "
          f"{(err / bound).tolist()} signed {signed.tolist()} ref {ref_signed.tolist()}")
    assert (err <= bound).all()
    # s = S / T: |s - s'| <= (|S - S'| + s' |T - T'|) / T with T >= T' - sum of the bounds
    rel_bound = (bound + ref_rel * bound.sum()) / (ref_abs.sum() - bound.sum())
    assert ((relative - ref_rel).abs() <= rel_bound).all()
    assert abs(relative.sum().item() - 1) <= 1e-6
    assert (signed.abs() <= absolute).all()
    assert tuple(terms.shape) == tuple(ref_terms.shape)
    count = terms.shape[1] * terms.shape[2] * x[0, :1].numel()
    s = (sigma * U.E2E_FACTOR).double()
    from_terms = terms[..., 0].sum((1, 2)) / (count * s)
    assert ((from_terms - absolute).abs() <= 1e-6 * absolute).all()
    from_terms = terms[..., 1].sum((1, 2)) / (count * s)
    assert ((from_terms - signed).abs() <= 1e-6 * absolute).all()
    assert (terms[..., 1].abs() <= terms[..., 0]).all()


def test_streaming_equals_one_shot(device, model):
    import nsm_amd
    R, factor = 2, 0.5
    x = torch.from_numpy(synthetic_batch(3, 4, 32, 32, seed_x=5)[0]).to(device)
    sigma = torch.linspace(1, 2, 4)
    z = torch.randn((4, R, 3, 32, 32), generator=torch.Generator().manual_seed(9)).to(device)
    one = nsm_amd.feature_sensitivity(model, x, sigma, repeats=R, factor=factor, chunk=4, noises=z)
    model.eval()
    before = [p.detach().clone() for p in model.parameters()]
    acc = nsm_amd.FeatureSensitivity(model, sigma, repeats=R, factor=factor, chunk=4)
    acc.update(x[:1], noises=z[:, :, :1])
    first = [t.clone() for t in acc.compute()[:3]]
    acc.update(x[1:], noises=z[:, :, 1:])
    got = acc.compute()
    assert not model.training                     # restored to what it was, as after the one-shot call
    model.train()
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
    da = ((got.absolute - one.absolute).abs() / one.absolute).max().item()
    ds = ((got.signed - one.signed).abs() / one.absolute).max().item()
    dr = (got.relative - one.relative).abs().max().item()
    print(f"streaming vs one-shot: absolute {da:.2e}, signed {ds:.2e} (of absolute), relative {dr:.2e}")
    assert da <= REDUCE_TOL and ds <= REDUCE_TOL and dr <= 2 * REDUCE_TOL
    acc.reset()
    assert (acc._acc == 0).all()
    acc.update(x[:1], noises=z[:, :, :1])
    again = acc.compute()
    assert all(torch.equal(a, b) for a, b in zip(again[:3], first))
    # another input shape re-captures
    small = x[:2, :, :20, :28].contiguous()
    zs = z[:, :, :2, :20, :28].contiguous()
    acc.reset()
    acc.update(small, noises=zs)
    want = nsm_amd.feature_sensitivity(model, small, sigma, repeats=R, factor=factor, chunk=4,
                                       noises=zs)
    assert all(torch.equal(a, b) for a, b in zip(acc.compute(), want))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_sixteen_bit_modes_run(device, model, dtype):
    import nsm_amd
    x, sigma, noises, (ref_abs, _, _, _) = U.e2e_case()
    model.set_compute_dtype(dtype)
    try:
        res = nsm_amd.feature_sensitivity(model, x.to(device), sigma, repeats=U.E2E_REPEATS,
                                          factor=U.E2E_FACTOR, noises=noises)
    finally:
        model.set_compute_dtype(None)
    absolute, relative = res.absolute.double().cpu(), res.relative.double().cpu()
    print(f"{dtype}: S {absolute.tolist()} deviation from the fp32 reference "
          f"{((absolute - ref_abs) / ref_abs).tolist()} relative {relative.tolist()}")
    assert torch.isfinite(absolute).all() and (absolute > 0).all()
    assert torch.isfinite(res.signed).all() and torch.isfinite(res.terms).all()
    assert abs(relative.sum().item() - 1) <= 1e-6
