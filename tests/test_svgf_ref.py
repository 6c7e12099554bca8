"""CPU: the float64 restatement of the SVGF denoiser (svgf_util.py) and its
seeded inputs: the decision margins of every case, that the edge weights of the
"planes" scene leave a filter to test (not a pass-through), that the filter
denoises, and the identities of the recurrence."""
import pytest
import torch

import svgf_util as S
import temporal_util as U

torch.set_num_threads(16)
IDS = ["x".join(map(str, s)) for s in S.SHAPES]


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_decision_margins(shape, family):
    """Position, depth, normal and nearest-tap rounding of every frame pair keep
    temporal_util.MARGIN, with both parameter sets (the verdicts do not depend
    on them, the lengths do)."""
    capped = (shape, family) == S.CAP_CASE
    for params in ("default", "cap") if capped else ("default",):
        _, r64, r32 = S.reference(shape, family, True, params)
        assert len(r64["out"]) == S.T == 6
        for t in range(1, S.T):
            m = r64["margins"][t]
            assert set(m) >= {"border", "depth", "normal", "nearest"}, m
            assert min(m.values()) >= U.MARGIN, (t, m)
            assert torch.equal(r64["accepted"][t], r32["accepted"][t])
            assert torch.equal(r64["length"][t], r32["length"][t].double())
            assert r64["accepted"][t].any()
    _, r64, _ = S.reference(shape, family, True, "default")
    if family == "planes":      # N passes min_history (random motion rejects too often for that)
        assert r64["length"][-1].max().item() > S.PARAMS["min_history"]
    else:
        assert r64["length"][-1].max().item() >= 2
    if capped:
        _, cap, _ = S.reference(shape, family, True, "cap")
        assert cap["length"][-1].max().item() == 4 and (r64["length"][-1] > cap["length"][-1]).any()


@pytest.mark.parametrize("shape", [(2, 1, 19, 37), (2, 1, 67, 129)], ids=["19x37", "67x129"])
def test_planes_filter_is_not_a_pass_through_and_denoises(shape):
    """On "planes", from the true variance: at every one of the 5 iterations at
    least 0.1 of the in-image non-centre taps weigh more than 1e-3 h(dx) h(dy),
    and the 5 iterations bring the MSE against the clean signal to at most 0.2
    of the noisy input's."""
    frames, _, depth, normals, clean = S.inputs(shape, "planes")
    c = frames[0].double()
    v = torch.full((shape[0], 1) + shape[2:], S.SIGMA_NOISE ** 2, dtype=torch.float64)
    p = S.PARAMS
    for i in range(5):
        c, v, share = S.atrous(c, v, depth[0], normals[0], 1 << i, p["sigma_z"], p["sigma_n"],
                               p["sigma_l"])
        print(f"{shape} iteration {i}: share of live taps {share:.2f}")
        assert share >= 0.1
    mse_in = (frames[0].double() - clean[0].double()).pow(2).mean().item()
    mse_out = (c - clean[0].double()).pow(2).mean().item()
    print(f"{shape}: MSE {mse_in:.5f} -> {mse_out:.5f} ({mse_out / mse_in:.3f})")
    assert mse_out <= 0.2 * mse_in


@pytest.mark.parametrize("family", S.FAMILIES)
def test_identities(family):
    """iterations = 0 with alpha = moments_alpha = 1 returns the input frames;
    a first frame has N = 1 everywhere and no accepted pixel."""
    shape = (2, 1, 19, 37)
    frames, mvs, depth, normals, _ = S.inputs(shape, family)
    r = S.sequence(frames, mvs, depth, normals, iterations=0, alpha=1.0, moments_alpha=1.0)
    for t in range(S.T):
        assert torch.equal(r["out"][t], frames[t].double())
    _, r64, _ = S.reference(shape, family)
    assert (r64["length"][0] == 1).all() and not r64["accepted"][0].any()
    assert torch.equal(r64["var"][0] >= 0, torch.ones_like(r64["var"][0], dtype=torch.bool))


def test_random_family_is_centre_only():
    """temporal_util.inputs has independent depth and normals per pixel: almost
    every tap weight vanishes, which is the centre-only path."""
    shape = (2, 1, 19, 37)
    frames, _, depth, normals, _ = S.inputs(shape, "random")
    v = torch.full((2, 1, 19, 37), 0.02, dtype=torch.float64)
    _, _, share = S.atrous(frames[0], v, depth[0], normals[0], 1)
    assert share < 0.1
