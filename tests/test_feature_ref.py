"""CPU: the feature recipe (nsm_amd/features.py), the numpy restatement the GPU
tests compare against (feature_util.compose_ref) and the argument checks of the
C entry, none of which needs a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import feature_util as U
import frame_util as F


def f32(v):
    return np.float32(v)


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the recipe -----------------------------------------------------------------
def test_parse_terms_table_round_trip():
    from nsm_amd import FeatureRecipe
    from nsm_amd import features as M
    assert (M.RAW, M.SUB, M.RATIO, M.DOT3) == (0, 1, 2, 3)
    r = U.recipe6()
    explicit = [("raw", 4), ("sub", 4, 8), ("ratio", 4, 8), ("ratio", 10, 0), ("dot3", 1, 5), 9]
    e = FeatureRecipe(explicit, in_channels=11)
    assert r == e and hash(r) == hash(e)
    assert r.in_channels == 11 and r.out_channels == 6 and r.ratio_floor == float(f32(1e-6))
    assert r.names == tuple(U.EXPRS) and e.names is None
    assert r.terms == (("raw", 4), ("sub", 4, 8), ("ratio", 4, 8), ("ratio", 10, 0),
                       ("dot3", 1, 5), ("raw", 9))
    t = r.table()
    assert t.dtype == np.int32 and t.shape == (6, 3)
    assert t.tolist() == [[0, 4, 0], [1, 4, 8], [2, 4, 8], [2, 10, 0], [3, 1, 5], [0, 9, 0]]
    # the table names the same recipe again
    back = FeatureRecipe([(M.OPS[op], a) if op == 0 else (M.OPS[op], a, b) for op, a, b in t.tolist()],
                         in_channels=11)
    assert back == r
    assert r.planes_read() == list(range(11))
    assert FeatureRecipe([0, ("sub", 2, 0)], 4).planes_read() == [0, 2]
    ident = FeatureRecipe.identity(7)
    assert ident.table().tolist() == [[0, c, 0] for c in range(7)] and ident.in_channels == 7
    wide = FeatureRecipe.parse(["z"], layout=U.LAYOUT, in_channels=12, ratio_floor=0.5)
    assert wide.in_channels == 12 and wide.ratio_floor == 0.5 and wide != r
    with pytest.raises(AttributeError):
        r.ratio_floor = 1.0
    with pytest.raises(AttributeError):
        r._terms = ()


def test_every_validation_error():
    from nsm_amd import FeatureRecipe
    bad = [
        (dict(terms=[("mul", 0, 1)], in_channels=4), "mul"),                   # bad op
        (dict(terms=[("sub", 0)], in_channels=4), "sub"),                      # arity
        (dict(terms=[("raw", 0, 1)], in_channels=4), "raw"),
        (dict(terms=[0.5], in_channels=4), "0.5"),
        (dict(terms=[True], in_channels=4), "True"),
        (dict(terms=[4], in_channels=4), r"\('raw', 4\)"),                     # index out of range
        (dict(terms=[("sub", 0, -1)], in_channels=4), r"\('sub', 0, -1\)"),
        (dict(terms=[("ratio", 4, 0)], in_channels=4), r"\('ratio', 4, 0\)"),
        (dict(terms=[("dot3", 0, 2)], in_channels=4), r"\('dot3', 0, 2\)"),     # j + 2 = 4 runs off
        (dict(terms=[("dot3", 2, 0)], in_channels=4), r"\('dot3', 2, 0\)"),
        (dict(terms=[], in_channels=4), "0 terms"),                            # Cout = 0
        (dict(terms=[0] * 17, in_channels=4), "17 terms"),                     # Cout = 17
        (dict(terms=[0], in_channels=0), "in_channels"),
        (dict(terms=[0], in_channels=65), "in_channels"),
        (dict(terms=[0], in_channels=4, ratio_floor=-1.0), "ratio_floor"),
        (dict(terms=[0], in_channels=4, ratio_floor=float("nan")), "ratio_floor"),
        (dict(terms=[0, 1], in_channels=4, names=["a"]), "names"),
    ]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            FeatureRecipe(**kw)
    assert FeatureRecipe([0] * 16, 64).out_channels == 16                      # the limits themselves
    assert FeatureRecipe([("dot3", 1, 0)], 4).out_channels == 1
    for exprs, word in (([".n"], "parse"), (["z*zf"], "parse"), (["z-q"], "'q'"), ([3], "parse")):
        with pytest.raises(ValueError, match=word):
            FeatureRecipe.parse(exprs, layout=U.LAYOUT)
    with pytest.raises(ValueError, match="string"):
        FeatureRecipe.parse("z-zf", layout=U.LAYOUT)
    with pytest.raises(ValueError, match="identity"):
        FeatureRecipe.identity(17)
    # a Cin mismatch: what compose_features, FramePipeline, dataset_stats and from_dir raise
    with pytest.raises(ValueError, match="11 raw channels, the frames have 7"):
        U.recipe6().check_input(7)
    U.recipe6().check_input(11)


# ---- 2. the restatement ----------------------------------------------------------------
@pytest.mark.parametrize("shape", F.PREP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_identity_equals_the_frame_oracle(shape):
    """The identity recipe is prepare_frames: prep_ref and prep_census bit for bit."""
    from nsm_amd import FeatureRecipe
    x = F.prep_input(shape)
    B, C, H, W = shape
    r = FeatureRecipe.identity(C)
    g = torch.Generator().manual_seed(3)
    stats = (torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5)
    for m in (16, None):
        Hp, Wp = F.padded(H, m), F.padded(W, m)
        for scrub, st in ((True, None), (False, None), (True, stats)):
            ref = F.prep_ref(x, pad_multiple=m, scrub_on=scrub, stats=st)
            got, census = U.compose_ref(x.numpy(), r, Hp, Wp, scrub=scrub,
                                        stats=None if st is None else (st[0].numpy(), st[1].numpy()))
            assert torch.equal(U.bits(torch.from_numpy(got)), U.bits(ref)), (m, scrub)
            assert torch.equal(torch.from_numpy(census), F.prep_census(x))
    assert F.prep_census(x).sum() > 0


def one_pixel(values, recipe, **kw):
    x = np.asarray(values, dtype=np.float32).reshape(1, -1, 1, 1)
    out, census = U.compose_ref(x, recipe, **kw)
    return out.reshape(-1), census.reshape(-1)


def test_ratio_guard():
    from nsm_amd import FeatureRecipe
    for floor in (1e-6, 0.25):
        r = FeatureRecipe([("ratio", 0, 1)], 2, ratio_floor=floor)
        below, at, above = U._around(floor)
        assert below < at < above and at == f32(r.ratio_floor)
        a = f32(3.0)
        for sign in (1.0, -1.0):
            for b in (below, at, f32(0.0)):
                out, _ = one_pixel([a, f32(sign) * b], r)
                assert bits_of(out)[0] == 0, (floor, sign, b)            # +0.0, whatever the sign
            out, _ = one_pixel([a, f32(sign) * above], r)
            assert out[0] == a / (f32(sign) * above) and out.dtype == np.float32
            assert abs(out[0]) > 1
            out, _ = one_pixel([a, f32(sign) * f32(np.inf)], r)
            assert out[0] == 0 and np.signbit(out[0]) == (sign < 0)      # 3 / -Inf = -0.0
        out, census = one_pixel([a, np.nan], r)                          # NaN is not below the floor
        assert np.isnan(out[0]) and census.tolist() == [1, 0, 0]
        out, census = one_pixel([a, np.nan], r, scrub=True)              # ... and the scrub takes it
        assert bits_of(out)[0] == 0 and census.tolist() == [1, 0, 0]
        out, census = one_pixel([np.inf, np.inf], r)
        assert np.isnan(out[0]) and census.tolist() == [1, 0, 0]
        out, census = one_pixel([U.FLT_MAX, 0.5], r)
        assert out[0] == np.inf and census.tolist() == [0, 1, 0]
    # a floor of 0 guards the division by zero only
    r0 = FeatureRecipe([("ratio", 0, 1)], 2, ratio_floor=0.0)
    assert bits_of(one_pixel([1.0, -0.0], r0)[0])[0] == 0
    assert one_pixel([1.0, 1e-30], r0)[0][0] == f32(1.0) / f32(1e-30)


def test_dot3_order_and_overlap():
    from nsm_amd import FeatureRecipe
    v = np.array([1.0000001, 3.3333333, -7.7777777, 0.1234567, 2.7182817], dtype=np.float32)
    for i, j in ((0, 0), (0, 1), (1, 0), (0, 2), (2, 2)):
        out, _ = one_pixel(v, FeatureRecipe([("dot3", i, j)], 5))
        want = (v[i] * v[j] + v[i + 1] * v[j + 1]) + v[i + 2] * v[j + 2]   # np.float32 scalars
        assert isinstance(want, np.float32) and bits_of(out)[0] == bits_of(want)[0], (i, j)
    # left to right: (big + -big) + 1 is 1, big + (-big + 1) is 0
    big = np.array([2.0 ** 50, 1.0, 1.0, 2.0 ** 50, -2.0 ** 100, 1.0], dtype=np.float32)
    out, _ = one_pixel(big, FeatureRecipe([("dot3", 0, 3)], 6))
    assert out[0] == 1.0
    # every product is rounded on its own: a fused multiply-add would keep the low bits
    p = np.array([1.0 + 2.0 ** -12, 1.0, 0.0, 1.0 + 2.0 ** -12, -1.0, 0.0], dtype=np.float32)
    out, _ = one_pixel(p, FeatureRecipe([("dot3", 0, 3)], 6))
    assert out[0] == f32(2.0 ** -11)                                       # not 2^-11 + 2^-24


def test_order_of_the_steps():
    """Census before the scrub, the scrub before the emitter offset, the offset
    before the normalisation, and only on its channel."""
    from nsm_amd import FeatureRecipe
    r = FeatureRecipe([0, 1, ("sub", 0, 1)], 2)
    out, census = one_pixel([np.inf, -0.0], r, scrub=True, emitter_channel=0, emitter=[2.5],
                            stats=([1.0, 0.0, 0.0], [2.0, 1.0, 1.0]), eps=0.0)
    assert census.tolist() == [0, 2, 0]                                    # Inf and Inf - -0
    assert out.tolist() == [(1.0 + 2.5 - 1.0) / 2.0, 0.0, 1.0]
    assert np.signbit(out[1])                                              # -0.0 kept: (-0 - 0) / 1
    x = U.feature_input((2, 11, 9, 13), pad_multiple=16)
    a, ca = U.compose_ref(x, U.recipe6(), 16, 16)
    b, cb = U.compose_ref(x, U.recipe6(), 16, 16, emitter_channel=5, emitter=[0.0, 2.5])
    assert np.array_equal(bits_of(a[:, :5]), bits_of(b[:, :5])) and np.array_equal(ca, cb)
    assert ca.min() > 0                                                    # every kind is met
    assert not np.array_equal(bits_of(a[1, 5]), bits_of(b[1, 5]))


# ---- 3. the C entry's checks ---------------------------------------------------------------
def test_error_path_without_gpu_work():
    """Argument validation fails before any launch, with a readable message."""
    import nsm_amd._lib as L
    keep = ctypes.create_string_buffer(64)      # never read: every call fails first
    p = ctypes.addressof(keep)
    table = (ctypes.c_int32 * 6)(0, 0, 0, 1, 0, 1)

    def compose(x=p, Cin=2, H=4, W=4, Hp=4, Wp=4, recipe=table, Cout=2, floor=1e-6, mean=None,
                std=None, echan=-1, emitter=None, out=p, part=None, report=None):
        return L.lib.nsm_feature_compose(x, 1, Cin, H, W, Hp, Wp, recipe, Cout, floor, mean, std,
                                         1e-8, 0, echan, emitter, out, part, report, None)

    cases = [
        (dict(x=None), "null"), (dict(out=None), "null"), (dict(recipe=None), "null"),
        (dict(mean=p), "mean and stdv"), (dict(part=p), "census"),
        (dict(recipe=(ctypes.c_int32 * 6)(0, 0, 0, 4, 0, 1)), "bad table"),      # op 4
        (dict(recipe=(ctypes.c_int32 * 6)(0, 2, 0, 1, 0, 1)), "bad table"),      # raw channel 2 of 2
        (dict(recipe=(ctypes.c_int32 * 6)(0, 0, 0, 1, 0, -1)), "bad table"),
        (dict(recipe=(ctypes.c_int32 * 6)(0, 0, 0, 3, 0, 0)), "bad table"),      # dot3 off the end
        (dict(echan=2, emitter=p), "emitter_channel"),                           # >= Cout
        (dict(echan=0), "emitter"), (dict(emitter=p), "emitter"),
        (dict(Cout=0), "output channels"), (dict(Cout=17), "output channels"),
        (dict(Cin=65), "raw channels"), (dict(floor=-1.0), "ratio_floor"),
        (dict(Hp=3), "padded"), (dict(Hp=8), "reflect"), (dict(Wp=8), "reflect"),
        (dict(H=1 << 15, W=1 << 15, Hp=1 << 15, Wp=1 << 15), "2\\^31"),
        (dict(x=p + 1), "unaligned"),
    ]
    import re
    for kw, word in cases:
        assert compose(**kw) == 1, kw
        assert re.search(word, L.last_error()), (kw, L.last_error())
    assert L.lib.nsm_feature_blocks(0, 4, 4) == 0 and L.lib.nsm_feature_blocks(17, 4, 4) == 0
    assert L.lib.nsm_feature_blocks(6, 0, 4) == 0
    assert L.lib.nsm_feature_blocks(16, 1 << 14, 1 << 13) == 0                   # 2^31 samples
    assert L.lib.nsm_feature_blocks(6, 1, 1) == 1
    one = L.lib.nsm_feature_blocks(1, 1088, 1920)
    assert one >= 1 and L.lib.nsm_feature_blocks(6, 1088, 1920) == one           # a thread holds Cout
