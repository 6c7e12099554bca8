"""G-buffer feature recipes: how each network input channel is made from the
rasteriser's raw buffers (paper §3.2).

The paper's feature selection starts from the raw buffers {d, n, z, n_e, z_f,
c_e, c_c} plus four channels composed from them, z - z_f, z / z_f, c_c / d and
n . n_e, ranks everything by sensitivity, drops the weak channels and repeats.
A `FeatureRecipe` is the declarative form of one candidate set: `Cout` terms
over `Cin` raw channels,

    i or ("raw", i)      x[i], bits unchanged
    ("sub", i, j)        x[i] - x[j]
    ("ratio", i, j)      x[i] / x[j] if |x[j]| > ratio_floor, else +0.0
                         (a NaN x[j] divides and gives NaN; the scrub handles it)
    ("dot3", i, j)       ((x[i] x[j]) + (x[i+1] x[j+1])) + (x[i+2] x[j+2])

every step one fp32 IEEE operation. `compose_features` (nsm_amd/frames.py) runs
a recipe on the device in one pass (csrc/nsm_features.hip); the same recipe
feeds `FramePipeline(recipe=...)`, `dataset_stats(recipe=...)` and
`PatchSampler.from_dir(recipe=...)`, so training and inference see the same bits.

    layout = {"d": 0, "n": 1, "z": 4, "ne": 5, "zf": 8, "ce": 9, "cc": 10}
    recipe = FeatureRecipe.parse(["z", "z-zf", "z/zf", "cc/d", "n.ne", "ce"], layout)
    recipe.names         # the strings, to print beside a feature_sensitivity ranking
    recipe.table()       # int32 [Cout, 3] of (op, a, b): what the C entry takes

This module is host-only: it imports neither torch nor the HIP library.
"""
import ctypes
import re

import numpy as np

RAW, SUB, RATIO, DOT3 = 0, 1, 2, 3
OPS = ("raw", "sub", "ratio", "dot3")
MAX_OUT, MAX_IN = 16, 64
_SIGNS = {"-": "sub", "/": "ratio", ".": "dot3"}
_EXPR = re.compile(r"^\s*(\w+)\s*(?:([-/.])\s*(\w+)\s*)?$")


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _term(t, cin):
    """(op, a, b) of one term, checked against `cin` raw channels."""
    if _is_int(t):
        t = ("raw", t)
    if not isinstance(t, (tuple, list)) or not t or not isinstance(t[0], str) or t[0] not in OPS:
        raise ValueError(f"feature recipe: bad term {t!r}: a channel index or one of "
                         f"('raw', i), ('sub', i, j), ('ratio', i, j), ('dot3', i, j)")
    op = OPS.index(t[0])
    want = 2 if op == RAW else 3
    if len(t) != want or not all(_is_int(v) for v in t[1:]):
        raise ValueError(f"feature recipe: term {tuple(t)!r} takes {want - 1} integer channel "
                         f"ind{'ex' if want == 2 else 'ices'}")
    span = 3 if op == DOT3 else 1
    for v in t[1:]:
        if not 0 <= v or v + span > cin:
            what = f"channels {v}..{v + 2}" if span == 3 else f"channel {v}"
            raise ValueError(f"feature recipe: term {tuple(t)!r} reads {what}, the raw frames "
                             f"have {cin} channels")
    return (op, int(t[1]), int(t[2]) if op != RAW else 0)


class FeatureRecipe:
    """An immutable description of `out_channels` network input channels over
    `in_channels` raw ones (see the module docstring for the terms). 1 <= Cout
    <= 16, 1 <= Cin <= 64, every index in range: ValueError naming the term
    otherwise. ratio_floor: the |denominator| at or below which a ratio is +0.0.
    names: one string per term (parse() sets them to its expressions)."""

    __slots__ = ("_terms", "_cin", "_floor", "_names", "_ctable")

    def __init__(self, terms, in_channels, ratio_floor=1e-6, names=None):
        if not _is_int(in_channels) or not 1 <= in_channels <= MAX_IN:
            raise ValueError(f"feature recipe: in_channels must be an integer in [1, {MAX_IN}], "
                             f"got {in_channels!r}")
        try:
            terms = list(terms)
        except TypeError:
            raise ValueError(f"feature recipe: terms must be a sequence, got {terms!r}") from None
        if not 1 <= len(terms) <= MAX_OUT:
            raise ValueError(f"feature recipe: {len(terms)} terms; a recipe has 1 to {MAX_OUT} "
                             "output channels")
        try:
            floor = float(ratio_floor)
        except (TypeError, ValueError):
            floor = float("nan")
        floor = float(np.float32(floor)) if floor == floor else floor
        if not 0.0 <= floor < float("inf"):
            raise ValueError(f"feature recipe: ratio_floor must be a finite number >= 0, got "
                             f"{ratio_floor!r}")
        enc = tuple(_term(t, int(in_channels)) for t in terms)
        if names is not None:
            names = tuple(str(n) for n in names)
            if len(names) != len(enc):
                raise ValueError(f"feature recipe: {len(names)} names for {len(enc)} terms")
        set_ = object.__setattr__
        set_(self, "_terms", enc)
        set_(self, "_cin", int(in_channels))
        set_(self, "_floor", floor)
        set_(self, "_names", names)
        set_(self, "_ctable", (ctypes.c_int32 * (3 * len(enc)))(*[v for t in enc for v in t]))

    def __setattr__(self, name, value):
        raise AttributeError("FeatureRecipe is immutable")

    __delattr__ = __setattr__

    # ---- construction ---------------------------------------------------------------
    @classmethod
    def identity(cls, channels):
        """All-raw in order: `channels` channels in, the same out."""
        if not _is_int(channels) or not 1 <= channels <= MAX_OUT:
            raise ValueError(f"feature recipe: identity of {channels!r} channels (1 to {MAX_OUT})")
        return cls(list(range(channels)), channels)

    @classmethod
    def parse(cls, exprs, layout, in_channels=None, ratio_floor=1e-6):
        """The recipe of expressions over named buffers: "z" (raw), "z-zf",
        "z/zf", "n.ne" (dot3). layout maps a name to its channel, a vector name
        to its first one. in_channels: the raw channel count (None: the highest
        channel of the layout + 1, a vector's last component not known to it).
        The strings become `names`."""
        if isinstance(exprs, str):
            raise ValueError("feature recipe: parse takes a list of expressions, got a string")
        exprs = [e for e in exprs]
        terms = []
        for e in exprs:
            m = _EXPR.match(e) if isinstance(e, str) else None
            if m is None:
                raise ValueError(f"feature recipe: cannot parse {e!r}: a name, or two names joined "
                                 "by '-', '/' or '.'")
            a, sign, b = m.groups()
            for n in (a, b):
                if n is not None and n not in layout:
                    raise ValueError(f"feature recipe: {e!r} names {n!r}, the layout has "
                                     f"{sorted(layout)}")
            terms.append(("raw", layout[a]) if sign is None else (_SIGNS[sign], layout[a], layout[b]))
        if in_channels is None:
            in_channels = max(int(v) for v in layout.values()) + 1
        return cls(terms, in_channels, ratio_floor, names=exprs)

    # ---- what it holds -----------------------------------------------------------------
    @property
    def in_channels(self):
        return self._cin

    @property
    def out_channels(self):
        return len(self._terms)

    @property
    def ratio_floor(self):
        return self._floor

    @property
    def names(self):
        return self._names

    @property
    def terms(self):
        """The terms in the explicit form: ("raw", i) or (op, i, j)."""
        return tuple((OPS[op], a) if op == RAW else (OPS[op], a, b) for op, a, b in self._terms)

    def table(self):
        """int32 [Cout, 3] of (op, a, b), RAW=0 SUB=1 RATIO=2 DOT3=3 (b of a raw term: 0)."""
        return np.array(self._terms, dtype=np.int32).reshape(-1, 3)

    def planes_read(self):
        """The raw channels some term reads, sorted."""
        used = set()
        for op, a, b in self._terms:
            span = 3 if op == DOT3 else 1
            used.update(range(a, a + span))
            if op != RAW:
                used.update(range(b, b + span))
        return sorted(used)

    def check_input(self, channels, what="feature recipe"):
        """ValueError unless frames of `channels` raw channels are this recipe's input."""
        if channels != self._cin:
            raise ValueError(f"{what}: the recipe is over {self._cin} raw channels, the frames "
                             f"have {channels}")

    def __eq__(self, other):
        return (isinstance(other, FeatureRecipe) and self._terms == other._terms
                and self._cin == other._cin and self._floor == other._floor)

    def __hash__(self):
        return hash((self._terms, self._cin, self._floor))

    def __repr__(self):
        return (f"FeatureRecipe({list(self.terms)!r}, in_channels={self._cin}, "
                f"ratio_floor={self._floor!r})")
