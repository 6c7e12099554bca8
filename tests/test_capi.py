"""CPU: the C-ABI library loads and exports every entry point include/nsm.h
declares; host-side helpers (fast division, tile/workspace planning)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nsm.h")
LIB = os.path.join(ROOT, "pcss-unet_amd", "nsm_amd", "libnsm.so")


def declared_symbols():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nsm_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(LIB)
    syms = declared_symbols()
    assert len(syms) >= 30
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing


def test_python_binding_covers_header():
    import nsm_amd._lib as L
    assert sorted(L.symbols()) == declared_symbols()
    assert L.lib.nsm_version() == 1


def test_error_path_without_gpu_work():
    """Argument validation fails before any launch, with a readable message."""
    import nsm_amd._lib as L
    rc = L.lib.nsm_conv_fwd(None, 0, 1, 1, 1, 32, None, None, 32, 3, None, 32, None, None, None,
                            0.2, None)
    assert rc == 1
    assert "null" in L.last_error()


P1 = 4096    # a non-null pointer that is never dereferenced: the checks come first

# (entry, its name in messages, index of the dtype argument, otherwise valid arguments):
# one entry per source that turns a dtype code into an element type (nsm_vgg.hip
# is fp32 only and has none), plus a resample entry whose whole body is typed
BAD_DTYPE = [
    ("nsm_bn_stats", "bn_stats", 6, [P1, 8, 64, 8, P1, None, 7, None]),
    ("nsm_avgpool2_fwd", "avgpool2_fwd", 6, [P1, 1, 4, 4, 8, P1, 7, None]),
    ("nsm_resize_bwd", "resize_bwd", 8, [P1, 1, 4, 4, 8, P1, 8, 8, 7, None]),
    ("nsm_head_fwd", "head_fwd", 8, [P1, 16, 1, 4, 4, P1, P1, P1, 7, None]),
    ("nsm_nchw_to_nhwc", "nchw_to_nhwc", 8, [P1, 1, 3, 4, 4, P1, 8, 8, 7, None]),
    ("nsm_conv_fwd_act", "conv_fwd_act", 17,
     [P1, 32, 1, 8, 8, 32, P1, P1, 32, 3, P1, 32, P1, P1, 0.2, None, 0, 7, None]),
]


@pytest.mark.parametrize("entry,name,at,args", BAD_DTYPE, ids=[c[0] for c in BAD_DTYPE])
def test_unknown_dtype_code_is_an_argument_error(entry, name, at, args):
    """A dtype code other than NSM_F32 / NSM_BF16 / NSM_F16 is NSM_E_ARG (1) with
    a message naming the entry and the code; nothing is launched (no GPU is
    needed, and the pointers are never read)."""
    import nsm_amd._lib as L
    args = list(args)
    assert args[at] == 7
    if entry == "nsm_bn_stats":
        args[5] = L.lib.nsm_reduce_chunks(args[2], args[3])
    assert getattr(L.lib, entry)(*args) == 1
    msg = L.last_error()
    assert name in msg and "dtype code 7" in msg, msg


def test_wgrad_workspace_plan():
    import nsm_amd._lib as L
    # conv6 3x3 at B=8, 64x64: M=1024, N=9216
    n = L.lib.nsm_conv_wgrad_ws(8, 64, 64, 1024, 1024, 3)
    assert n % (1024 * 9216) == 0 and n >= 1024 * 9216
    assert L.lib.nsm_reduce_chunks(524288, 32) >= 1


def fastdiv(n, d):
    """Python replica of nsm::make_fastdiv / fdiv (nsm_common.h)."""
    if d <= 1:
        return n
    l = (d - 1).bit_length()
    p = 31 + l
    mul = ((1 << p) + d - 1) // d
    return ((n * mul) >> 32) >> (p - 32)


def test_fastdiv_exact():
    rng = np.random.default_rng(0)
    for d in list(range(1, 300)) + [540, 960, 1080, 1920, 65536, 262144, 1 << 20]:
        ns = list(range(0, 2000)) + [int(v) for v in rng.integers(0, 2**31, 2000)] + [2**31 - 1]
        for n in ns:
            assert fastdiv(n, d) == n // d, (n, d)


def test_tail_plan_blocks_never_straddle_parameters():
    """nsm_tail_plan (host): blocks of nsm_tail_chunk() elements, one parameter
    each, covering the flat buffer in order."""
    import nsm_amd._lib as L
    sizes = [1728, 16, 512, 37, 9000, 4, 1, 9, 9437184]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    seg_off = (ctypes.c_int64 * len(offs))(*offs.tolist())
    nseg = len(sizes)
    nblk = L.lib.nsm_tail_plan(seg_off, nseg, None, None, None, None, 0)
    ch = L.lib.nsm_tail_chunk()
    assert nblk == sum(-(-s // ch) for s in sizes)
    bs, lo, hi = (ctypes.c_int * nblk)(), (ctypes.c_int64 * nblk)(), (ctypes.c_int64 * nblk)()
    sb = (ctypes.c_int * (nseg + 1))()
    assert L.lib.nsm_tail_plan(seg_off, nseg, bs, lo, hi, sb, nblk) == nblk
    assert lo[0] == 0 and hi[nblk - 1] == offs[-1]
    for b in range(nblk):
        s = bs[b]
        assert offs[s] <= lo[b] < hi[b] <= offs[s + 1] and hi[b] - lo[b] <= ch
        if b:
            assert lo[b] == hi[b - 1]
    assert [sb[s] for s in range(nseg + 1)] == [0] + list(np.cumsum([-(-s // ch) for s in sizes]))
    assert L.lib.nsm_tail_ws_bytes(nseg, nblk) > 0
