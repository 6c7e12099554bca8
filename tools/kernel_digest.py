#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libnsm: per kernel symbol its
resource metadata (VGPR / AGPR / SGPR counts, LDS bytes, private segment size,
spill counts) and a hash of its disassembled body. A refactor that moves
kernels between sources must leave all three identical.

    python tools/kernel_digest.py BUILD_DIR_A BUILD_DIR_B

BUILD_DIR: a directory of objects (csrc/build, or make BUILD=...). A kernel
instantiated by several objects is counted once. Exit status 1 on a difference.
"""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
        "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def run(*a):
    return subprocess.run(a, check=True, capture_output=True, text=True).stdout


def digest(build):
    """{kernel symbol: (metadata tuple, body hash)} over the objects of `build`"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(build, "*.o"))):
            fat, co = os.path.join(tmp, "fat"), os.path.join(tmp, os.path.basename(obj) + ".co")
            try:
                run(LLVM + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj)
            except subprocess.CalledProcessError:
                continue  # a source without device code
            run(LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co)
            meta = {}
            for blk in run(LLVM + "llvm-readelf", "--notes", co).split("\n  - .")[1:]:
                sym = re.search(r"\.symbol:\s+'?([^\s']+?)\.kd'?\s", blk + "\n")
                if sym:
                    meta[sym.group(1)] = tuple(
                        int(m.group(1)) if (m := re.search(r"\.%s:\s+(\d+)" % k, blk)) else 0
                        for k in META)
            dis = run(LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co)
            dis = re.sub(r"[ \t]*//.*$", "", dis, flags=re.M)  # addresses and encodings
            for m in re.finditer(r"^<(\S+)>:\n(.*?)(?=^<|^Disassembly|\Z)", dis, re.M | re.S):
                if m.group(1) in meta:
                    # without the padding up to the next function's alignment
                    body = re.sub(r"(\s*(s_nop 0|s_code_end|\.\.\.))*\s*\Z", "", m.group(2))
                    out[m.group(1)] = (meta[m.group(1)], hashlib.sha1(body.encode()).hexdigest())
            missing = set(meta) - set(out)
            assert not missing, "no disassembly for %s" % sorted(missing)[:3]
    return out


def main():
    a, b = digest(sys.argv[1]), digest(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    meta = sorted(k for k in a if k in b and a[k][0] != b[k][0])
    body = sorted(k for k in a if k in b and a[k][0] == b[k][0] and a[k][1] != b[k][1])
    print("kernels: %d / %d; only in A: %d, only in B: %d; metadata differs: %d; body differs: %d"
          % (len(a), len(b), len(only_a), len(only_b), len(meta), len(body)))
    for title, names in (("only in A", only_a), ("only in B", only_b), ("metadata", meta),
                         ("body", body)):
        for k in names:
            print("%s: %s %s" % (title, k, (a.get(k, b.get(k))[0], b.get(k, a.get(k))[0])
                                 if title == "metadata" else ""))
    return 1 if only_a or only_b or meta or body else 0


if __name__ == "__main__":
    sys.exit(main())
