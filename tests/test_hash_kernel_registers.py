"""Register budget of the two hash kernels that carry the step, read from the built libcda.so (CPU only).

gfx950 has 512 VGPRs per SIMD lane: a kernel of at most 128 runs 4 waves per SIMD, one of 129..168 only 3.  The leaf
kernel once went from 119 to 144 unnoticed (a second copy of block 0's rounds for the parity midstate), so the
numbers the compiler recorded in the code object's metadata are asserted here: vgpr_count <= 128, no spilled VGPR
and no private segment (scratch).  SGPR spills are not counted: they go to lanes of a VGPR that vgpr_count already
includes and touch no memory."""
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import vmcnt_check as V  # noqa: E402

LIB = os.path.join(ROOT, "celestia-app_amd", "cda", "libcda.so")
READOBJ = os.path.join(os.path.dirname(V.OBJDUMP), "llvm-readobj")

pytestmark = pytest.mark.skipif(not (os.path.exists(V.OBJDUMP) and os.path.exists(READOBJ) and os.path.exists(LIB)),
                                reason="needs llvm-objdump, llvm-readobj and the built libcda.so")

KEY = re.compile(r"^\s*(?:- )?\.(name|vgpr_count|vgpr_spill_count|private_segment_fixed_size|wavefront_size):\s*(\S+)")


def kernel_metadata(lib, tmp):
    """{kernel name: {key: int}} from the amdhsa.kernels notes of every gfx950 code object in lib."""
    out = {}
    for co in V.code_objects(lib, tmp):
        text = subprocess.run([READOBJ, "--notes", co], capture_output=True, text=True, check=True).stdout
        cur = {}
        for ln in text.splitlines():
            m = KEY.match(ln)
            if not m:
                continue
            key, val = m.groups()
            if key == "wavefront_size":  # the last key of a kernel's map (keys are sorted)
                if "vgpr_count" in cur:
                    out[cur["name"]] = {k: int(v) for k, v in cur.items() if k != "name"}
                cur = {}
            elif key != "name" or "private_segment_fixed_size" not in cur:
                cur[key] = val.strip("'\"")  # an argument's .name precedes the kernel's own keys: overwritten
    return out


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    return kernel_metadata(LIB, str(tmp_path_factory.mktemp("co")))


@pytest.mark.parametrize("kernel", ["leaf_hash_kernel", "nmt_levels_kernel"])
def test_four_waves_per_simd_without_spills(meta, kernel):
    found = {n: m for n, m in meta.items() if kernel in n}
    assert len(found) == 1, sorted(meta)
    (name, m), = found.items()
    print(name, m)
    assert m["vgpr_count"] <= 128, m
    assert m["vgpr_spill_count"] == 0, m
    assert m["private_segment_fixed_size"] == 0, m
