"""Register and LDS budget of small_square_kernel (csrc/small_square_kernels.hip), read from the built libcda.so (CPU
only), in the manner of test_hash_kernel_registers.py.

The kernel runs a whole k <= 8 square in one 256-thread workgroup.  Its budget: at most 128 VGPRs (4 waves per SIMD, the
limit the other hash kernels are held to), no spilled VGPR and no private segment, and at most 80 KiB of LDS, static
plus what the launcher asks for, which is half of a CU's 160 KiB, so that two blocks share a CU.  The launcher's figure
is csrc/mixed_route.h's small_square_lds_bytes, asked of tests/san/mixed_route_dump.cpp."""
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
KERNEL = "small_square_kernel"
LDS_BUDGET = 80 * 1024

pytestmark = pytest.mark.skipif(not (os.path.exists(V.OBJDUMP) and os.path.exists(READOBJ) and os.path.exists(LIB)),
                                reason="needs llvm-objdump, llvm-readobj and the built libcda.so")

KEY = re.compile(r"^\s*(?:- )?\.(name|symbol|vgpr_count|vgpr_spill_count|private_segment_fixed_size|"
                 r"group_segment_fixed_size|max_flat_workgroup_size):\s*(\S+)")


def kernels(lib, tmp):
    """[{key: value}] for every kernel whose name holds KERNEL, from the amdhsa.kernels notes of the code objects."""
    found = []
    for co in V.code_objects(lib, tmp):
        text = subprocess.run([READOBJ, "--notes", co], capture_output=True, text=True, check=True).stdout
        # one kernel's map runs from its .args (or first key) to its .wavefront_size; split on the latter
        for chunk in text.split(".wavefront_size:"):
            cur = {}
            for ln in chunk.splitlines():
                m = KEY.match(ln)
                if m:
                    cur[m.group(1)] = m.group(2).strip("'\"")  # an argument's .name comes first: overwritten
            if KERNEL in cur.get("symbol", "") and "vgpr_count" in cur:
                found.append(cur)
    return found


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    return kernels(LIB, str(tmp_path_factory.mktemp("co")))


@pytest.fixture(scope="module")
def launcher_lds(tmp_path_factory):
    """The dynamic LDS the launcher requests for a launch whose largest block has k = 1, 2, 4, 8."""
    exe = str(tmp_path_factory.mktemp("mixed_route") / "mixed_route_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "san", "mixed_route_dump.cpp")])
    out = {}
    for k in (1, 2, 4, 8):
        text = subprocess.run([exe, "8", str(k)], capture_output=True, text=True, check=True, timeout=60).stdout
        (line,) = [ln.split() for ln in text.splitlines() if ln.startswith("lds ")]
        assert int(line[1]) == k
        out[k] = int(line[2])
    return out


def test_kernel_appears_once(meta):
    assert len(meta) == 1, meta


def test_four_waves_per_simd_without_spills(meta):
    (m,) = meta
    print(m)
    assert int(m["vgpr_count"]) <= 128, m
    assert int(m["vgpr_spill_count"]) == 0, m
    assert int(m["private_segment_fixed_size"]) == 0, m
    assert int(m["max_flat_workgroup_size"]) == 256, m


def test_two_blocks_share_a_cu(meta, launcher_lds):
    (m,) = meta
    static = int(m["group_segment_fixed_size"])
    print("static LDS", static, "dynamic by kmax", launcher_lds)
    for k, dyn in launcher_lds.items():
        assert static + dyn <= LDS_BUDGET, (k, static, dyn)
    assert launcher_lds[8] >= 2048 + 1024 * 64  # the matrices and both codec states of a k = 8 block
