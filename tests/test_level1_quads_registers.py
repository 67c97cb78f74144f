"""Register budget of nmt_level1_quads_kernel, read from the built libcda.so (CPU only): four level-1 nodes per thread,
with a chaining state kept across them, must still run 4 waves per SIMD (vgpr_count <= 128) with no spilled VGPR and
no private segment.  (With both block-2 schedules of the parity form's row-top / col-left pair in registers at once
the kernel spilled 44 VGPRs.)  Metadata reader and skip condition: test_hash_kernel_registers.py."""
import pytest

from test_hash_kernel_registers import LIB, kernel_metadata, pytestmark  # noqa: F401


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    return kernel_metadata(LIB, str(tmp_path_factory.mktemp("co")))


def test_quads_kernel_four_waves_per_simd_without_spills(meta):
    found = {n: m for n, m in meta.items() if "nmt_level1_quads_kernel" in n}
    assert len(found) == 1, sorted(meta)
    (name, m), = found.items()
    print(name, m)
    assert m["vgpr_count"] <= 128, m
    assert m["vgpr_spill_count"] == 0, m
    assert m["private_segment_fixed_size"] == 0, m
