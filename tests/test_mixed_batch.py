"""CPU tests of the mixed-size batch (cda_extend_commit_mixed): the pure routing header csrc/mixed_route.h, asked of
tests/san/mixed_route_dump.cpp (a stand-alone host program built with the plain C++ compiler under ASan + UBSan, as
codec_shape_dump.cpp is), the Python offsets helper, and the argument checks of both entry points, which run before
any device work."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cda
from cda import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 8, 2, 2, 16, 4, 1, 8, 32, 4, 16, 1]
# written out by hand: the blocks' first share (k^2 shares each) and first root (2k each), then the totals
ODS_SHARES = [0, 1, 65, 69, 73, 329, 345, 346, 410, 1434, 1450, 1706, 1707]
ROOTS = [0, 2, 18, 22, 26, 58, 66, 68, 84, 148, 156, 188, 190]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mixed_route") / "mixed_route_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "san", "mixed_route_dump.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")

    def run(small_max, ks):
        out = subprocess.run([exe, str(small_max), *map(str, ks)], env=env, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        got = {}
        for line in out.stdout.splitlines():
            f = line.split()
            got.setdefault(f[0], []).append([int(x) for x in f[1:] if x != ":"])
        return got
    return run


EXPECT = {
    0: dict(small=[],
            groups=[[1, 0, 6, 11], [2, 2, 3], [4, 5, 9], [8, 1, 7], [16, 4, 10], [32, 8]],
            runs=[[1, 0, 1], [8, 1, 1], [2, 2, 2], [16, 4, 1], [4, 5, 1], [1, 6, 1], [8, 7, 1], [32, 8, 1], [4, 9, 1],
                  [16, 10, 1], [1, 11, 1]]),
    4: dict(small=[0, 2, 3, 5, 6, 9, 11],
            groups=[[8, 1, 7], [16, 4, 10], [32, 8]],
            runs=[[8, 1, 1], [16, 4, 1], [8, 7, 1], [32, 8, 1], [16, 10, 1]]),
    8: dict(small=[0, 1, 2, 3, 5, 6, 7, 9, 11],
            groups=[[16, 4, 10], [32, 8]],
            runs=[[16, 4, 1], [32, 8, 1], [16, 10, 1]]),
}


@pytest.mark.parametrize("small_max", [0, 4, 8])
def test_routing_header(dump, small_max):
    got = dump(small_max, KS)
    want = EXPECT[small_max]
    assert got["check"] == [[0, 0]]
    assert got["ods"] == [[s * 512 for s in ODS_SHARES]]
    assert got["eds"] == [[4 * s * 512 for s in ODS_SHARES]]
    assert got["roots"] == [ROOTS]
    assert got["small"] == [want["small"]]
    assert got.get("group", []) == want["groups"]
    assert got.get("run", []) == want["runs"]
    # a descriptor per small block: log2 k, the block, its packed ODS / EDS bytes and its first 96-B record (4k each)
    assert got.get("desc", []) == [[KS[b].bit_length() - 1, b, ODS_SHARES[b] * 512, 4 * ODS_SHARES[b] * 512, 2 * ROOTS[b]]
                                   for b in want["small"]]
    if want["small"]:
        kmax = max(KS[b] for b in want["small"])
        (k, lds), = got["lds"]
        assert k == kmax and lds == 2048 + max(1024 * kmax * kmax, 18944) and lds <= 80 * 1024
    else:
        assert "lds" not in got


def test_routing_header_runs_join_neighbours_only(dump):
    """Equal sizes side by side are one run; a small block between two ends it (the run is one contiguous range)."""
    got = dump(4, [16, 16, 2, 16, 8, 8, 8])
    assert got["run"] == [[16, 0, 2], [16, 3, 1], [8, 4, 3]]
    assert got["group"] == [[8, 4, 5, 6], [16, 0, 1, 3]]


def test_routing_header_argument_check(dump):
    assert dump(8, [2, 3, 4])["check"] == [[1, 1]]
    assert dump(8, [2, 0, 3])["check"] == [[1, 1]]
    assert dump(8, [2, 1024, 4, 2048])["check"] == [[2, 1]]
    assert dump(8, [1024, 3])["check"] == [[1, 1]]  # the power-of-two check comes first, as in the single-size calls


def test_python_offsets_helper():
    off = N.mixed_offsets(KS)
    assert off["ods"].tolist() == [s * 512 for s in ODS_SHARES]
    assert off["eds"].tolist() == [4 * s * 512 for s in ODS_SHARES]
    assert off["roots"].tolist() == ROOTS
    assert off["recs"].tolist() == [2 * r for r in ROOTS]
    small = N.mixed_offsets([2, 1])
    assert small["ods"].tolist() == [0, 2048, 2560] and small["recs"].tolist() == [0, 8, 12]


def test_entry_points_check_arguments_without_gpu():
    L = cda.lib()
    ks = (ctypes.c_uint32 * 3)(2, 3, 4)
    err = N.ErrInfo()
    assert L.cda_extend_commit_mixed(None, 3, ks, None, None, None, None, None, ctypes.byref(err)) == N.E_ARG
    assert L.cda_extend_commit_mixed_device(None, 3, ks, None, None, None, None, None, None) == N.E_ARG
    assert L.cda_set_option(None, N.OPT_MIXED_SMALL_MAX, 4) == N.E_ARG


def test_not_pow2_names_the_block_without_gpu():
    """ks is checked before the context is used: a context handle that is never dereferenced stands in for one (the
    build container has no GPU to make a real one), with every buffer non-null."""
    L = cda.lib()
    ks = (ctypes.c_uint32 * 3)(2, 3, 4)
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    err = N.ErrInfo()
    assert L.cda_extend_commit_mixed(p, 3, ks, p, None, p, p, p, ctypes.byref(err)) == N.E_NOT_POW2
    assert (err.code, err.block) == (N.E_NOT_POW2, 1)
    assert L.cda_extend_commit_mixed_device(p, 3, ks, p, p, p, p, p, None) == N.E_NOT_POW2
    big = (ctypes.c_uint32 * 3)(2, 4, 1024)
    assert L.cda_extend_commit_mixed(p, 3, big, p, None, p, p, p, ctypes.byref(err)) == N.E_UNSUPPORTED
    assert (err.code, err.block) == (N.E_UNSUPPORTED, 2)
    assert L.cda_extend_commit_mixed(p, 0, ks, p, None, p, p, p, ctypes.byref(err)) == N.E_ARG
    assert L.cda_extend_commit_mixed(p, 3, None, p, None, p, p, p, ctypes.byref(err)) == N.E_ARG
