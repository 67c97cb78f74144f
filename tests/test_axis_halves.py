"""CPU tests of the row and column halves: the rule's Python mirrors cda.rows.verify_host and
assemble_host on squares extended and committed by the oracle (its codec and its wrapper tree), repairability of what
they assemble, the rule header's host form (csrc/axis_half_rule.h, run by a stand-alone program under ASan + UBSan)
against a restatement of the rule here, the C ABI of the five new calls without a device and the new kernels'
registers.  tests/test_axis_halves_gpu.py holds the device side and uses the helpers here."""
import ctypes
import functools
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from cda import _native as N
from cda import rows
from cda.rows import BAD_ROOT, CONFLICT, DUPLICATE, MALFORMED, PLACED, AxisHalf
from test_befp import OracleCodec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("cda_axis_halves_verify", "cda_axis_halves_verify_device", "cda_axis_halves_assemble_device",
             "cda_square_rebuild_axes")
KERNELS = ("axis_half_prep_kernel", "axis_half_scatter_kernel", "axis_half_combine_kernel", "axis_half_claim_kernel",
           "axis_half_place_kernel", "axis_half_gather_kernel")


class OracleRows(OracleCodec):
    """The oracle's codec and its wrapper tree, as cda.rows takes them."""

    def axis_root(self, k, index, cells):
        rc, root, _ = O.nmt_axis_root(k, index, cells)
        return root if rc == 0 else None


CODEC = OracleRows(True)


@functools.lru_cache(maxsize=None)
def block(k, seed=0x26A0):
    """An honest block by the oracle: (ods, eds, row_roots, col_roots, dah)."""
    ods = O.gen_ods(k, seed + k)
    rc, eds, rr, cr, dah = O.extend_commit(ods)
    assert rc == 0
    return ods, eds, rr, cr, bytes(dah)


def half_of(eds, k, axis, index, side, root_off=0):
    grid = eds.reshape(2 * k, 2 * k, N.SHARE_SIZE)
    line = grid[:, index] if axis else grid[index]
    return AxisHalf(axis, index, side, line[side * k:(side + 1) * k].copy(), root_off)


def axis_of(eds, k, axis, index):
    grid = eds.reshape(2 * k, 2 * k, N.SHARE_SIZE)
    return grid[:, index] if axis else grid[index]


def every_half(eds, k):
    return [half_of(eds, k, axis, index, side) for axis in (0, 1) for index in range(2 * k) for side in (0, 1)]


def flipped_half(h, cell=0, byte=100):
    shares = np.array(h.shares, np.uint8).copy()
    shares[cell, byte] ^= 0x01
    return AxisHalf(h.axis, h.index, h.side, shares, h.root_off)


def descending_half(eds, k):
    """A first half of a Q0 row with two shares swapped so that their namespaces descend."""
    for index in range(k):
        h = half_of(eds, k, 0, index, 0)
        ns = [bytes(c[:N.NAMESPACE_SIZE]) for c in h.shares]
        for j in range(k - 1):
            if ns[j] < ns[j + 1]:
                shares = h.shares.copy()
                shares[[j, j + 1]] = shares[[j + 1, j]]
                return AxisHalf(0, index, 0, shares)
    raise AssertionError("no row of Q0 with two namespaces")


def named_malformed(eds, k):
    """One descriptor per clause of H0."""
    good = half_of(eds, k, 0, 0, 0)
    return {"axis": AxisHalf(2, 0, 0, good.shares), "index": AxisHalf(1, 2 * k, 1, good.shares),
            "side": AxisHalf(0, 1 % (2 * k), 2, good.shares), "root_off": AxisHalf(0, 0, 0, good.shares, root_off=1)}


def conflict_pair(k):
    """Two ODS that differ in share (0, 0) after the namespace: row 0 of A under A's row roots, column 0 of B under
    B's column roots.  -> (row half of A, column half of B, row_roots, col_roots, eds_a, eds_b)."""
    ods_a = block(k)[0]
    ods_b = ods_a.copy()
    ods_b[0, 100] ^= 0x01
    rc_a, eds_a, rr_a, _, _ = O.extend_commit(ods_a)
    rc_b, eds_b, _, cr_b, _ = O.extend_commit(ods_b)
    assert rc_a == 0 and rc_b == 0
    return half_of(eds_a, k, 0, 0, 0), half_of(eds_b, k, 1, 0, 0), rr_a, cr_b, eds_a, eds_b


# ---- verify_host ----
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_every_half_of_every_axis_verifies(k):
    _, eds, rr, cr, _ = block(k)
    halves = every_half(eds, k)
    statuses, axes = rows.verify_host(halves, rr, cr, CODEC)
    assert statuses.tolist() == [PLACED] * (8 * k)
    for h, got in zip(halves, axes):
        assert np.array_equal(got, axis_of(eds, k, h.axis, h.index)), (h.axis, h.index, h.side)
    # cda.wrapper's tree gives the same verdicts as the oracle's
    assert rows.verify_host(halves[:4], rr, cr, OracleCodec(False))[0].tolist() == [PLACED] * 4


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_bad_halves_are_bad_root_and_malformed(k):
    _, eds, rr, cr, _ = block(k)
    w = 2 * k
    for axis, index, side in ((0, 0, 0), (0, w - 1, 1), (1, k - 1, 1), (1, k, 0)):
        h = half_of(eds, k, axis, index, side)
        assert rows.verify_host([flipped_half(h, cell=k - 1, byte=511)], rr, cr, CODEC)[0].tolist() == [BAD_ROOT]
        bad_r, bad_c = rr.copy(), cr.copy()
        (bad_c if axis else bad_r)[index, 89] ^= 0x80
        assert rows.verify_host([h], bad_r, bad_c, CODEC)[0].tolist() == [BAD_ROOT]
        # under the root of the other axis of the same index
        assert rows.verify_host([AxisHalf(1 - axis, index, side, h.shares)], rr, cr, CODEC)[0].tolist() == \
            [PLACED if np.array_equal(axis_of(eds, k, 0, index), axis_of(eds, k, 1, index)) else BAD_ROOT]
    named = named_malformed(eds, k)
    assert sorted(named) == ["axis", "index", "root_off", "side"]
    for name, h in named.items():
        statuses, axes = rows.verify_host([h], rr, cr, CODEC)
        assert statuses.tolist() == [MALFORMED] and not axes.any(), name
    if k >= 4:
        h = descending_half(eds, k)
        assert CODEC.axis_root(k, h.index, rows.complete_host(h, k, CODEC)) is None  # the push-order leg
        assert rows._axis_root(OracleCodec(True), k, h.index, rows.complete_host(h, k, CODEC)) is None
        assert rows.verify_host([h], rr, cr, CODEC)[0].tolist() == [BAD_ROOT]


# ---- assemble_host ----
def test_every_placement_status():
    k, w = 2, 4
    _, eds, rr, cr, _ = block(k)
    row1 = [half_of(eds, k, 0, 1, 0), half_of(eds, k, 0, 1, 1)]
    halves = row1 + [row1[0], half_of(eds, k, 1, 2, 1), flipped_half(half_of(eds, k, 0, 3, 0)),
                     named_malformed(eds, k)["side"]]
    got_eds, present, statuses = rows.assemble_host(halves, rr, cr, CODEC)
    assert statuses.tolist() == [PLACED, DUPLICATE, DUPLICATE, PLACED, BAD_ROOT, MALFORMED]
    want_present = np.zeros((w, w), np.uint8)
    want_present[1, :] = 1
    want_present[:, 2] = 1
    assert np.array_equal(present.reshape(w, w), want_present)
    grid = eds.reshape(w, w, N.SHARE_SIZE) * want_present[:, :, None]
    assert np.array_equal(got_eds.reshape(w, w, N.SHARE_SIZE), grid)
    # the other side first: the same square
    again = rows.assemble_host([row1[1], row1[0]], rr, cr, CODEC)
    assert again[2].tolist() == [PLACED, DUPLICATE] and again[1].sum() == w
    assert np.array_equal(again[0].reshape(w, w, -1)[1], eds.reshape(w, w, -1)[1])
    empty = rows.assemble_host([], rr, cr, CODEC)
    assert empty[0].shape == (w * w, 512) and not empty[1].any() and len(empty[2]) == 0


@pytest.mark.parametrize("k", [1, 2, 4])
def test_conflict_is_the_higher_indexed_of_a_row_and_a_column(k):
    w = 2 * k
    row_a, col_b, rr, cr, eds_a, eds_b = conflict_pair(k)
    assert rows.verify_host([row_a, col_b], rr, cr, CODEC)[0].tolist() == [PLACED, PLACED]
    for order, first_eds in (([row_a, col_b], eds_a), ([col_b, row_a], eds_b)):
        eds, present, statuses = rows.assemble_host(order, rr, cr, CODEC)
        assert statuses.tolist() == [PLACED, CONFLICT]
        assert present.sum() == 2 * w - 1
        grid = eds.reshape(w, w, N.SHARE_SIZE)
        assert np.array_equal(grid[0, 0], first_eds.reshape(w, w, -1)[0, 0])
        # the conflicting half still places the cells it owns
        assert np.array_equal(grid[0, 1:], eds_a.reshape(w, w, -1)[0, 1:])
        assert np.array_equal(grid[1:, 0], eds_b.reshape(w, w, -1)[1:, 0])


def test_shuffling_changes_nothing_but_the_order():
    k, w = 4, 8
    _, eds, rr, cr, _ = block(k)
    rng = np.random.default_rng(26)
    halves = [half_of(eds, k, int(a), int(i), int(s)) for a, i, s in
              zip(rng.integers(0, 2, 24), rng.integers(0, w, 24), rng.integers(0, 2, 24))]
    halves += [flipped_half(halves[3]), named_malformed(eds, k)["axis"]]
    base = rows.assemble_host(halves, rr, cr, CODEC)
    assert {PLACED, DUPLICATE, BAD_ROOT, MALFORMED} <= set(base[2].tolist())
    for seed in range(3):
        order = np.random.default_rng(seed).permutation(len(halves))
        eds2, present2, statuses2 = rows.assemble_host([halves[t] for t in order], rr, cr, CODEC)
        assert np.array_equal(eds2, base[0]) and np.array_equal(present2, base[1])
        # which half of an axis is PLACED and which DUPLICATE follows the order; what is verified does not
        verified = lambda s: [x in (PLACED, DUPLICATE) for x in s]  # noqa: E731
        assert verified(statuses2.tolist()) == verified(base[2][order].tolist())
        assert sorted(statuses2.tolist()) == sorted(base[2].tolist())


# ---- repairability ----
@pytest.mark.parametrize("k", [2, 4])
def test_k_axes_repair_and_fewer_rows_with_fewer_columns_do_not(k):
    _, eds, rr, cr, _ = block(k)
    w = 2 * k
    rng = np.random.default_rng(k)
    for axis in (0, 1):
        picked = rng.permutation(w)[:k]
        halves = [half_of(eds, k, axis, int(i), int(rng.integers(0, 2))) for i in picked]
        a_eds, present, statuses = rows.assemble_host(halves, rr, cr, CODEC)
        assert statuses.tolist() == [PLACED] * k and present.sum() == k * w
        rc, r_eds, r_present, _, _ = O.repair(a_eds, present, rr, cr)
        assert rc == 0 and r_present.all() and np.array_equal(r_eds, eds)
    r_rows, r_cols = rng.permutation(w)[:k - 1], rng.permutation(w)[:k - 1]
    halves = [half_of(eds, k, 0, int(i), 0) for i in r_rows] + [half_of(eds, k, 1, int(i), 1) for i in r_cols]
    a_eds, present, statuses = rows.assemble_host(halves, rr, cr, CODEC)
    assert statuses.tolist() == [PLACED] * len(halves)
    rc, r_eds, r_present, _, _ = O.repair(a_eds, present, rr, cr)
    assert rc == N.E_UNREPAIRABLE and np.array_equal(r_present, present)


# ---- the rule header against a restatement of the rule ----
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def align256(v):
    return (v + 255) & ~255


def expected_dump():
    out = []
    for k in (1, 2):
        w = 2 * k
        for asm in (0, 1):
            nroots = 4 * k if asm else 4 * k + 1
            for axis, index, side, root_off in itertools.product(range(3), range(w + 1), range(3), (0, 1, 4 * k)):
                ok = axis <= 1 and index < w and side <= 1 and root_off + 4 * k <= nroots and not (asm and root_off)
                mask = "".join(str(int(j >= k)) if ok and side == 1 else "1" for j in range(w))
                src = [j - side * k if ok and side * k <= j < side * k + k else -1 for j in range(w)]
                out.append("H %d %d %d %d %d %d : %d %d %d %s %s" % (
                    k, asm, axis, index, side, root_off, ok, index if ok else 0,
                    root_off + axis * w + index if ok else -1, mask, " ".join(map(str, src))))
    k, w = 1, 2
    for n in (1, 2, 3):
        pairs = [(p, q) for q in range(n) for p in range(q)]
        for s in range(8 ** n):
            ids = [s // 8 ** p % 8 for p in range(n)]
            descs = [(i >> 2, (i >> 1) & 1, i & 1) for i in ids]
            for v in range(1 << n):
                for e in range(1 << len(pairs)):
                    equal = {pq: bool(e >> t & 1) for t, pq in enumerate(pairs)}
                    status = [PLACED if v >> p & 1 else BAD_ROOT for p in range(n)]
                    axis_half, cell_owner = {}, [-1] * (w * w)
                    for p, (axis, index, _) in enumerate(descs):
                        if status[p] == PLACED:
                            axis_half.setdefault((axis, index), p)
                    for p, (axis, index, _) in enumerate(descs):
                        if status[p] != PLACED:
                            continue
                        if axis_half[(axis, index)] != p:
                            status[p] = DUPLICATE
                            continue
                        for pos in range(w):
                            other = axis_half.get((1 - axis, pos))
                            if other is None or p < other:
                                cell_owner[pos * w + index if axis else index * w + pos] = p
                            elif not equal[(min(p, other), max(p, other))]:
                                status[p] = CONFLICT
                    owners = [axis_half.get((a, i), -1) for a in (0, 1) for i in range(w)]
                    out.append("S %s %d %d : %s" % (" ".join(map(str, ids)), v, e,
                                                    " ".join(map(str, status + owners + cell_owner))))
    for k in (1, 2, 4, 16, 128, 512):
        for n in (0, 1, 7, 255, 256, 257):
            for asm in (0, 1):
                size = 4 * align256(8 * n) + align256(96 * n) + align256(n * 2 * k) + (align256(16 * k) if asm else 0)
                out.append("A %d %d %d %d" % (k, n, asm, size))
    out.append("axis_half_rule_dump: done")
    return out


def test_rule_header_and_workspace_under_asan_ubsan(tmp_path):
    """tests/san/axis_half_rule_dump.cpp, a stand-alone host program (hipcc as the host compiler: the headers need
    HIP's; no device code, no device), line for line against expected_dump."""
    exe = str(tmp_path / "axis_half_rule_dump")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-g", "--offload-host-only", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "san", "axis_half_rule_dump.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got, want = out.stdout.splitlines(), expected_dump()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == b
    seen = set()
    for line in want:
        if line[0] == "S":
            left, right = line.split(" : ")
            seen |= {int(x) for x in right.split()[:len(left.split()) - 3]}  # "S", the ids, v, e
    assert seen == {PLACED, DUPLICATE, CONFLICT, BAD_ROOT}


# ---- ABI ----
def test_new_calls_are_declared_and_exported(tmp_path):
    full = open(os.path.join(ROOT, "include", "cda.h")).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    L = N.lib()
    for name in NEW_CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*cda_ctx\s*\*", src), name
        assert name in N.EXPORTS and getattr(L, name).restype is ctypes.c_int
    assert re.search(r"\bint\s+cda_square_axis_halves\s*\(\s*cda_square\s*\*", src)
    assert "cda_square_axis_halves" in N.EXPORTS and L.cda_square_axis_halves.restype is ctypes.c_int
    assert re.search(r"typedef struct \{\s*uint32_t axis, index, side, root_off;\s*\} cda_axis_half_desc;", src)
    assert ctypes.sizeof(N.AxisHalfDesc) == N.AXIS_HALF_DESC_DTYPE.itemsize == 16
    assert N.AXIS_HALF_DESC_DTYPE.names == tuple(f for f, _ in N.AxisHalfDesc._fields_)
    for name, _ in N.AxisHalfDesc._fields_:
        assert getattr(N.AxisHalfDesc, name).offset == N.AXIS_HALF_DESC_DTYPE.fields[name][1]
    c = tmp_path / "sizes.c"
    c.write_text('#include "cda.h"\n#include <stdio.h>\nint main(void) { printf("%zu %d %d %d %d %d %d %d\\n", '
                 "sizeof(cda_axis_half_desc), CDA_HALF_PLACED, CDA_HALF_DUPLICATE, CDA_HALF_CONFLICT, "
                 "CDA_HALF_BAD_ROOT, CDA_HALF_MALFORMED, CDA_SIDE_FIRST, CDA_SIDE_SECOND); return 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(c)])
    assert subprocess.check_output([exe], text=True).split() == ["16", "0", "1", "2", "3", "4", "0", "1"]
    assert (N.HALF_PLACED, N.HALF_DUPLICATE, N.HALF_CONFLICT, N.HALF_BAD_ROOT, N.HALF_MALFORMED) == (0, 1, 2, 3, 4)
    assert (N.HALF_PLACED, N.HALF_DUPLICATE, N.HALF_CONFLICT, N.HALF_MALFORMED) == \
        (N.SAMPLE_PLACED, N.SAMPLE_DUPLICATE, N.SAMPLE_CONFLICT, N.SAMPLE_MALFORMED)
    assert (N.SIDE_FIRST, N.SIDE_SECOND) == (0, 1)


def test_new_calls_check_arguments_before_any_device_work():
    """Every rejection of the shape comes before the context is looked at, so it shows with no device at all."""
    L = N.lib()
    h = ctypes.c_void_p()
    V = ctypes.c_void_p

    def calls(k, n):
        yield L.cda_axis_halves_verify(None, k, n, None, None, None, 0, None, None)
        yield L.cda_axis_halves_verify_device(None, k, n, None, None, None, 0, None, None, None)
        yield L.cda_axis_halves_assemble_device(None, k, n, None, None, None, None, None, None, None)
        yield L.cda_square_rebuild_axes(None, k, n, None, None, None, None, ctypes.byref(h), None, None, None, None,
                                        None)
    for k in (0, 3, 6, 768):
        assert list(calls(k, 1)) == [N.E_NOT_POW2] * 4, k
    assert list(calls(1024, 1)) == [N.E_UNSUPPORTED] * 4     # 2k > 1024 leaves
    assert list(calls(512, 1 << 21)) == [N.E_UNSUPPORTED] * 4  # nhalves 2k = 2^31
    assert list(calls(512, (1 << 21) - 1)) == [N.E_ARG] * 4    # the null context
    assert list(calls(4, 0)) == [N.E_ARG] * 4
    assert h.value is None
    assert L.cda_square_axis_halves(None, 1, None, None, 0) == N.E_ARG
    # misaligned device pointers and null sections, still without a context to reach
    assert L.cda_axis_halves_verify_device(None, 4, 1, V(4), V(24), V(4), 16, V(4), V(16), None) == N.E_ARG
    assert L.cda_axis_halves_assemble_device(None, 4, 1, V(4), V(16), V(4), V(8), V(4), V(4), None) == N.E_ARG


# ---- registers ----
@pytest.mark.parametrize("kernel", KERNELS)
def test_axis_half_kernels_have_no_scratch(kernel, tmp_path):
    """No spilled VGPR and no private segment, read from the built library's metadata; at most 128 VGPRs."""
    import test_hash_kernel_registers as R
    if not (os.path.exists(R.V.OBJDUMP) and os.path.exists(R.READOBJ) and os.path.exists(R.LIB)):
        pytest.skip("needs llvm-objdump, llvm-readobj and the built libcda.so")
    found = {n: m for n, m in R.kernel_metadata(R.LIB, str(tmp_path)).items() if kernel in n}
    assert len(found) == 1, sorted(found)
    (name, m), = found.items()
    print(name, m)
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_count"] <= 128, m
