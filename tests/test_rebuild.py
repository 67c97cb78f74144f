"""CPU tests of a square rebuilt from proved samples: the placement rule's Python mirror
cda.sampling.assemble_host on squares committed by the oracle's trees, cda.befp.from_samples, and the C ABI of the three
new calls without a device.  tests/test_rebuild_gpu.py holds the device side and uses the helpers here."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

import oracle_lib as O
from cda import _native as N
from cda import befp, sampling
from cda.proof import NMTProof
from cda.sampling import CONFLICT, DUPLICATE, MALFORMED, PLACED, REJECTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("cda_samples_assemble_device", "cda_square_open_eds_device", "cda_square_rebuild")


class OracleSquare:
    """A 2k x 2k square as a producer committed it, by the oracle (ora_roots, ora_axis_leaf_nodes,
    ora_nmt_prove_range): the row trees over `eds`, the column trees over `col_eds` (default: the same bytes).  Two
    squares that differ in one cell commit that cell differently in its row tree and its column tree, and every
    sample still verifies against the root of its own tree."""

    def __init__(self, eds, k, col_eds=None):
        self.k, self.w = k, 2 * k
        self.eds = {0: np.ascontiguousarray(eds, np.uint8), 1: np.ascontiguousarray(eds if col_eds is None else col_eds)}
        rc0, self.row_roots, _, _, _ = O.roots(self.eds[0])
        rc1, _, self.col_roots, _, _ = O.roots(self.eds[1])
        assert rc0 == 0 and rc1 == 0
        self._leaves = {}

    def cell(self, axis, index, pos):
        grid = self.eds[axis].reshape(self.w, self.w, N.SHARE_SIZE)
        return (grid[pos, index] if axis else grid[index, pos]).tobytes()

    def sample(self, axis, index, pos):
        """(axis, index, pos, share, NMTProof): leaf `pos` of row (axis 0) or column (axis 1) `index`."""
        key = (axis, index)
        if key not in self._leaves:
            self._leaves[key] = O.axis_leaf_nodes(self.eds[axis], axis, index)
        return (axis, index, pos, self.cell(axis, index, pos),
                NMTProof(pos, pos + 1, O.nmt_prove_range(self._leaves[key], pos, pos + 1)))

    def every_cell_twice(self):
        return [self.sample(axis, i, j) for axis in (0, 1) for i in range(self.w) for j in range(self.w)]


def cell_of(sample, w):
    axis, index, pos = sample[:3]
    return pos * w + index if axis else index * w + pos


def flipped(share, byte=100):
    return share[:byte] + bytes([share[byte] ^ 0x01]) + share[byte + 1:]


def two_tree_square(k, seed, row, col):
    """An honest square whose column tree `col` commits other bytes in cell (row, col) than its row tree does."""
    eds = O.extend(O.gen_ods(k, seed))
    other = eds.copy()
    other.reshape(2 * k, 2 * k, N.SHARE_SIZE)[row, col, 100] ^= 0x01
    return OracleSquare(eds, k, col_eds=other)


def expected_by_construction(samples, kinds, w):
    """What the rule says, from how the test made each sample (kinds[p]: "good", REJECTED or MALFORMED), without a
    hash: -> (eds, present, statuses)."""
    eds = np.zeros((w * w, N.SHARE_SIZE), np.uint8)
    present = np.zeros(w * w, np.uint8)
    statuses = np.zeros(len(samples), np.uint8)
    placed = {}
    for p, (s, kind) in enumerate(zip(samples, kinds)):
        if kind != "good":
            statuses[p] = kind
            continue
        cell = cell_of(s, w)
        if cell in placed:
            statuses[p] = DUPLICATE if placed[cell] == s[3] else CONFLICT
            continue
        placed[cell] = s[3]
        eds[cell] = np.frombuffer(s[3], np.uint8)
        present[cell] = 1
        statuses[p] = PLACED
    return eds, present, statuses


def test_assemble_host_every_status():
    """k = 2: every cell by its row and by its column proof, shuffled; cell (1, 2) is committed differently by its two
    trees; then one more sample of each status that is not PLACED."""
    k, w = 2, 4
    sq = two_tree_square(k, 0x22B0, 1, 2)
    samples = sq.every_cell_twice()
    rng = np.random.default_rng(22)
    samples = [samples[i] for i in rng.permutation(len(samples))]
    kinds = ["good"] * len(samples)
    first = {}
    for s in samples:
        first.setdefault(cell_of(s, w), s)
    dup = sq.sample(0, 3, 3)
    conflict_cell = first[1 * w + 2]
    other = sq.sample(1 - conflict_cell[0], *((2, 1) if conflict_cell[0] == 0 else (1, 2)))
    assert cell_of(other, w) == 1 * w + 2 and other[3] != conflict_cell[3]
    a, i, j, share, proof = sq.sample(1, 0, 1)
    extras = [(dup, "good"), (other, "good"), ((a, i, j, flipped(share), proof), REJECTED),
              ((2, i, j, share, proof), MALFORMED)]
    samples += [s for s, _ in extras]
    kinds += [kd for _, kd in extras]
    want_eds, want_present, want = expected_by_construction(samples, kinds, w)
    assert want[-4:].tolist() == [DUPLICATE, CONFLICT, REJECTED, MALFORMED]
    assert sorted(want[:32].tolist()) == [PLACED] * 16 + [DUPLICATE] * 15 + [CONFLICT]
    eds, present, statuses = sampling.assemble_host(samples, sq.row_roots, sq.col_roots)
    assert statuses.tolist() == want.tolist()
    assert present.tolist() == [1] * 16 and np.array_equal(present, want_present)
    assert np.array_equal(eds, want_eds)
    # all but the contested cell are the square's own bytes; that one is its first sample's
    grid = sq.eds[0].copy()
    grid[1 * w + 2] = np.frombuffer(conflict_cell[3], np.uint8)
    assert np.array_equal(eds, grid)


def test_assemble_host_rejections_and_empty():
    k, w = 2, 4
    sq = OracleSquare(O.extend(O.gen_ods(k, 0x22B1)), k)
    a, i, j, share, proof = sq.sample(0, 1, 2)
    bad = [(a, (i + 1) % w, j, share, proof),                      # under the wrong root
           (a, i, j, share, NMTProof(j, j + 1, proof.nodes[:-1])),  # a node short
           (a, w, j, share, proof), (a, i, w, share, proof), (-1, i, j, share, proof)]
    eds, present, statuses = sampling.assemble_host(bad, sq.row_roots, sq.col_roots)
    assert statuses.tolist() == [REJECTED, REJECTED, MALFORMED, MALFORMED, MALFORMED]
    assert not present.any() and not eds.any()
    eds, present, statuses = sampling.assemble_host([], sq.row_roots, sq.col_roots)
    assert eds.shape == (16, 512) and not present.any() and len(statuses) == 0
    # the proof's own range is not believed: the leaf is [pos, pos + 1) by the rule
    lying = (a, i, j + 1, share, NMTProof(j, j + 1, proof.nodes))
    assert sampling.assemble_host([lying], sq.row_roots, sq.col_roots)[2].tolist() == [REJECTED]


def test_befp_from_samples_on_a_badly_encoded_square():
    """k = 4, one Q1 cell altered before commitment (the oracle's trees): the row through it is FRAUD by the samples a
    node holds; k - 1 usable samples are not a proof."""
    from test_befp import CODECS
    k, w = 4, 8
    row, col = 2, 5
    bad = O.extend(O.gen_ods(k, 0x22B2))
    bad.reshape(w, w, N.SHARE_SIZE)[row, col, 7] ^= 0x10
    sq = OracleSquare(bad, k)
    samples = sq.every_cell_twice()
    rng = np.random.default_rng(44)
    shuffled = [samples[i] for i in rng.permutation(len(samples))]
    shuffled += shuffled[:40]  # duplicates
    for axis, index in ((0, row), (1, col)):
        proof = befp.from_samples(shuffled, axis, index, k)
        assert (proof.axis, proof.index) == (axis, index)
        assert [p for p, _, _ in proof.shares] == list(range(w))
        for pos, share, nmt in proof.shares:
            assert share == sq.cell(axis, index, pos) and (nmt.start, nmt.end) == (index, index + 1)
        for codec in CODECS.values():
            assert befp.validate_host(proof, sq.row_roots, sq.col_roots, codec=codec) == befp.FRAUD
    honest = befp.from_samples(shuffled, 0, row + 1, k)
    assert befp.validate_host(honest, sq.row_roots, sq.col_roots, codec=CODECS["leopard"]) == befp.NO_FRAUD
    # the row's own proofs are of no use to its fraud proof; k - 1 column proofs are too few, k are enough
    own = [sq.sample(0, row, j) for j in range(w)]
    few = [sq.sample(1, j, row) for j in (6, 1, 3)]
    assert befp.from_samples(own + few + few, 0, row, k) is None
    assert befp.from_samples(own, 0, row, k) is None
    enough = befp.from_samples(own + few + [sq.sample(1, 4, row)], 0, row, k)
    assert [p for p, _, _ in enough.shares] == [1, 3, 4, 6]
    assert befp.validate_host(enough, sq.row_roots, sq.col_roots, codec=CODECS["leopard"]) == befp.FRAUD


def test_new_calls_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "cda.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = N.lib()
    for name in NEW_CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*cda_ctx\s*\*", src), name
        assert name in N.EXPORTS
        assert getattr(L, name).restype is ctypes.c_int
    assert re.search(r"typedef struct \{\s*uint32_t axis, index, pos, node_off, nnodes;\s*\} cda_sample_desc;", src)
    assert ctypes.sizeof(N.SampleDesc) == N.SAMPLE_DESC_DTYPE.itemsize == 20
    assert N.SAMPLE_DESC_DTYPE.names == tuple(f for f, _ in N.SampleDesc._fields_)
    full = open(os.path.join(ROOT, "include", "cda.h")).read()
    for name in ("PLACED", "DUPLICATE", "CONFLICT", "REJECTED", "MALFORMED"):
        assert f"#define CDA_SAMPLE_{name} {getattr(N, 'SAMPLE_' + name)} " in full
    assert len({PLACED, DUPLICATE, CONFLICT, REJECTED, MALFORMED}) == 5


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_assemble_workspace_and_rule_under_asan_ubsan(tmp_path):
    """The layout of the assemble workspace (csrc/rebuild.h) bound to a heap buffer of exactly its measured size and
    written the way the kernels index it, through csrc/sample_place_rule.h: tests/san/rebuild_arena_check.cpp, a
    stand-alone host program (hipcc as the host compiler: the header needs HIP's; no device code, no device)."""
    exe = str(tmp_path / "rebuild_arena_check")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-g", "--offload-host-only", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "san", "rebuild_arena_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rebuild_arena_check: all passed" in out.stdout


def test_new_calls_check_arguments_before_any_device_work():
    L = N.lib()
    h = ctypes.c_void_p()
    assert L.cda_samples_assemble_device(None, 4, 0, None, None, None, 0, None, None, None, None, None) == N.E_ARG
    assert L.cda_square_open_eds_device(None, 4, None, ctypes.byref(h), None, None, None, None, None) == N.E_ARG
    assert L.cda_square_rebuild(None, 4, 0, None, None, None, 0, None, None, ctypes.byref(h), None, None, None, None,
                                None) == N.E_ARG
    assert h.value is None
