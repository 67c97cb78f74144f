"""CPU tests of the blob commitment proofs: the tiling against pkg/inclusion/paths.go's vectors and the
oracle, SubtreeWalk's schedule (csrc/commitment_rule.h, dumped by a stand-alone program under ASan + UBSan) against
the recursion of cda/commitment.py, the host prover and verifier on mainnet block 408 and on synthetic squares with
every verdict of rules C0-C8, the ABI of the new calls and the verifier's workspace layout under the sanitizers.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import cda
import commitment_cases as K
import oracle_lib as O
from cda import _native as N
from cda import commitment as C
from cda import inclusion as I
from test_inclusion import COORDS, mainnet_blobs, mainnet_ods
from test_square import mainnet_txs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ---- tiles ----
@pytest.mark.parametrize("start,end,maxd,mind,want", COORDS)
def test_tiles_are_the_paths_go_coordinates(start, end, maxd, mind, want):
    """Test_calculateSubTreeRootCoordinates' cases with W = 2^(maxDepth - minDepth): the tile of size z at c is the
    coordinate (maxDepth - log2 z, c / z).  (The vectors include unaligned starts, which no blob has; the greedy rule
    answers them alike.)"""
    W = 1 << (maxd - mind)
    got = [(maxd - (z.bit_length() - 1), c // z) for c, z in C.subtree_tiles(start, end, W)]
    assert got == want


def test_tiles_equal_the_oracle_for_every_aligned_range():
    for lg in range(6):
        k = 1 << lg
        for lw in range(lg + 1):
            W = 1 << lw
            for s in range(0, k, W):
                for e in range(s + 1, k + 1):
                    tiles = C.subtree_tiles(s, e, W)
                    assert [(lg - (z.bit_length() - 1), c // z) for c, z in tiles] == \
                        O.subtree_root_coords(lg, lg - lw, s, e), (k, W, s, e)
                    assert sum(z for _, z in tiles) == e - s and tiles[0][0] == s


@pytest.mark.parametrize("threshold", [1, 2, 64])
def test_a_blobs_tiles_are_its_mountains(threshold):
    """Over the rows of every aligned blob with k <= 32 the tile sizes are MerkleMountainRangeSizes(len, W): the
    square's subtree roots are the mountains CreateCommitment hashes."""
    for k in (1, 2, 4, 8, 16, 32):
        for n in range(1, k * k + 1):
            W = I.sub_tree_width(n, threshold)
            assert W <= k
            want = I.merkle_mountain_range_sizes(n, W)
            for s in range(0, k * k - n + 1, W):
                sizes = [z for _, a, b in C.blob_rows(k, s, n) for _, z in C.subtree_tiles(a, b, W)]
                assert sizes == want, (k, s, n, W)


# ---- the walk's schedule ----
@pytest.fixture(scope="module")
def walk_dump(tmp_path_factory):
    """commitment_walk_dump under ASan + UBSan, every (k <= 64, W, s, e)."""
    exe = str(tmp_path_factory.mktemp("walk") / "commitment_walk_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(SAN, "commitment_walk_dump.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    return subprocess.run([exe, "64"], env=env, capture_output=True, text=True, check=True).stdout.splitlines()


def test_walk_schedule_equals_the_recursion(walk_dump):
    """Which subtree root and which proof node enters where: SubtreeWalk's level-by-level schedule equals nmt's
    recursion (fold_row's trace) for every case, ends at node 0 with every node used, and rejects none."""
    cases = [(k, W, s, e) for k in (1, 2, 4, 8, 16, 32, 64) for W in (1 << i for i in range(k.bit_length()))
             for s in range(0, k, W) for e in range(s + 1, k + 1)]
    assert len(walk_dump) == len(cases)
    node = bytes(29) * 2 + bytes(32)
    for line, (k, W, s, e) in zip(walk_dump, cases):
        head, tiles, roots, nodes, end = [x.strip() for x in line.split("|")]
        assert head == f"{k} {W} {s} {e}"
        want_tiles = C.subtree_tiles(s, e, W)
        assert tiles.split() == [f"T{z}@{c}" for c, z in want_tiles], line
        nn = bin(s).count("1") + bin(2 * k - e).count("1")
        trace = []
        assert C.fold_row(s, e, W, 2 * k, [node] * len(want_tiles), [node] * nn, trace) is not None, line
        want_r = sorted(f"R{i}@{lv}:{pos}" for kind, i, lv, pos in trace if kind == "R")
        want_n = sorted(f"N{i}@{lv}:{pos}" for kind, i, lv, pos in trace if kind == "N")
        assert sorted(roots.split()) == want_r and sorted(nodes.split()) == want_n, line
        assert len(want_r) == len(want_tiles) and len(want_n) == nn
        assert end == f"end 0:1:0:{nn}", line


# ---- host prover and verifier ----
def check_proof_against_oracle(sq, proof, start, n, threshold):
    """The proof's pieces are the oracle's: nmt ProveRange of each row, merkle.ProofsFromByteSlices of each row root,
    and paths.go's coordinates read out of the oracle's trees."""
    k, W = sq.k, I.sub_tree_width(n, threshold)
    lg = (2 * k).bit_length() - 1
    rows = C.blob_rows(k, start, n)
    assert len(proof.rows) == len(rows)
    assert (proof.row_proof.start_row, proof.row_proof.end_row) == (rows[0][0], rows[-1][0])
    for (row, s, e), pr, rr, mp in zip(rows, proof.rows, proof.row_proof.row_roots, proof.row_proof.proofs):
        leaves = O.axis_leaf_nodes(sq.eds, 0, row)
        assert (pr.nmt.start, pr.nmt.end) == (s, e) and pr.nmt.nodes == O.nmt_prove_range(leaves, s, e)
        coords = O.subtree_root_coords(lg - 1, lg - 1 - (W.bit_length() - 1), s, e)
        assert pr.subtree_roots == [C.tree_node(sq.row_nodes[row], 2 * k, lg - 1 - d, p) for d, p in coords]
        leaf_hash, aunts, root = O.merkle_proof(sq.roots, row)
        assert rr == sq.roots[row] and root == sq.dah
        assert (mp.total, mp.index, mp.leaf_hash, mp.aunts) == (4 * k, row, leaf_hash, aunts)


def test_block_408_blobs_verify_against_the_header():
    """Every blob of mainnet block 408: its proof from the oracle's trees verifies VALID against the header's
    data_hash and the PFB's commitment, and its subtree roots hash (the oracle's merkle root) to that commitment."""
    data_hash = mainnet_txs()[1]
    sq = K.HostSquare(mainnet_ods())
    assert sq.dah == data_hash
    blobs = mainnet_blobs()
    assert blobs
    for b in blobs:
        proof, commitment = sq.prove(b["start"], b["n"], b["ns"], 64)
        check_proof_against_oracle(sq, proof, b["start"], b["n"], 64)
        assert commitment == b["commitment"] == O.merkle_root(proof.subtree_roots())
        assert proof.verify_host(data_hash, b["commitment"], 64) == N.CP_VALID
        assert proof.verify_host(data_hash, bytes(32), 64) == N.CP_COMMITMENT
        assert proof.verify_host(bytes(32), b["commitment"], 64) == N.CP_ROW_PROOF


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_synthetic_squares_valid_proofs(k):
    """A blob of one share, one ending mid-row and one filling the square, at W = 1, 2 and k (where the square has
    room for them): built from the oracle's trees, VALID, and GetCommitment's value."""
    blobs = {(0, 1, 64), (k * k - 1, 1, 64), (0, k * k, 1), (0, k * k, 64)}  # (start, len, threshold)
    if k >= 2:
        blobs |= {(0, k + k // 2, 64), (k, k // 2, 64), (2, 2, 1), (k * k - 2, 2, 1), (1, k, 64)}
    seen_w = set()
    for start, n, threshold in sorted(blobs):
        ods, (ns,) = K.square_with_blobs(k, [(start, n)], 0x51 + start + n)
        sq = K.HostSquare(ods)
        proof, commitment = sq.prove(start, n, ns, threshold)
        check_proof_against_oracle(sq, proof, start, n, threshold)
        assert O.get_commitment(sq.eds, start, n, threshold) == (0, commitment)
        assert proof.verify_host(sq.dah, commitment, threshold) == N.CP_VALID, (k, start, n, threshold)
        seen_w.add(I.sub_tree_width(n, threshold))
    assert {1, min(2, k), k} <= seen_w


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_every_verdict_by_one_named_mutation(k):
    """Each of the nine non-zero verdicts by one named mutation of a valid proof, and of two mutations the earlier
    rule's (k = 1 has no alignment to break: W is 1)."""
    cases = K.mutation_cases(k)
    wrong = [(label, want, K.host_verdict(case)) for label, case, want in cases if K.host_verdict(case) != want]
    assert not wrong, wrong[:8]
    singles = {want for label, _, want in cases if " & " not in label}
    assert singles == set(range(10)) - ({N.CP_ALIGNMENT} if k == 1 else set())


def test_prover_rejects_what_the_rule_rejects():
    sq = K.HostSquare(O.gen_ods(4, 3))
    for start, n, threshold in [(0, 0, 64), (15, 2, 64), (0, 17, 64), (1, 2, 1), (0, 4, 0)]:
        with pytest.raises(ValueError):
            sq.prove(start, n, bytes(29), threshold)


def test_packing_refuses_sizes_the_records_cannot_hold():
    case = K.base_case(2)
    p = K.mutated(case)["proof"]
    p.rows[0].subtree_roots[0] += b"x"
    with pytest.raises(ValueError):
        C.pack_commitment_proofs([p], [0], [0], [64])
    p = K.mutated(case)["proof"]
    p.row_proof.row_roots.pop()
    with pytest.raises(ValueError):
        C.pack_commitment_proofs([p], [0], [0], [64])
    a = C.pack_commitment_proofs([case["proof"]] * 2, [0, 0], [0, 1], [64, 64])
    assert a["descs"]["row_off"].tolist() == [0, 2] and a["rows"]["root_off"].tolist() == [0, 1, 2, 3]


# ---- ABI ----
def test_new_calls_are_declared_exported_and_check_null_arguments():
    header = open(os.path.join(ROOT, "include", "cda.h")).read()
    L = cda.lib()
    for name in ("cda_commitment_proof_sizes", "cda_square_commitment_proofs", "cda_commitment_proofs_verify",
                 "cda_commitment_proofs_verify_device"):
        assert name + "(" in header and name in N.EXPORTS and hasattr(L, name)
    assert L.cda_commitment_proof_sizes(4, 64, 1, None, None, None) == N.E_ARG
    assert L.cda_square_commitment_proofs(None, 1, None, 64, 6, 1, 1, None, None, None, None, None, None, None, None,
                                          None) == N.E_ARG
    assert L.cda_commitment_proofs_verify(None, 1, None, None, None, None, 0, None, 0, None, 0, None, 0, None, 0, None,
                                          0, None) == N.E_ARG
    assert L.cda_commitment_proofs_verify_device(None, 1, None, None, None, None, 0, None, 0, None, 0, None, 0, None, 0,
                                                 None, 0, None, None) == N.E_ARG
    for i in range(10):
        name = ["VALID", "MALFORMED", "ROW_COUNT", "RANGE", "ALIGNMENT", "ROOT_COUNT", "NAMESPACE", "ROW_PROOF",
                "SUBTREE_ROOTS", "COMMITMENT"][i]
        assert getattr(N, "CP_" + name) == i and f"CDA_CP_{name} = {i}," in header


def test_proof_sizes_without_a_device():
    """cda_commitment_proof_sizes is host arithmetic: the rows and tiles of the Python mirror, CDA_E_ARG for what the
    prover rejects."""
    L = cda.lib()
    nrows, nroots = ctypes.c_uint64(), ctypes.c_uint64()
    for k in (1, 2, 4, 8):
        for threshold in (1, 2, 64):
            blobs = K.aligned_blobs(k, threshold)
            q = np.array(blobs, N.BLOB_RANGE_DTYPE)
            assert L.cda_commitment_proof_sizes(k, threshold, len(q), N._p(q), ctypes.byref(nrows),
                                                ctypes.byref(nroots)) == N.OK
            W = [I.sub_tree_width(n, threshold) for _, n in blobs]
            assert nrows.value == sum(len(C.blob_rows(k, s, n)) for s, n in blobs)
            assert nroots.value == sum(len(C.subtree_tiles(a, b, w)) for (s, n), w in zip(blobs, W)
                                       for _, a, b in C.blob_rows(k, s, n))
    for k, threshold, blob in [(4, 64, (0, 0)), (4, 64, (16, 1)), (4, 64, (10, 7)), (4, 0, (0, 1)), (4, 1, (1, 2)),
                               (4, 1, (2, 5))]:
        q = np.array([blob], N.BLOB_RANGE_DTYPE)
        assert L.cda_commitment_proof_sizes(k, threshold, 1, N._p(q), ctypes.byref(nrows),
                                            ctypes.byref(nroots)) == N.E_ARG, (k, threshold, blob)
    q = np.array([(0, 1)], N.BLOB_RANGE_DTYPE)
    assert L.cda_commitment_proof_sizes(3, 64, 1, N._p(q), ctypes.byref(nrows), ctypes.byref(nroots)) == N.E_NOT_POW2


def test_structs_match_header():
    """include/cda.h: cda_blob_range 8, cda_commitment_row 56, cda_commitment_proof_desc 60 bytes."""
    assert ctypes.sizeof(N.BlobRange) == 8 == N.BLOB_RANGE_DTYPE.itemsize
    assert ctypes.sizeof(N.CommitmentRow) == 56 == N.COMMITMENT_ROW_DTYPE.itemsize
    assert ctypes.sizeof(N.CommitmentProofDesc) == 60 == N.COMMITMENT_PROOF_DESC_DTYPE.itemsize
    for ct, dt in ((N.BlobRange, N.BLOB_RANGE_DTYPE), (N.CommitmentRow, N.COMMITMENT_ROW_DTYPE),
                   (N.CommitmentProofDesc, N.COMMITMENT_PROOF_DESC_DTYPE)):
        for name, _ in ct._fields_:
            assert getattr(ct, name).offset == dt.fields[name][1], name


def test_header_struct_sizes_by_the_compiler(tmp_path):
    """The sizes as a C compiler lays the header's structs out."""
    src = tmp_path / "sizes.c"
    src.write_text('#include "cda.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(cda_blob_range), sizeof(cda_commitment_row), sizeof(cda_commitment_proof_desc)); '
                   'return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    assert subprocess.check_output([exe], text=True).split() == ["8", "56", "60"]


@pytest.mark.parametrize("kernel", ["square_commitment_proofs_kernel", "commitment_roots_kernel",
                                    "commitment_prep_kernel", "commitment_ns_kernel", "commitment_chain_kernel",
                                    "commitment_rows_kernel", "commitment_combine_kernel"])
def test_commitment_kernels_have_no_scratch(kernel, tmp_path):
    """No spilled VGPR and no private segment, read from the built library's metadata; at most 128 VGPRs (4 waves per
    SIMD) for all but the chain kernel, which DESIGN §23 leaves at 3 waves (at most 168)."""
    import test_hash_kernel_registers as R
    if not (os.path.exists(R.V.OBJDUMP) and os.path.exists(R.READOBJ) and os.path.exists(R.LIB)):
        pytest.skip("needs llvm-objdump, llvm-readobj and the built libcda.so")
    found = {n: m for n, m in R.kernel_metadata(R.LIB, str(tmp_path)).items() if kernel in n}
    assert len(found) == 1, sorted(found)
    (name, m), = found.items()
    print(name, m)
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_count"] <= (168 if kernel == "commitment_chain_kernel" else 128), m


# ---- workspace layout ----
def test_verify_workspace_under_asan_ubsan(tmp_path):
    """commit_verify_workspace (csrc/commitment.h) bound to a heap buffer of exactly its measured size and written
    through over every slot: tests/san/commitment_arena_check.cpp, a stand-alone host program (hipcc as the host
    compiler: the header needs HIP's; no device code, no device)."""
    exe = str(tmp_path / "commitment_arena_check")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-g", "--offload-host-only", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(SAN, "commitment_arena_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "commitment_arena_check: all passed" in out.stdout
