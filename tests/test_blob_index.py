"""CPU tests of reading a square back: the rule's Python mirror (cda.blob.index_host) on mainnet block
408, the round trip txs -> square.construct -> parse_txs, the rule header's host form (csrc/share_index_rule.h, run by
a stand-alone program under ASan + UBSan over every k = 2 square of an alphabet of share headers) against the mirror,
and the ABI of the two new calls.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import blob_cases as K
import cda
from cda import _native as N
from cda import blob as B
from cda import square as S
from test_inclusion import mainnet_blobs, mainnet_ods
from test_square import mainnet_txs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")


# ---- block 408 ----
def test_block_408_has_three_sequences():
    ods = mainnet_ods()
    seqs, com, summary = B.index_host(list(ods), 32, 64, commit=K.oracle_commit(64))
    assert [(int(s["kind"]), int(s["start"]), int(s["nshares"]), int(s["seq_len"]), int(s["status"])) for s in seqs] == [
        (N.SEQ_KIND_TX, 0, 364, 173621, 0), (N.SEQ_KIND_PFB, 364, 1, 351, 0), (N.SEQ_KIND_BLOB, 368, 352, 169275, 0)]
    assert summary == {"k": 32, "nseq": 3, "npadding": 307, "norphans": 0, "first_orphan": N.NO_SHARE}
    assert seqs[0]["ns"].tobytes() == S.TX_NAMESPACE and seqs[1]["ns"].tobytes() == S.PAY_FOR_BLOB_NAMESPACE
    (want,) = mainnet_blobs()
    blobs, flagged = B.get_all(B.HostSquare(ods, commit=K.oracle_commit(64)))
    assert flagged == [] and len(blobs) == 1
    (b,) = blobs
    assert (b.data, b.namespace, b.share_version, b.start, b.nshares, b.commitment) == \
        (want["data"], want["ns"], want["version"], want["start"], want["n"], want["commitment"])
    assert com[2].tobytes() == want["commitment"] and not com[:2].any()
    host = B.HostSquare(ods, commit=K.oracle_commit(64))
    assert B.get(host, want["ns"], want["commitment"]) == b and B.included(host, want["ns"], want["commitment"])
    flipped = bytes([want["commitment"][0] ^ 1]) + want["commitment"][1:]
    assert not B.included(host, want["ns"], flipped)
    with pytest.raises(B.BlobNotFound):
        B.get(host, want["ns"], flipped)


# ---- round trip ----
def check_round_trip(txs, shares, info):
    normal = [t for t in txs if S.unmarshal_blob_tx(t) is None]
    pfbs = [S.unmarshal_blob_tx(t)[0] for t in txs if S.unmarshal_blob_tx(t) is not None]
    got_normal, got_pfbs, got_idx = B.parse_txs(B.HostSquare(shares))
    assert got_normal == normal and got_pfbs == pfbs
    assert got_idx == info["pfb_share_indexes"]


def test_round_trip_block_408():
    txs, _ = mainnet_txs()
    ss, shares, info = S.construct(txs, 128, 64)
    assert ss == 32
    check_round_trip(txs, shares, info)


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_round_trip_synthetic(k):
    txs = list(K.synthetic_txs(k))
    ss, shares, info = S.construct(txs, 128, 64)
    assert ss == k
    if k == 1:
        assert info["blobs"] == 0 and info["normal_txs"] > 0
    if k == 2:
        assert info["normal_txs"] == 0 and info["blobs"] > 0
    check_round_trip(txs, shares, info)
    # every blob comes back as it went in, in square order (namespace, then PFB order)
    blobs, flagged = B.get_all(B.HostSquare(shares, commit=K.oracle_commit(64)))
    want = sorted(((b["ns"], i, b["data"]) for i, b in enumerate(b for t in txs if S.unmarshal_blob_tx(t)
                                                                for b in S.unmarshal_blob_tx(t)[1])),
                  key=lambda x: (x[0], x[1]))
    assert flagged == [] and [(b.namespace, b.data) for b in blobs] == [(ns, d) for ns, _, d in want]
    assert [b.start for b in blobs] == sorted(i for idx in info["pfb_share_indexes"] for i in idx)


def test_index_wrapper_round_trip():
    for idx in ([], [0], [5, 300, 16383]):
        assert B.unmarshal_index_wrapper(S.marshal_index_wrapper(b"tx bytes", idx)) == (b"tx bytes", idx)
    with pytest.raises(ValueError):
        B.unmarshal_index_wrapper(b"\x0a\x02hi")


# ---- the rule header against the mirror ----
@pytest.fixture(scope="module")
def rule_dump(tmp_path_factory):
    """share_index_rule_dump under ASan + UBSan: every k = 2 square over the alphabet, threshold 1."""
    exe = str(tmp_path_factory.mktemp("rule") / "share_index_rule_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(SAN, "share_index_rule_dump.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    stdin = "".join(h.hex() + "\n" for _, h in K.ALPHABET)
    return subprocess.run([exe, "1"], input=stdin, env=env, capture_output=True, text=True,
                          check=True).stdout.splitlines()


def test_rule_dump_equals_index_host(rule_dump):
    """Line for line; and every status bit, an orphan count above zero and a sequence cut by padding occur in the
    set, so the alphabet cannot lose a case unnoticed."""
    A = len(K.ALPHABET)
    assert A >= 8 and len(rule_dump) == A ** 4 >= 4096
    shares = [h + bytes(512 - len(h)) for _, h in K.ALPHABET]
    seen_status, seen_orphans, seen_kinds = 0, 0, set()
    for c, line in enumerate(rule_dump):
        idx = [c // A ** 3, c // A ** 2 % A, c // A % A, c % A]
        seqs, _, summary = B.index_host([shares[i] for i in idx], 2, 1, commit=False)
        want = "%d %d %d %d | %d %d %d %d |" % (*idx, summary["nseq"], summary["npadding"], summary["norphans"],
                                                 summary["first_orphan"])
        for s in seqs:
            want += " %d:%d:%d:%d:%d:%d:%s" % (s["start"], s["nshares"], s["seq_len"], s["kind"], s["share_version"],
                                                s["status"], s["ns"].tobytes().hex())
            seen_status |= int(s["status"])
            seen_kinds.add(int(s["kind"]))
        assert line == want, (idx, line, want)
        seen_orphans = max(seen_orphans, summary["norphans"])
    assert seen_status == (N.SEQ_TRUNCATED | N.SEQ_BROKEN | N.SEQ_VERSION | N.SEQ_RESERVED_NS | N.SEQ_UNALIGNED)
    assert seen_orphans == 4 and seen_kinds == {N.SEQ_KIND_TX, N.SEQ_KIND_PFB, N.SEQ_KIND_BLOB}
    # a length of 0xFFFFFFFF claims millions of shares, not one: truncated, every share behind it inside the claim
    huge = [i for i, (name, _) in enumerate(K.ALPHABET) if "0xFFFFFFFF" in name]
    assert len(huge) == 2
    for i, want_n in zip(huge, (8910721, 8985288)):
        rec = rule_dump[i * A ** 3 + 3 * A ** 2 + 3 * A + 3].split("|")[2].split()[0].split(":")  # then continuations
        assert int(rec[1]) == want_n and int(rec[2]) == 0xFFFFFFFF and int(rec[5]) & N.SEQ_TRUNCATED
        assert rule_dump[i * A ** 3 + 3 * A ** 2 + 3 * A + 3].split("|")[1].split()[2] == "0"  # no orphan


def test_named_mutations_give_their_bits():
    """The hostile squares of the GPU tests, on the host: each named mutation sets its bit in some record."""
    base, _, summary = B.index_host(list(K.synthetic_square(8)[0]), 8, 64, commit=False)
    assert not base["status"].any() and summary["norphans"] == 0
    for name, bit, _ in K.MUTATIONS:
        case = K.mutated(8, name)
        seqs, _, _ = B.index_host(list(case["ods"]), 8, case["threshold"], commit=False)
        assert np.bitwise_or.reduce(seqs["status"]) & bit, name
    _, _, s = B.index_host(list(K.orphan_run_square()), 8, 64, commit=False)
    assert s["first_orphan"] == 0 and s["norphans"] >= 2
    seqs, _, s = B.index_host(list(K.continuation_only_square()), 8, 64, commit=False)
    assert len(seqs) == 0 and s == {"k": 8, "nseq": 0, "npadding": 0, "norphans": 64, "first_orphan": 0}
    for ods in K.huge_length_squares():
        seqs, _, _ = B.index_host(list(ods), 8, 64, commit=False)
        big = seqs[seqs["seq_len"] >= 0xFFFFFFFE]
        assert len(big) >= 1 and (big["status"] & N.SEQ_TRUNCATED).all() and (big["nshares"] > 8000000).all()


# ---- ABI ----
def test_new_calls_are_declared_exported_and_check_arguments():
    header = open(os.path.join(ROOT, "include", "cda.h")).read()
    L = cda.lib()
    for name in ("cda_square_index", "cda_square_read"):
        assert name + "(" in header and name in N.EXPORTS and hasattr(L, name)
    summary = N.SquareSummary()
    assert L.cda_square_index(None, 64, 0, None, None, ctypes.byref(summary)) == N.E_ARG
    assert L.cda_square_read(None, 1, None, None, 0, None) == N.E_ARG
    for name, value in (("TRUNCATED", 1), ("BROKEN", 2), ("VERSION", 4), ("RESERVED_NS", 8), ("UNALIGNED", 16)):
        assert getattr(N, "SEQ_" + name) == value and f"CDA_SEQ_{name} = {value}," in header
    assert "CDA_SEQ_KIND_TX = 0, CDA_SEQ_KIND_PFB = 1, CDA_SEQ_KIND_BLOB = 2" in header


def test_structs_match_header(tmp_path):
    """cda_sequence 48, cda_square_summary 20, cda_sequence_range 16 bytes: ctypes, numpy and a C compiler agree."""
    assert ctypes.sizeof(N.Sequence) == 48 == N.SEQUENCE_DTYPE.itemsize
    assert ctypes.sizeof(N.SquareSummary) == 20
    assert ctypes.sizeof(N.SequenceRange) == 16 == N.SEQUENCE_RANGE_DTYPE.itemsize
    for ct, dt in ((N.Sequence, N.SEQUENCE_DTYPE), (N.SequenceRange, N.SEQUENCE_RANGE_DTYPE)):
        for name, _ in ct._fields_:
            assert getattr(ct, name).offset == dt.fields[name][1], name
    src = tmp_path / "sizes.c"
    src.write_text('#include "cda.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(cda_sequence), sizeof(cda_square_summary), sizeof(cda_sequence_range)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    assert subprocess.check_output([exe], text=True).split() == ["48", "20", "16"]


@pytest.mark.parametrize("kernel", ["share_scan_totals_kernel", "share_index_kernel", "sequence_read_kernel"])
def test_blob_kernels_have_no_scratch(kernel, tmp_path):
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
