"""CPU tests of the share proofs to the data root (cda_square_share_proofs, cda_share_proofs_validate): the merkle
walk the row-proof kernel evaluates (csrc/merkle_walk_rule.h, plan::merkle_walk) against cda.proof.Proof.verify, the
argument checks and record sizes of the new entry points, the new kernels' register budget, and the tx share ranges
of mainnet block 408.  No GPU.
"""
import ctypes
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import cda
import oracle_lib as O
from cda import _native as N
from cda import proof as P
from cda import square as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "celestia-app_amd", "csrc")
DUMP_SRC = [os.path.join(ROOT, "tests", "san", "merkle_walk_dump.cpp"), os.path.join(CSRC, "plan.cpp")]


def _inner(left, right):
    return hashlib.sha256(b"\x01" + left + right).digest()


def _fold(leaf_hash, aunts, order):
    """The root the header's fold order gives: aunt j on the left where order[j] == 'L'."""
    h = leaf_hash
    for a, side in zip(aunts, order):
        h = _inner(a, h) if side == "L" else _inner(h, a)
    return h


def _verifies(total, index, leaf_hash, aunts, root, item):
    try:
        P.Proof(total, index, leaf_hash, aunts).verify(root, item)
        return True
    except P.ProofError:
        return False


def _check_dump(lines):
    """Every line of merkle_walk_dump against Proof.verify.  Trees of up to 64 leaves are built by the oracle
    (ora_merkle_proof: real leaf hash, aunts and root); for the larger totals the aunts are random and the root is
    the one the printed fold order gives, which Proof.verify's own recursion must then reproduce."""
    rng = random.Random(0x51DE)
    trees = {}
    accepted = rejected = 0
    for ln in lines:
        f = ln.split()
        total, index, na, rest = int(f[0]), int(f[1]), int(f[2]), f[3:]
        reject = rest == ["reject"]
        item = b"item%04d" % max(index, 0)
        if 0 < total <= 64 and 0 <= index < total:
            if total not in trees:
                items = [b"item%04d" % i for i in range(total)]
                trees[total] = [O.merkle_proof(items, i) for i in range(total)]
            leaf_hash, aunts, root = trees[total][index]
            aunts = (aunts + [bytes(32)] * na)[:na]  # dropped from the top, or padded
            assert leaf_hash == hashlib.sha256(b"\x00" + item).digest()
        else:
            leaf_hash = hashlib.sha256(b"\x00" + item).digest()
            aunts = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(min(na, 128))]
            root = bytes(32) if reject else _fold(leaf_hash, aunts, rest)
        want = _verifies(total, index, leaf_hash, aunts, root, item)
        assert want == (not reject), ln
        if not reject:
            assert len(rest) == na and _fold(leaf_hash, aunts, rest) == root, ln
        accepted += want
        rejected += not want
    return accepted, rejected


@pytest.fixture(scope="module")
def dump_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mw") / "merkle_walk_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe] + DUMP_SRC)
    return subprocess.check_output([exe, "64", "300"], text=True).splitlines()


def test_merkle_walk_matches_proof_verify(dump_lines):
    """plan::merkle_walk (the header the row-proof kernel includes) gives Proof.verify's verdict and the fold order
    that rebuilds the oracle's root: every (total, index) up to 64 leaves with 0 .. path length + 1 aunts, index -1
    and index = total, 300 random totals up to 2^62, total <= 0 and more than MAX_AUNTS aunts."""
    accepted, rejected = _check_dump(dump_lines)
    assert accepted >= 64 * 65 // 2 + 300 and rejected >= 2 * accepted, (accepted, rejected)
    assert any(ln.startswith("8 3 101 ") and ln.endswith("reject") for ln in dump_lines)


def test_merkle_walk_dump_under_sanitizers(tmp_path, dump_lines):
    """The same program as a plain executable built with AddressSanitizer and UBSan prints the same lines."""
    exe = str(tmp_path / "merkle_walk_dump_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe] + DUMP_SRC)
    assert subprocess.check_output([exe, "64", "300"], text=True).splitlines() == dump_lines


def test_share_proof_entry_points_reject_bad_arguments_without_gpu():
    """Argument checks run before any device work: negative codes, no abort."""
    L = cda.lib()
    assert L.cda_square_share_proofs(None, 1, None, 2, 1, None, None, None, None, None, None, None, 0, None) == N.E_ARG
    assert L.cda_share_proofs_validate(None, 1, None, None, None, None, 0, None, 0, None, 0, None, 0, None, 0,
                                       None) == N.E_ARG
    assert L.cda_share_proofs_validate_device(None, 1, None, None, None, None, 0, None, 0, None, 0, None, 0, None, 0,
                                              None, None) == N.E_ARG
    H = N.lib(N.HOOKS_LIB_PATH)
    os.environ["CDA_FAULT_INJECT"] = "entry"
    try:
        assert H.cda_square_share_proofs(None, 1, None, 2, 1, None, None, None, None, None, None, None, 0,
                                         None) == N.E_NOMEM
        assert H.cda_share_proofs_validate(None, 1, None, None, None, None, 0, None, 0, None, 0, None, 0, None, 0,
                                           None) == N.E_NOMEM
        assert H.cda_share_proofs_validate_device(None, 1, None, None, None, None, 0, None, 0, None, 0, None, 0, None,
                                                  0, None, None) == N.E_NOMEM
    finally:
        del os.environ["CDA_FAULT_INJECT"]


def test_share_proof_structs_match_header():
    """include/cda.h: cda_share_range 8, cda_share_row 48, cda_share_proof_desc 68 bytes."""
    assert ctypes.sizeof(N.ShareRange) == 8 == N.SHARE_RANGE_DTYPE.itemsize
    assert ctypes.sizeof(N.ShareRow) == 48 == N.SHARE_ROW_DTYPE.itemsize
    assert ctypes.sizeof(N.ShareProofDesc) == 68 == N.SHARE_PROOF_DESC_DTYPE.itemsize
    for ct, dt in ((N.ShareRange, N.SHARE_RANGE_DTYPE), (N.ShareRow, N.SHARE_ROW_DTYPE),
                   (N.ShareProofDesc, N.SHARE_PROOF_DESC_DTYPE)):
        for name, _ in ct._fields_:
            assert getattr(ct, name).offset == dt.fields[name][1], name


def test_header_struct_sizes_by_the_compiler(tmp_path):
    """The sizes as a C compiler lays the header's structs out."""
    src = tmp_path / "sizes.c"
    src.write_text('#include "cda.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(cda_share_range), sizeof(cda_share_row), sizeof(cda_share_proof_desc)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    assert subprocess.check_output([exe], text=True).split() == ["8", "48", "68"]


@pytest.mark.parametrize("kernel", ["square_share_proofs_kernel", "row_proof_verify_kernel",
                                    "share_validate_prep_kernel", "share_validate_combine_kernel"])
def test_share_proof_kernels_register_budget(kernel, tmp_path):
    """No spilled VGPR, no private segment, at most 128 VGPRs (4 waves per SIMD), read from the built library's
    metadata as tests/test_sampling.py does for the kernels before these."""
    import test_hash_kernel_registers as R
    if not (os.path.exists(R.V.OBJDUMP) and os.path.exists(R.READOBJ) and os.path.exists(R.LIB)):
        pytest.skip("needs llvm-objdump, llvm-readobj and the built libcda.so")
    found = {n: m for n, m in R.kernel_metadata(R.LIB, str(tmp_path)).items() if kernel in n}
    assert len(found) == 1, sorted(found)
    (name, m), = found.items()
    print(name, m)
    assert m["vgpr_count"] <= 128 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m


# ---- tx share ranges on mainnet block 408 ----
def mainnet_txs():
    z = np.load(os.path.join(GOLDEN, "mainnet_h408_txs.npz"))
    offs = z["offsets"]
    return [z["data"][offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)], z["data_hash"].tobytes()


def _compact_sequence(shares):
    """The bytes of a compact sequence given ALL its shares (parsed back: headers and reserved bytes dropped)."""
    out = b""
    for i, sh in enumerate(shares):
        out += sh[S.NS + 1 + (4 if i == 0 else 0) + 4:]
    return out[:int.from_bytes(shares[0][S.NS + 1:S.NS + 5], "big")]


def test_find_tx_share_range_block_408():
    """For each of block 408's txs, the shares in the returned range, parsed back as compact shares, hold exactly
    that tx's bytes (index-wrapped for the BlobTx) with its length prefix at the expected offset; the range is the
    tightest one (its first share holds the prefix's first byte, its last share the tx's last byte)."""
    txs, _ = mainnet_txs()
    assert len(txs) == 274
    k, shares, info = S.construct(txs, 128, 64)
    assert k == 32
    blob = [S.unmarshal_blob_tx(t) is not None for t in txs]
    assert sum(blob) == 1
    seqs = {}
    for ns, first, n in ((S.TX_NAMESPACE, 0, info["tx_shares"]),
                         (S.PAY_FOR_BLOB_NAMESPACE, info["tx_shares"], info["pfb_shares"])):
        assert all(sh[:S.NS] == ns for sh in shares[first:first + n])
        seqs[ns] = (first, _compact_sequence(shares[first:first + n]))
    pos = {S.TX_NAMESPACE: 0, S.PAY_FOR_BLOB_NAMESPACE: 0}
    for i, raw in enumerate(txs):
        ns = S.PAY_FOR_BLOB_NAMESPACE if blob[i] else S.TX_NAMESPACE
        unit = raw
        if blob[i]:
            unit = S.marshal_index_wrapper(S.unmarshal_blob_tx(raw)[0], info["pfb_share_indexes"][0])
        first, seq = seqs[ns]
        lo = pos[ns]
        hi = lo + len(S.varint(len(unit))) + len(unit)
        assert seq[lo:hi] == S.varint(len(unit)) + unit  # where the tx lies in its sequence
        pos[ns] = hi
        start, end = S.find_tx_share_range(txs, i, 128, 64)
        assert first <= start < end <= first + (info["pfb_shares"] if blob[i] else info["tx_shares"])
        # the range's shares parsed back: sequence bytes [b0, b1) hold the tx at offset lo - b0
        s0, s1 = start - first, end - first
        b0 = 0 if s0 == 0 else 474 + (s0 - 1) * 478
        b1 = 474 + (s1 - 1) * 478
        got = b"".join(sh[S.NS + 1 + (4 if first + s0 + j == first else 0) + 4:]
                       for j, sh in enumerate(shares[start:end]))
        assert got[lo - b0:hi - b0] == S.varint(len(unit)) + unit
        assert b0 <= lo and hi <= b1
        assert lo < (474 + s0 * 478) and hi - 1 >= (474 + (s1 - 2) * 478 if s1 >= 2 else 0)  # tight at both ends
    with pytest.raises(S.SquareError):
        S.find_tx_share_range(txs, len(txs), 128, 64)
