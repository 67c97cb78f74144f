"""Blobs read back from a retained square: what is in it, by namespace and share commitment.

celestia-node's blob service (blob.Get / GetAll / GetProof / Included) asks with a namespace and a share commitment.
A node that downloaded, repaired or rebuilt a square has its bytes on the device and nothing else: no share ranges.
cda_square_index finds every sequence of the square (the TRANSACTION and PAY_FOR_BLOB sequences and the blobs) with
one ordered scan over the share headers and hashes the clean blobs' commitments out of the retained tree nodes;
cda_square_read copies payloads out with the share headers stripped.  The range a commitment was found at is what
Square.commitment_proofs takes.

The rule is csrc/share_index_rule.h; index_host is its mirror here, written from the definitions (last(g), claims)
and not from the scan's encoding.  Parity unpinned: go-square's shares package (ParseBlobs, ParseTxs) is not in the
reference tree; the rule restates specs/src/specs/shares.md:27-107 and specs/src/specs/namespace.md.
"""
from dataclasses import dataclass

import numpy as np

from . import _native as N
from . import inclusion
from .appconsts import NAMESPACE_SIZE, SUBTREE_ROOT_THRESHOLD
from .square import (PAY_FOR_BLOB_NAMESPACE, TX_NAMESPACE, compact_shares_needed, parse_fields, read_varint)

SPARSE_FIRST, SPARSE_NEXT = 478, 482
COMPACT_FIRST, COMPACT_NEXT = 474, 478


class BlobNotFound(Exception):
    pass


@dataclass
class Blob:
    """A blob as the square holds it: shares [start, start + nshares) of the ODS."""
    namespace: bytes
    data: bytes
    share_version: int
    start: int
    nshares: int
    commitment: bytes


# ---- the rule on the host ----
def _claim(compact, seq_len):
    if compact:
        return max(1, compact_shares_needed(seq_len))
    return inclusion.sparse_shares_needed(seq_len)


def _reserved(ns):
    return (ns[0] == 0 and not any(ns[1:28])) or ns[0] == 0xFF


def strip_host(shares, start, nshares, seq_len, compact):
    """Payload bytes [0, seq_len) of the sequence at shares [start, start + nshares): 34 bytes stripped from a blob's
    first share and 30 from its later ones, 38 and 34 from a compact sequence's."""
    first, later = (38, 34) if compact else (34, 30)
    out = bytearray()
    for j in range(nshares):
        if len(out) >= seq_len:
            break
        out += bytes(shares[start + j])[first if j == 0 else later:]
    if len(out) < seq_len:
        raise ValueError(f"sequence at share {start}: {nshares} shares hold fewer than {seq_len} bytes")
    return bytes(out[:seq_len])


def index_host(ods_shares, k, threshold=SUBTREE_ROOT_THRESHOLD, commit=None, ctx=None):
    """The mirror of cda_square_index on the k x k ODS shares (row-major) -> (SEQUENCE_DTYPE rows, (nseq, 32) uint8
    commitments, summary dict).  The commitment of a status-0 blob is CreateCommitment over its parsed bytes:
    commit(ns, data, share_version) -> 32 bytes (default inclusion.create_commitment, which hashes on the device);
    commit=False leaves them out (None).  threshold 0: CDA_SEQ_UNALIGNED is not looked at."""
    n = k * k
    if len(ods_shares) != n:
        raise ValueError(f"{len(ods_shares)} shares are not a {k} x {k} square")
    heads = [bytes(s[:34]) for s in ods_shares]
    seqs, npad, orphans = [], 0, []
    last = None  # (share index, the sequence it started or None for a padding share)
    for g, h in enumerate(heads):
        ns, info, seq_len = h[:NAMESPACE_SIZE], h[29], int.from_bytes(h[30:34], "big")
        owner = last[1] if last is not None else None
        inside = owner is not None and g < owner["start"] + owner["nshares"]
        if not info & 1:
            if not inside:
                orphans.append(g)
            elif ns != owner["ns"] or info >> 1 != owner["share_version"]:
                owner["status"] |= N.SEQ_BROKEN
            continue
        if inside:
            owner["status"] |= N.SEQ_BROKEN
        compact = ns in (TX_NAMESPACE, PAY_FOR_BLOB_NAMESPACE)
        if not compact and seq_len == 0:
            npad += 1
            last = (g, None)
            continue
        kind = N.SEQ_KIND_BLOB if not compact else (N.SEQ_KIND_TX if ns == TX_NAMESPACE else N.SEQ_KIND_PFB)
        cnt = _claim(compact, seq_len)
        status = 0
        if g + cnt > n:
            status |= N.SEQ_TRUNCATED
        if info >> 1:
            status |= N.SEQ_VERSION
        if kind == N.SEQ_KIND_BLOB:
            if _reserved(ns):
                status |= N.SEQ_RESERVED_NS
            if threshold:
                W = inclusion.sub_tree_width(cnt, threshold)
                if W > k or g % W:
                    status |= N.SEQ_UNALIGNED
        rec = {"start": g, "nshares": cnt, "seq_len": seq_len, "kind": kind, "share_version": info >> 1,
               "status": status, "ns": ns}
        seqs.append(rec)
        last = (g, rec)
    out = np.zeros(len(seqs), N.SEQUENCE_DTYPE)
    for i, r in enumerate(seqs):
        out[i] = (r["start"], r["nshares"], r["seq_len"], r["kind"], r["share_version"], r["status"], 0,
                  np.frombuffer(r["ns"], np.uint8), 0)
    com = None
    if commit is not False:
        if commit is None:
            def commit(ns, data, version):
                return inclusion.create_commitment(inclusion.Blob(ns, data, version), threshold, ctx)
        com = np.zeros((len(seqs), 32), np.uint8)
        for i, r in enumerate(seqs):
            if r["kind"] == N.SEQ_KIND_BLOB and r["status"] == 0:
                data = strip_host(ods_shares, r["start"], r["nshares"], r["seq_len"], False)
                com[i] = np.frombuffer(commit(r["ns"], data, r["share_version"]), np.uint8)
    summary = {"k": k, "nseq": len(seqs), "npadding": npad, "norphans": len(orphans),
               "first_orphan": orphans[0] if orphans else N.NO_SHARE}
    return out, com, summary


class HostSquare:
    """The ODS shares of a square with Square's index / read, on the host.  commit: index_host's (default: the
    commitments by inclusion.create_commitment, which hashes on the device; a callable for another engine)."""

    def __init__(self, ods_shares, commit=None):
        self.shares = [bytes(s) for s in ods_shares]
        self.k = max(1, int(round(len(self.shares) ** 0.5)))
        self._commit = commit

    def index(self, threshold=SUBTREE_ROOT_THRESHOLD, commitments=True):
        return index_host(self.shares, self.k, threshold, self._commit if commitments else False)

    def read(self, seqs):
        return [strip_host(self.shares, int(q["start"]), int(q["nshares"]), int(q["seq_len"]), bool(q["compact"]))
                for q in N.Square.sequence_ranges(seqs)]


# ---- the blob service ----
def get_all(square, namespaces=None, threshold=SUBTREE_ROOT_THRESHOLD):
    """blob.GetAll: the blobs of `namespaces` (29-byte namespaces; None: every namespace) in the square, in square
    order -> (list of Blob, flagged).  Only blobs of status 0 are returned; flagged holds the SEQUENCE_DTYPE records
    of the asked namespaces' blobs that have a status bit set."""
    seqs, com, _ = square.index(threshold)
    want = None if namespaces is None else {bytes(ns) for ns in namespaces}
    pick = [i for i in range(len(seqs)) if seqs[i]["kind"] == N.SEQ_KIND_BLOB and
            (want is None or seqs[i]["ns"].tobytes() in want)]
    good = [i for i in pick if seqs[i]["status"] == 0]
    datas = square.read(seqs[good]) if good else []
    blobs = [Blob(seqs[i]["ns"].tobytes(), d, int(seqs[i]["share_version"]), int(seqs[i]["start"]),
                  int(seqs[i]["nshares"]), com[i].tobytes()) for i, d in zip(good, datas)]
    return blobs, [seqs[i] for i in pick if seqs[i]["status"] != 0]


def _find(square, ns, commitment, threshold):
    ns, commitment = bytes(ns), bytes(commitment)
    seqs, com, _ = square.index(threshold)
    for i in range(len(seqs)):
        if (seqs[i]["kind"] == N.SEQ_KIND_BLOB and seqs[i]["status"] == 0 and seqs[i]["ns"].tobytes() == ns and
                com[i].tobytes() == commitment):
            return seqs[i]
    return None


def get(square, ns, commitment, threshold=SUBTREE_ROOT_THRESHOLD):
    """blob.Get: the blob of namespace `ns` with share commitment `commitment`, or BlobNotFound."""
    rec = _find(square, ns, commitment, threshold)
    if rec is None:
        raise BlobNotFound(f"no blob with commitment {bytes(commitment).hex()} in namespace {bytes(ns).hex()}")
    (data,) = square.read(np.array([rec], N.SEQUENCE_DTYPE))
    return Blob(bytes(ns), data, int(rec["share_version"]), int(rec["start"]), int(rec["nshares"]), bytes(commitment))


def included(square, ns, commitment, threshold=SUBTREE_ROOT_THRESHOLD):
    """blob.Included, the prover's half: the square holds a blob of `ns` with that commitment."""
    return _find(square, ns, commitment, threshold) is not None


def get_proof(square, ns, commitment, threshold=SUBTREE_ROOT_THRESHOLD):
    """blob.GetProof: the commitment proof (cda.commitment.CommitmentProof) of that blob, or BlobNotFound."""
    rec = _find(square, ns, commitment, threshold)
    if rec is None:
        raise BlobNotFound(f"no blob with commitment {bytes(commitment).hex()} in namespace {bytes(ns).hex()}")
    return square.commitment_proofs([(int(rec["start"]), int(rec["nshares"]))], [bytes(ns)], threshold)[0]


# ---- the compact sequences ----
def split_units(seq):
    """The varint-delimited units of a compact sequence's bytes."""
    out, i = [], 0
    while i < len(seq):
        n, i = read_varint(seq, i)
        if i + n > len(seq):
            raise ValueError("a unit runs past the end of its sequence")
        out.append(bytes(seq[i:i + n]))
        i += n
    return out


def unmarshal_index_wrapper(raw):
    """The inverse of square.marshal_index_wrapper -> (tx, share_indexes)."""
    tx, idx, type_id = b"", [], b""
    for f, wt, v in parse_fields(raw) or []:
        if f == 1 and wt == 2:
            tx = v
        elif f == 2 and wt == 2:
            i = 0
            while i < len(v):
                x, i = read_varint(v, i)
                idx.append(x)
        elif f == 2 and wt == 0:
            idx.append(v)
        elif f == 3 and wt == 2:
            type_id = v
    if type_id != b"INDX":
        raise ValueError("not an IndexWrapper")
    return tx, idx


def parse_txs(square):
    """The inverse of square.construct's compact part: (normal txs, PFB txs, their share indexes) read from the
    TRANSACTION and PAY_FOR_BLOB sequences of `square` (a Square or a HostSquare)."""
    seqs, _, _ = square.index(0, commitments=False)
    units = {}
    for kind in (N.SEQ_KIND_TX, N.SEQ_KIND_PFB):
        found = seqs[seqs["kind"] == kind]
        if len(found) > 1 or (len(found) and found[0]["status"]):
            raise ValueError("the square's compact sequences are not as square.Construct lays them out")
        units[kind] = split_units(square.read(found)[0]) if len(found) else []
    wrapped = [unmarshal_index_wrapper(u) for u in units[N.SEQ_KIND_PFB]]
    return units[N.SEQ_KIND_TX], [tx for tx, _ in wrapped], [idx for _, idx in wrapped]


__all__ = ["Blob", "BlobNotFound", "HostSquare", "get", "get_all", "get_proof", "included", "index_host", "parse_txs",
           "split_units", "strip_host", "unmarshal_index_wrapper"]
