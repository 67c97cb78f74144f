"""Namespace data with completeness proofs from a retained square (nmt ProveNamespace / Proof.VerifyNamespace).

"Give me everything in namespace N of this block, and prove nothing was withheld": per row of the extended square
whose root's [min, max] holds N, the row's shares of N with the inclusion proof of their whole run, or, where the row
has no share of N, an absence proof.  One libcda call finds the runs in the retained leaf records, gathers the proofs
from the retained nodes and copies the shares (cda_square_prove_namespace); one call verifies a batch of rows,
completeness included (cda_nmt_verify_namespace).  The rows' proofs to the data root are cda_square_share_proofs'.
"""
import numpy as np

from . import _native as N
from .appconsts import NAMESPACE_SIZE
from .proof import NMTProof


def rows_of_namespace(row_roots, nid):
    """The rows whose root has min <= nid <= max (the rows a namespace query must answer for), from the row roots."""
    nid = bytes(nid)
    out = []
    for r, root in enumerate(row_roots):
        root = bytes(root)
        if root[:NAMESPACE_SIZE] <= nid <= root[NAMESPACE_SIZE:2 * NAMESPACE_SIZE]:
            out.append(r)
    return out


def get_shares_by_namespace(square, nid):
    """Every share of namespace `nid` in the block of `square` (an open cda Square), row by row, each row with its
    proof of completeness -> list of (row, shares, NMTProof): shares the row's shares of nid in order ([] with an
    absence proof: proof.leaf_hash set).  Rows whose root excludes nid are not listed: their root is the proof."""
    nid = bytes(nid)
    if len(nid) != NAMESPACE_SIZE:
        raise ValueError(f"namespace of {len(nid)} bytes, not {NAMESPACE_SIZE}")
    rows = rows_of_namespace(square.row_roots, nid)
    if not rows:
        return []
    results, nodes, leaf_hashes, shares = square.prove_namespace([(N.AXIS_ROW, r, nid) for r in rows])
    out = []
    for i, r in enumerate(rows):
        res = results[i]
        proof = NMTProof(int(res["start"]), int(res["end"]), [nodes[i, j].tobytes() for j in range(int(res["nnodes"]))])
        if res["kind"] == N.NSP_ABSENCE:
            proof.leaf_hash = leaf_hashes[i].tobytes()
        off = int(res["share_off"])
        out.append((r, [shares[off + j].tobytes() for j in range(int(res["nshares"]))], proof))
    return out


def pack_namespace_proofs(nid, rows, row_roots):
    """The flat arrays cda_nmt_verify_namespace takes for `rows` ((row, shares, NMTProof) as get_shares_by_namespace
    returns them), proof i against row_roots[row] -> dict(descs, namespaces, roots, nodes, leaf_hashes, leaves)."""
    nid = bytes(nid)
    roots = np.ascontiguousarray(row_roots, np.uint8).reshape(-1, N.NODE_SIZE)
    descs = np.zeros(len(rows), N.NMT_NS_PROOF_DESC_DTYPE)
    nodes, leaf_hashes, leaves = [], [], []
    for i, (row, shares, p) in enumerate(rows):
        lh = N.NO_LEAF_HASH
        if p.leaf_hash:
            lh = len(leaf_hashes)
            leaf_hashes.append(bytes(p.leaf_hash))
        descs[i] = (p.start, p.end, len(nodes), len(p.nodes), len(leaves), len(shares), row, lh)
        nodes += [bytes(x) for x in p.nodes]
        leaves += [bytes(x) for x in shares]

    def flat(items, n):
        if any(len(x) != n for x in items):
            raise ValueError(f"cda_nmt_verify_namespace takes items of {n} bytes")
        return np.frombuffer(b"".join(items), np.uint8).reshape(-1, n) if items else np.zeros((0, n), np.uint8)
    return {"descs": descs, "namespaces": np.tile(np.frombuffer(nid, np.uint8), (len(rows), 1)), "roots": roots,
            "nodes": flat(nodes, N.NODE_SIZE), "leaf_hashes": flat(leaf_hashes, N.NODE_SIZE),
            "leaves": flat(leaves, N.SHARE_SIZE)}


def verify_namespace_data(ctx, nid, rows, row_roots):
    """NMTProof.verify_namespace(nid, shares, row_roots[row]) of every (row, shares, proof) on the device, one call
    (cda_nmt_verify_namespace) -> list of bool.  A row number outside row_roots is False."""
    rows = list(rows)
    if not rows:
        return []
    a = pack_namespace_proofs(nid, rows, row_roots)
    ok = ctx.nmt_verify_namespace(a["descs"], a["namespaces"], a["roots"], a["nodes"], a["leaf_hashes"], a["leaves"])
    return [bool(x) for x in ok]
