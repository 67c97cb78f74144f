"""Sample proofs: prove cells of a retained square, verify proved cells in batches.

What connects block production to repair (celestia-app @ 2025-02-13): a node that has extended a block hands out
cells with their NMT proofs -- any cell of the 2k x 2k square against its row or its column root, which is
wrapper.ErasuredNamespacedMerkleTree.ProveRange (pkg/wrapper/nmt_wrapper.go:127-130; its test proves every cell of an
erasured axis, nmt_wrapper_test.go:151-180) -- and a sampling or reconstruction pipeline checks every cell it receives
with nmt.Proof.VerifyInclusion before the square goes to repair.  Both run on the device here: Square.prove
(cda_square_prove) gathers the proofs of many cells from the retained tree nodes in one launch, Context.nmt_verify
(cda_nmt_verify) checks many proofs in one launch.  ShareProof.verify_proof (cda.proof) stays on the host: a handful of
hashes.
"""
import numpy as np

from . import _native as N
from .appconsts import NAMESPACE_SIZE, PARITY_SHARES_NAMESPACE
from .proof import NMTProof


def sample_namespace(k, axis, index, pos, share):
    """The namespace a cell's leaf hashes under (the wrapper's quadrant rule, nmt_wrapper.go:138-140): the share's own
    inside Q0, else the parity namespace.  (axis, index, pos): leaf `pos` of row (axis 0) or column (axis 1) `index`."""
    return bytes(share[:NAMESPACE_SIZE]) if index < k and pos < k else PARITY_SHARES_NAMESPACE


def sample_proofs(square, coords, axis):
    """Proofs of the cells at `coords` ((row, col) pairs) of an open Square against their row roots (axis 0) or column
    roots (axis 1), one launch.  -> list of (axis, index, pos, share bytes, NMTProof)."""
    coords = [(int(r), int(c)) for r, c in coords]
    q = np.zeros(len(coords), N.RANGE_QUERY_DTYPE)
    for i, (r, c) in enumerate(coords):
        index, pos = (c, r) if axis else (r, c)
        q[i] = (axis, index, pos, pos + 1)
    counts, nodes, shares = square.prove(q)
    return [(axis, int(q[i]["index"]), int(q[i]["start"]), shares[i].tobytes(),
             NMTProof(int(q[i]["start"]), int(q[i]["end"]), [nodes[i, j].tobytes() for j in range(counts[i])]))
            for i in range(len(coords))]


def pack_samples(samples, k):
    """The arrays cda_nmt_verify takes for `samples` ((axis, index, pos, share, NMTProof) tuples of a 2k x 2k square):
    (descs, namespaces, nodes, leaves); roots are indexed rows first: row i -> i, column j -> 2k + j."""
    n = len(samples)
    descs = np.zeros(n, N.NMT_PROOF_DESC_DTYPE)
    namespaces = np.zeros((n, NAMESPACE_SIZE), np.uint8)
    leaves = np.zeros((n, N.SHARE_SIZE), np.uint8)
    nodes = []
    for i, (axis, index, pos, share, proof) in enumerate(samples):
        descs[i] = (proof.start, proof.end, len(nodes), len(proof.nodes), i, (2 * k if axis else 0) + index)
        namespaces[i] = np.frombuffer(sample_namespace(k, axis, index, pos, share), np.uint8)
        leaves[i] = np.frombuffer(bytes(share), np.uint8)
        nodes += [bytes(x) for x in proof.nodes]
    nodes = np.frombuffer(b"".join(nodes), np.uint8).reshape(-1, N.NODE_SIZE) if nodes else \
        np.zeros((0, N.NODE_SIZE), np.uint8)
    return descs, namespaces, nodes, leaves


def verify_samples(ctx, samples, row_roots, col_roots):
    """nmt.Proof.VerifyInclusion of every sample ((axis, index, pos, share, NMTProof): one cell each) against the
    square's roots, one launch.  -> list of bool."""
    if not samples:
        return []
    row_roots = np.ascontiguousarray(row_roots, np.uint8).reshape(-1, N.NODE_SIZE)
    col_roots = np.ascontiguousarray(col_roots, np.uint8).reshape(-1, N.NODE_SIZE)
    k = len(row_roots) // 2
    for axis, index, pos, share, proof in samples:
        if proof.end - proof.start != 1 or proof.start != pos or len(share) != N.SHARE_SIZE or \
                any(len(x) != N.NODE_SIZE for x in proof.nodes):
            raise ValueError("a sample is one 512-byte cell with the proof of [pos, pos + 1) in 90-byte nodes")
    descs, namespaces, nodes, leaves = pack_samples(samples, k)
    ok = ctx.nmt_verify(descs, namespaces, np.concatenate([row_roots, col_roots]), nodes, leaves)
    return [bool(x) for x in ok]
