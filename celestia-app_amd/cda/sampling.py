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


# ---- a square rebuilt from proved samples: place, repair, retain ----
PLACED, DUPLICATE, CONFLICT, REJECTED, MALFORMED = (N.SAMPLE_PLACED, N.SAMPLE_DUPLICATE, N.SAMPLE_CONFLICT,
                                                    N.SAMPLE_REJECTED, N.SAMPLE_MALFORMED)


def pack_sample_descs(samples):
    """The arrays cda_square_rebuild takes for `samples` ((axis, index, pos, share, NMTProof) tuples):
    (descs, shares, nodes).  Only the proof's nodes are used: the leaf is [pos, pos + 1) by the rule."""
    n = len(samples)
    descs = np.zeros(n, N.SAMPLE_DESC_DTYPE)
    shares = np.zeros((n, N.SHARE_SIZE), np.uint8)
    nodes = []
    for i, (axis, index, pos, share, proof) in enumerate(samples):
        if len(share) != N.SHARE_SIZE or any(len(x) != N.NODE_SIZE for x in proof.nodes):
            raise ValueError("a sample is one 512-byte cell with a proof in 90-byte nodes")
        descs[i] = (axis, index, pos, len(nodes), len(proof.nodes))
        shares[i] = np.frombuffer(bytes(share), np.uint8)
        nodes += [bytes(x) for x in proof.nodes]
    nodes = np.frombuffer(b"".join(nodes), np.uint8).reshape(-1, N.NODE_SIZE) if nodes else \
        np.zeros((0, N.NODE_SIZE), np.uint8)
    return descs, shares, nodes


def assemble_host(samples, row_roots, col_roots):
    """The placement rule (csrc/sample_place_rule.h) on the host, the mirror cda_samples_assemble_device is tested
    against: every sample is verified with NMTProof.verify_inclusion under the namespace of sample_namespace; the
    lowest-indexed verified sample of a cell is PLACED, every later verified one DUPLICATE or CONFLICT by its bytes.
    -> (eds ((2k)^2, 512) uint8, zero where nothing is placed; present ((2k)^2,) uint8; statuses (n,) uint8)."""
    w = len(row_roots)
    k = w // 2
    eds = np.zeros((w * w, N.SHARE_SIZE), np.uint8)
    present = np.zeros(w * w, np.uint8)
    statuses = np.zeros(len(samples), np.uint8)
    placed = {}
    for p, (axis, index, pos, share, proof) in enumerate(samples):
        if axis not in (0, 1) or not 0 <= index < w or not 0 <= pos < w:
            statuses[p] = MALFORMED
            continue
        share = bytes(share)
        root = bytes(col_roots[index]) if axis else bytes(row_roots[index])
        ns = sample_namespace(k, axis, index, pos, share)
        # the range is the rule's, not the message's: only the nodes of the carried proof are used
        if not NMTProof(pos, pos + 1, list(proof.nodes)).verify_inclusion(ns, [share], root):
            statuses[p] = REJECTED
            continue
        cell = pos * w + index if axis else index * w + pos
        if cell not in placed:
            placed[cell] = share
            eds[cell] = np.frombuffer(share, np.uint8)
            present[cell] = 1
            statuses[p] = PLACED
        else:
            statuses[p] = DUPLICATE if placed[cell] == share else CONFLICT
    return eds, present, statuses


def rebuild(ctx, samples, row_roots, col_roots, want_eds=False):
    """cda_square_rebuild over `samples`: verified, placed, repaired against the roots (rsmt2d Repair) and retained,
    without the square leaving the device.  -> (Square, statuses, present[, eds]).  When Repair fails CdaError carries
    the code (E_UNREPAIRABLE, E_BYZANTINE with axis and index) and, as attributes, statuses, present and eds."""
    descs, shares, nodes = pack_sample_descs(samples)
    rc, sq, statuses, present, eds, err = ctx.rebuild_square_status(descs, shares, nodes, row_roots, col_roots,
                                                                    want_eds)
    if rc != N.OK:
        e = N.CdaError(rc, axis=err.axis, index=err.index)
        e.statuses, e.present, e.eds = statuses, present, eds
        raise e
    return (sq, statuses, present, eds) if want_eds else (sq, statuses, present)
