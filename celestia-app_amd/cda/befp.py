"""Bad-encoding fraud proofs: build one from a retained square, validate batches on the device.

rsmt2d's Repair stops with ErrByzantineData{Axis, Index, Shares} when an axis it rebuilt does not hash to the committed
root (cda_repair: CDA_E_BYZANTINE with the axis and index).  Its consumer is the bad-encoding fraud proof (BEFP,
specs/src/specs/fraud_proofs.md:3-13, networking.md:66-92, proto/types.proto:233-259): at least k shares of that axis,
each with its NMT proof against the ORTHOGONAL root, from which any light client rebuilds the axis and sees that its
root is not the committed one.  The verifier of the reference stack lives in celestia-node, outside the pinned tree, so
the rule below (B1-B4) is this project's statement of it; the message shape and what the shares are
follow the spec and rsmt2d.

    create(square, axis, index)           the producer, for a node that holds the committed square (open_square_eds)
    from_samples(samples, axis, index, k) the producer, for a node that holds proved samples (cda.sampling.rebuild)
    validate_host(proof, rows, cols)      B1-B4 on the host (hashlib), the mirror the device form is tested against
    validate(ctx, proofs, roots)          cda_befp_validate: the whole batch in one call
"""
from dataclasses import dataclass

import numpy as np

from . import _native as N
from .proof import NMTProof
from .sampling import sample_namespace
from .wrapper import ErasuredNamespacedMerkleTree, PushError

FRAUD, NO_FRAUD, MALFORMED, TOO_FEW, BAD_SHARE = (N.BEFP_FRAUD, N.BEFP_NO_FRAUD, N.BEFP_MALFORMED, N.BEFP_TOO_FEW,
                                                  N.BEFP_BAD_SHARE)
ROW, COL = N.AXIS_ROW, N.AXIS_COL


@dataclass
class BadEncodingProof:
    """Axis (axis, index) of a square and `shares`: (pos, share bytes, NMTProof of leaf [index, index + 1) in the
    orthogonal tree `pos`) in increasing pos.  block: which (row_roots, col_roots) of a validate() call it is against."""
    axis: int
    index: int
    shares: list
    block: int = 0


def create(square, axis, index, positions=None):
    """The BEFP of axis (axis, index) of an open Square over the cells at `positions` (default: all 2k): one
    Square.prove call, each cell proved in its orthogonal tree."""
    w = 2 * square.k
    positions = list(range(w)) if positions is None else sorted(int(p) for p in positions)
    q = np.array([(1 - axis, pos, index, index + 1) for pos in positions], N.RANGE_QUERY_DTYPE)
    counts, nodes, cells = square.prove(q)
    return BadEncodingProof(int(axis), int(index),
                            [(pos, cells[i].tobytes(),
                              NMTProof(index, index + 1, [nodes[i, j].tobytes() for j in range(counts[i])]))
                             for i, pos in enumerate(positions)])


def from_samples(samples, axis, index, k):
    """The BEFP of axis (axis, index) of a 2k x 2k square out of samples a node already holds ((axis, index, pos,
    share, NMTProof) tuples, cda.sampling): those cells of the axis that were proved in their ORTHOGONAL trees, in
    increasing position, the first sample of a position standing for it.  -> BadEncodingProof, or None when fewer than
    k positions are covered (B2 would say TOO_FEW).  Nothing is verified here: validate does that."""
    by_pos = {}
    for s_axis, s_index, s_pos, share, nmt in samples:
        # leaf `index` of the orthogonal tree s_index is cell s_index of the axis
        if s_axis == 1 - axis and s_pos == index and 0 <= s_index < 2 * k:
            by_pos.setdefault(int(s_index), (bytes(share), nmt))
    if len(by_pos) < k:
        return None
    return BadEncodingProof(int(axis), int(index), [(pos,) + by_pos[pos] for pos in sorted(by_pos)])


def _orthogonal_root(proof, pos, row_roots, col_roots):
    return bytes(col_roots[pos]) if proof.axis == ROW else bytes(row_roots[pos])


def validate_host(proof, row_roots, col_roots, codec=None, reason=None):
    """B1-B4 of one proof against a block's 2k row roots and 2k column roots, on the host.  codec:
    encode(k shards) -> k parity shards, decode(2k shards or None) -> 2k shards (default: rsmt2d.LeoRSCodec).
    -> FRAUD, NO_FRAUD, MALFORMED, TOO_FEW or BAD_SHARE.  reason: a list that receives why B4 said FRAUD ("order": the
    tree could not be built, "root": its root differs); the two are one verdict, and which one it is depends on the
    decoder."""
    w = len(row_roots)
    k = w // 2
    # B1
    if proof.axis not in (ROW, COL) or not 0 <= proof.index < w or len(proof.shares) > w or len(col_roots) != w:
        return MALFORMED
    last = -1
    for pos, share, nmt in proof.shares:
        if not last < pos < w:
            return MALFORMED
        last = pos
    # B2
    if len(proof.shares) < k:
        return TOO_FEW
    # B3: every share in its orthogonal tree, as leaf `index`
    for pos, share, nmt in proof.shares:
        if len(share) != N.SHARE_SIZE:
            return BAD_SHARE
        ns = sample_namespace(k, proof.axis, proof.index, pos, share)
        # the range is the rule's, not the message's: only the nodes of the carried proof are used
        p = NMTProof(proof.index, proof.index + 1, list(nmt.nodes))
        if not p.verify_inclusion(ns, [share], _orthogonal_root(proof, pos, row_roots, col_roots)):
            return BAD_SHARE
    # B4: rebuild the axis from the shares, re-encode its parity half, and commit to it
    if codec is None:
        from .rsmt2d import LeoRSCodec
        codec = LeoRSCodec()
    slots = [None] * w
    for pos, share, nmt in proof.shares:
        slots[pos] = bytes(share)
    slots = [bytes(x) for x in codec.decode(slots)] if any(x is None for x in slots) else slots
    slots = slots[:k] + [bytes(x) for x in codec.encode(slots[:k])]
    tree = ErasuredNamespacedMerkleTree(k, proof.index)
    try:
        for cell in slots:
            tree.push(cell)
    except PushError:
        if reason is not None:
            reason.append("order")
        return FRAUD
    committed = bytes(row_roots[proof.index]) if proof.axis == ROW else bytes(col_roots[proof.index])
    if tree._root_node() == committed:
        return NO_FRAUD
    if reason is not None:
        reason.append("root")
    return FRAUD


def pack(proofs, k):
    """The arrays cda_befp_validate takes for `proofs` of 2k x 2k squares: (descs, entries, shares, nodes).  Block b's
    roots are roots[4k b : 4k (b + 1)], rows then columns."""
    descs = np.zeros(len(proofs), N.BEFP_DESC_DTYPE)
    n = sum(len(p.shares) for p in proofs)
    entries = np.zeros(n, N.BEFP_ENTRY_DTYPE)
    shares = np.zeros((n, N.SHARE_SIZE), np.uint8)
    nodes, e = [], 0
    for i, p in enumerate(proofs):
        descs[i] = (p.axis, p.index, e, len(p.shares), 4 * k * p.block)
        for pos, share, nmt in p.shares:
            if len(share) != N.SHARE_SIZE or any(len(x) != N.NODE_SIZE for x in nmt.nodes):
                raise ValueError("a BEFP entry is one 512-byte share with a proof in 90-byte nodes")
            entries[e] = (pos, len(nodes), len(nmt.nodes))
            shares[e] = np.frombuffer(bytes(share), np.uint8)
            nodes += [bytes(x) for x in nmt.nodes]
            e += 1
    nodes = np.frombuffer(b"".join(nodes), np.uint8).reshape(-1, N.NODE_SIZE) if nodes else \
        np.zeros((0, N.NODE_SIZE), np.uint8)
    return descs, entries, shares, nodes


def pack_roots(roots):
    """[(row_roots, col_roots)] -> (4k nblocks, 90) uint8, per block rows then columns."""
    return np.frombuffer(b"".join(bytes(r) for rc in roots for x in rc for r in x), np.uint8).reshape(-1, N.NODE_SIZE)


def validate(ctx, proofs, roots):
    """cda_befp_validate of `proofs` against roots[proof.block] = (row_roots, col_roots), one call.  -> list of verdict
    codes."""
    if not proofs:
        return []
    k = len(roots[0][0]) // 2
    return [int(v) for v in ctx.befp_validate(k, *pack(proofs, k), pack_roots(roots))]
