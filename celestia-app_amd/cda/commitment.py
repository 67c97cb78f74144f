"""Blob commitment proofs: "the blob with share commitment C is in the block with data root R", without the blob's
shares (celestia-app @ 2025-02-13, docs/architecture/adr-011: "Blob Inclusion Proof").

A proof carries, per row the blob touches, the subtree roots of the row's range (pkg/inclusion/paths.go's
coordinates: the inner nodes go-square's CreateCommitment hashes as mountains), the nodes of nmt ProveRange of that
range, and the row root with its RFC-6962 proof in the data root.  The verifier folds each row's subtree roots and
nodes to the row root, the row roots to the data root, and all subtree roots to the commitment.

Parity unpinned: the verifier's counterpart (VerifySubtreeRootInclusion) lives in celestia-node and nmt, outside the
reference tree; rules C0-C8 (include/cda.h CDA_CP_*) are this project's statement of it.  What is pinned:
the tiling (paths.go's test vectors), the commitment over the subtree roots (mainnet block 408's PFBs) and the data
root.  verify_host is the pure-Python statement of C0-C8 on hashlib; the device runs cda_commitment_proofs_verify.
"""
from dataclasses import dataclass, field

import numpy as np

from . import _native as N
from . import appconsts
from .inclusion import sub_tree_width
from .proof import NMTProof, Proof, ProofError, RowProof, _sha256, _split_point

NS = appconsts.NAMESPACE_SIZE
MAX_K = 32768          # the widest ODS the codec accepts
MAX_ROOTS = 1 << 18    # subtree roots of one proof the device folds (commitment_rule.h kCommitMaxRoots)


def subtree_tiles(s, e, W):
    """The greedy tiling of a row's range [s, e) under subtree width W -> [(cursor, size)]: at cursor c the largest
    power of two z <= W with c % z == 0 and c + z <= e.  The tile of size 2^h at c is node (h, c >> h) of the row
    tree."""
    out, c = [], s
    while c < e:
        z = W
        while z > 1 and (c % z or c + z > e):
            z //= 2
        out.append((c, z))
        c += z
    return out


def blob_rows(k, start, length):
    """The rows of the ODS range [start, start + length) of a k x k square -> [(row, s, e)]."""
    end = start + length
    r0, r1 = start // k, (end - 1) // k
    return [(r, start % k if r == r0 else 0, (end - 1) % k + 1 if r == r1 else k) for r in range(r0, r1 + 1)]


def _nmt_node(left, right):
    """nmt HashNode with IgnoreMaxNamespace -> (node, siblings in order)."""
    parity = b"\xff" * NS
    mx = left[NS:2 * NS] if right[:NS] == parity else right[NS:2 * NS]
    return left[:NS] + mx + _sha256(b"\x01", left, right), left[NS:2 * NS] <= right[:NS]


def fold_row(s, e, W, leaves, roots, nodes, trace=None):
    """A row's subtree roots (left to right) and the nodes of ProveRange(s, e) folded to the root of the tree of
    `leaves` leaves, by nmt's recursion: recompute the subtree, taking a subtree root whenever the recursion's range
    is the next tile, otherwise splitting, and taking a proof node for every subtree outside the range.  -> the root,
    or None if a root or node is missing or left over, or siblings are out of namespace order.  trace (a list) gets
    ("R" | "N", index, level, position) for every root and node in the order they are taken."""
    tiles = subtree_tiles(s, e, W)
    state = {"r": 0, "n": 0, "bad": False}

    def take(kind, items, lo, hi):
        i = state[kind]
        state[kind] += 1
        if trace is not None:
            level = (hi - lo).bit_length() - 1
            trace.append(("R" if kind == "r" else "N", i, level, lo >> level))
        return bytes(items[i]) if i < len(items) else None

    def compute(lo, hi):
        if hi <= s or lo >= e:
            return take("n", nodes, lo, hi)
        if state["r"] < len(tiles) and tiles[state["r"]] == (lo, hi - lo):
            return take("r", roots, lo, hi)
        if hi - lo == 1:
            return None  # a leaf of the range that no tile covers: not a tiling
        mid = lo + (hi - lo) // 2
        left, right = compute(lo, mid), compute(mid, hi)
        if left is None or right is None:
            return None
        node, ordered = _nmt_node(left, right)
        state["bad"] = state["bad"] or not ordered
        return node

    top = compute(0, leaves)
    if top is None or state["bad"] or state["r"] != len(roots) or state["n"] != len(nodes):
        return None
    return top


def merkle_root(items):
    """merkle.HashFromByteSlices."""
    if not items:
        return _sha256(b"")
    if len(items) == 1:
        return _sha256(b"\x00", bytes(items[0]))
    k = _split_point(len(items))
    return _sha256(b"\x01", merkle_root(items[:k]), merkle_root(items[k:]))


def merkle_proofs(items):
    """merkle.ProofsFromByteSlices -> (root, [Proof]) with the aunts bottom-up."""
    def trails(lo, hi):
        if hi - lo == 1:
            return _sha256(b"\x00", bytes(items[lo])), [[]]
        k = _split_point(hi - lo)
        lroot, lt = trails(lo, lo + k)
        rroot, rt = trails(lo + k, hi)
        return _sha256(b"\x01", lroot, rroot), [t + [rroot] for t in lt] + [t + [lroot] for t in rt]
    root, tr = trails(0, len(items))
    return root, [Proof(len(items), i, _sha256(b"\x00", bytes(items[i])), t) for i, t in enumerate(tr)]


@dataclass
class CommitmentRow:
    """One row of a commitment proof: the subtree roots of the row's range, left to right, and nmt ProveRange of it."""
    subtree_roots: list
    nmt: NMTProof


@dataclass
class CommitmentProof:
    namespace: bytes             # NamespaceVersion ‖ NamespaceID, 29 bytes
    rows: list = field(default_factory=list)
    row_proof: RowProof = None

    def subtree_roots(self):
        return [bytes(x) for r in self.rows for x in r.subtree_roots]

    def verify_host(self, data_root, commitment, threshold=appconsts.SUBTREE_ROOT_THRESHOLD):
        """Rules C0-C8 -> CP_VALID or the first rule that fails (the verdict cda_commitment_proofs_verify gives)."""
        rp, rows, n = self.row_proof, self.rows, len(self.rows)
        if len(rp.row_roots) != n or len(rp.proofs) != n:
            raise ValueError("a commitment proof has one row root and one row proof per row")
        if n == 0 or threshold == 0 or sum(len(r.subtree_roots) for r in rows) > MAX_ROOTS:
            return N.CP_MALFORMED
        if rp.end_row - rp.start_row + 1 != n:
            return N.CP_ROW_COUNT
        total = rp.proofs[0].total
        k = total // 4
        if total <= 0 or total % 4 or k & (k - 1) or k > MAX_K:
            return N.CP_RANGE
        for i, (r, p) in enumerate(zip(rows, rp.proofs)):
            s, e = r.nmt.start, r.nmt.end
            if p.total != total or p.index != rp.start_row + i or s < 0 or s >= e or e > k or (i and s) or \
                    (i + 1 < n and e != k):
                return N.CP_RANGE
        W = sub_tree_width(sum(r.nmt.end - r.nmt.start for r in rows), threshold)
        if W > k or rows[0].nmt.start % W:
            return N.CP_ALIGNMENT
        if any(len(r.subtree_roots) != len(subtree_tiles(r.nmt.start, r.nmt.end, W)) for r in rows):
            return N.CP_ROOT_COUNT
        ns = bytes(self.namespace)
        if any(bytes(x[:NS]) != ns or bytes(x[NS:2 * NS]) != ns for x in self.subtree_roots()):
            return N.CP_NAMESPACE
        for p, rr in zip(rp.proofs, rp.row_roots):
            try:
                p.verify(data_root, rr)
            except ProofError:
                return N.CP_ROW_PROOF
        for r, rr in zip(rows, rp.row_roots):
            if fold_row(r.nmt.start, r.nmt.end, W, 2 * k, r.subtree_roots, r.nmt.nodes) != bytes(rr):
                return N.CP_SUBTREE_ROOTS
        return N.CP_VALID if merkle_root(self.subtree_roots()) == bytes(commitment) else N.CP_COMMITMENT


def tree_node(tree, w, h, pos):
    """Node (height h, position pos) of a row tree exported as 2w - 1 nodes: the w leaves, each level, the root."""
    return bytes(tree[sum(w >> i for i in range(h)) + pos])


def prove_host(row_nodes, roots, k, start, length, namespace, threshold=appconsts.SUBTREE_ROOT_THRESHOLD,
               row_proofs=None):
    """The commitment proof of the blob at ODS shares [start, start + length) over exported tree nodes.  row_nodes[r]:
    the 4k - 1 nodes of row tree r (cda_extend_commit_nodes' row_nodes); roots: rowRoots ‖ colRoots (4k nodes of 90 B);
    row_proofs: merkle_proofs(roots)[1] if the caller has them.  -> (CommitmentProof, commitment)."""
    if length <= 0 or threshold <= 0 or start < 0 or start + length > k * k:
        raise ValueError("the blob does not lie in the square")
    W = sub_tree_width(length, threshold)
    if W > k or start % W:
        raise ValueError(f"a blob of {length} shares starts at a multiple of {W} no greater than the square")
    w = 2 * k
    if row_proofs is None:
        row_proofs = merkle_proofs(roots)[1]
    rows, rr, proofs = [], [], []
    for row, s, e in blob_rows(k, start, length):
        tree = row_nodes[row]
        sub = [tree_node(tree, w, z.bit_length() - 1, c // z) for c, z in subtree_tiles(s, e, W)]
        left = [tree_node(tree, w, b, (s >> b) - 1) for b in range(w.bit_length(), -1, -1) if s >> b & 1]
        r = w - e
        right = [tree_node(tree, w, b, (w >> b) - (r >> b)) for b in range(w.bit_length() + 1) if r >> b & 1]
        rows.append(CommitmentRow(sub, NMTProof(s, e, left + right)))
        rr.append(bytes(roots[row]))
        proofs.append(row_proofs[row])
    proof = CommitmentProof(bytes(namespace), rows, RowProof(rr, proofs, start // k, (start + length - 1) // k))
    return proof, merkle_root(proof.subtree_roots())


def proofs_from_raw(raw, namespaces):
    """The flat arrays cda_square_commitment_proofs wrote (Square.commitment_proofs_raw) -> [CommitmentProof]."""
    rows, out = raw["rows"], []
    for q in range(len(raw["row_off"]) - 1):
        lo, hi = int(raw["row_off"][q]), int(raw["row_off"][q + 1])
        rs = [CommitmentRow([raw["subtree_roots"][int(rows[r]["root_off"]) + j].tobytes()
                             for j in range(int(rows[r]["nroots"]))],
                            NMTProof(int(rows[r]["nmt_start"]), int(rows[r]["nmt_end"]),
                                     [raw["nodes"][r, j].tobytes() for j in range(int(rows[r]["nnodes"]))]))
              for r in range(lo, hi)]
        rp = RowProof([raw["row_roots"][r].tobytes() for r in range(lo, hi)],
                      [Proof(int(rows[r]["total"]), int(rows[r]["index"]), raw["leaf_hashes"][r].tobytes(),
                             [raw["aunts"][r, j].tobytes() for j in range(int(rows[r]["naunts"]))])
                       for r in range(lo, hi)], int(rows[lo]["row"]), int(rows[hi - 1]["row"]))
        out.append(CommitmentProof(bytes(namespaces[q]), rs, rp))
    return out


def pack_commitment_proofs(proofs, root_index, commitment_index, thresholds):
    """The flat arrays cda_commitment_proofs_verify takes for `proofs` (proof i verifies against data root
    root_index[i] and commitment commitment_index[i] under thresholds[i]) -> dict(descs, rows, row_roots, leaf_hashes,
    nodes, subtree_roots, aunts).  Sizes the C records cannot hold raise ValueError."""
    NODE = N.NODE_SIZE

    def sized(x, n, what):
        x = bytes(x)
        if len(x) != n:
            raise ValueError(f"{what} of {len(x)} bytes: cda_commitment_proofs_verify takes {n}")
        return x
    descs = np.zeros(len(proofs), N.COMMITMENT_PROOF_DESC_DTYPE)
    rows = np.zeros(sum(len(p.rows) for p in proofs), N.COMMITMENT_ROW_DTYPE)
    row_roots = np.zeros((len(rows), NODE), np.uint8)
    leaf_hashes = np.zeros((len(rows), 32), np.uint8)
    nodes, sub, aunts, r = [], [], [], 0
    for i, p in enumerate(proofs):
        rp = p.row_proof
        if len(rp.row_roots) != len(p.rows) or len(rp.proofs) != len(p.rows):
            raise ValueError("a commitment proof has one row root and one row proof per row")
        ns = sized(p.namespace, NS, "namespace")
        descs[i] = (r, len(p.rows), rp.start_row, rp.end_row, root_index[i], commitment_index[i], thresholds[i],
                    np.frombuffer(ns, np.uint8), 0)
        for row, rr, mp in zip(p.rows, rp.row_roots, rp.proofs):
            rows[r] = (row.nmt.start, row.nmt.end, len(nodes), len(row.nmt.nodes), len(sub), len(row.subtree_roots),
                       mp.total, mp.index, len(aunts), len(mp.aunts), 0, 0)
            nodes += [sized(x, NODE, "node") for x in row.nmt.nodes]
            sub += [sized(x, NODE, "subtree root") for x in row.subtree_roots]
            aunts += [sized(x, 32, "aunt") for x in mp.aunts]
            row_roots[r] = np.frombuffer(sized(rr, NODE, "row root"), np.uint8)
            leaf_hashes[r] = np.frombuffer(sized(mp.leaf_hash, 32, "leaf hash"), np.uint8)
            r += 1

    def flat(items, n):
        return np.frombuffer(b"".join(items), np.uint8).reshape(-1, n) if items else np.zeros((0, n), np.uint8)
    return {"descs": descs, "rows": rows, "row_roots": row_roots, "leaf_hashes": leaf_hashes,
            "nodes": flat(nodes, NODE), "subtree_roots": flat(sub, NODE), "aunts": flat(aunts, 32)}


def verify_commitment_proofs(ctx, proofs, data_roots, commitments, threshold=appconsts.SUBTREE_ROOT_THRESHOLD):
    """CommitmentProof.verify_host of every proof on the device, one call (cda_commitment_proofs_verify).  data_roots:
    one root for all proofs (bytes) or one per proof; commitments: one per proof; threshold: one for all or one per
    proof.  -> the CP_* verdict of each proof."""
    proofs = list(proofs)
    if not proofs:
        return []
    roots = [bytes(data_roots)] * len(proofs) if isinstance(data_roots, (bytes, bytearray)) else \
        [bytes(x) for x in data_roots]
    coms = [bytes(x) for x in commitments]
    thr = [int(threshold)] * len(proofs) if isinstance(threshold, int) else [int(x) for x in threshold]
    if len(roots) != len(proofs) or len(coms) != len(proofs) or len(thr) != len(proofs) or \
            any(len(x) != 32 for x in roots + coms):
        raise ValueError("one 32-byte data root or one per proof, one 32-byte commitment and one threshold per proof")
    uniq = {}
    index = [uniq.setdefault(x, len(uniq)) for x in roots]
    a = pack_commitment_proofs(proofs, index, list(range(len(proofs))), thr)
    verdicts = ctx.commitment_proofs_verify(a["descs"], a["rows"], a["row_roots"], a["leaf_hashes"], a["nodes"],
                                            a["subtree_roots"], a["aunts"],
                                            np.frombuffer(b"".join(uniq), np.uint8).reshape(-1, 32),
                                            np.frombuffer(b"".join(coms), np.uint8).reshape(-1, 32))
    return [int(v) for v in verdicts]
