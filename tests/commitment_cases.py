"""What tests/test_commitment_proofs.py (CPU) and tests/test_commitment_proofs_gpu.py share: squares whose blobs have a
namespace of their own, their trees from the oracle, and the named mutations that produce each verdict of rules C0-C8.
"""
import copy
import functools

import numpy as np

import oracle_lib as O
from cda import _native as N
from cda import commitment as C
from cda.inclusion import sub_tree_width

NS = 29


def aligned_blobs(k, threshold):
    """Every (start, len) of a k x k square that a blob may have under `threshold`."""
    return [(s, n) for s in range(k * k) for n in range(1, k * k - s + 1)
            if sub_tree_width(n, threshold) <= k and s % sub_tree_width(n, threshold) == 0]


def square_with_blobs(k, blobs, seed):
    """A k x k ODS in which every blob ((start, len), ascending, disjoint) and every gap between them has one
    namespace of its own, ascending in row-major order -> (ods, the blobs' namespaces)."""
    rng = np.random.default_rng(seed)
    ods = rng.integers(0, 256, (k * k, 512), dtype=np.uint8)
    bounds, cursor = [], 0
    for s, n in blobs:
        assert s >= cursor
        if s > cursor:
            bounds.append((cursor, s, None))
        bounds.append((s, s + n, (s, n)))
        cursor = s + n
    if cursor < k * k:
        bounds.append((cursor, k * k, None))
    names = {}
    for i, (lo, hi, blob) in enumerate(bounds):
        ns = bytes(NS - 4) + (i + 1).to_bytes(4, "big")
        ods[lo:hi, :NS] = np.frombuffer(ns, np.uint8)
        if blob:
            names[blob] = ns
    return ods, [names[b] for b in blobs]


class HostSquare:
    """The oracle's view of a square: the row trees of the ODS rows, rowRoots ‖ colRoots and the data root."""

    def __init__(self, ods):
        self.ods = ods
        self.k = int(round(len(ods) ** 0.5))
        rc, self.eds, rr, cr, self.dah = O.extend_commit(ods)
        assert rc == 0
        self.roots = [x.tobytes() for x in rr] + [x.tobytes() for x in cr]
        self.row_nodes = [O.tree_levels(O.axis_leaf_nodes(self.eds, 0, r)) for r in range(self.k)]
        self.data_root, self.row_proofs = C.merkle_proofs(self.roots)
        assert self.data_root == self.dah

    def prove(self, start, length, ns, threshold=64):
        return C.prove_host(self.row_nodes, self.roots, self.k, start, length, ns, threshold, self.row_proofs)


BASE_BLOBS = {1: [(0, 1)], 2: [(1, 2)], 4: [(3, 6)], 8: [(3, 12)], 16: [(3, 20)]}


@functools.lru_cache(maxsize=None)
def base_case(k):
    """A square with one blob that starts at an odd share and crosses a row (k = 1: its one share), proved at threshold
    64 (W = 1) -> dict(proof, data_root, commitment, threshold)."""
    (start, n), = BASE_BLOBS[k]
    ods, (ns,) = square_with_blobs(k, [(start, n)], 0xC0 + k)
    sq = HostSquare(ods)
    proof, commitment = sq.prove(start, n, ns, 64)
    return {"proof": proof, "data_root": sq.data_root, "commitment": commitment, "threshold": 64}


def _flip(b, i):
    out = bytearray(b)
    out[i % len(out)] ^= 0x10
    return bytes(out)


def _set(case, **kw):
    case.update(kw)


def _mut_range(c):
    c["proof"].row_proof.proofs[-1].index += 1


def _mut_root_count(c):
    c["proof"].rows[-1].subtree_roots.pop()


def _mut_namespace(c):
    c["proof"].namespace = _flip(c["proof"].namespace, 20)


def _mut_row_proof(c):
    a = c["proof"].row_proof.proofs[0].aunts
    a[0] = _flip(a[0], 5)


def _mut_subtree(c):
    nodes = c["proof"].rows[0].nmt.nodes
    nodes[-1] = _flip(nodes[-1], 70)  # a digest byte of the node behind the range: the namespaces stay in order


# (name, the verdict it produces, the mutation of a case), in the order of the rules.  "alignment" verifies the proof
# under threshold 1: W becomes 2 or more while the blob starts at an odd share (not at k = 1, where W is always 1).
MUTATIONS = [
    ("threshold zero", N.CP_MALFORMED, lambda c: _set(c, threshold=0)),
    ("end row + 1", N.CP_ROW_COUNT, lambda c: setattr(c["proof"].row_proof, "end_row", c["proof"].row_proof.end_row + 1)),
    ("last index + 1", N.CP_RANGE, _mut_range),
    ("threshold one", N.CP_ALIGNMENT, lambda c: _set(c, threshold=1)),
    ("subtree root dropped", N.CP_ROOT_COUNT, _mut_root_count),
    ("namespace byte", N.CP_NAMESPACE, _mut_namespace),
    ("aunt byte", N.CP_ROW_PROOF, _mut_row_proof),
    ("node digest byte", N.CP_SUBTREE_ROOTS, _mut_subtree),
    ("commitment byte", N.CP_COMMITMENT, lambda c: _set(c, commitment=_flip(c["commitment"], 9))),
]


def mutated(case, *names):
    """A deep copy of `case` with the named mutations applied."""
    out = copy.deepcopy(case)
    for name in names:
        next(fn for n, _, fn in MUTATIONS if n == name)(out)
    return out


def mutation_cases(k):
    """[(label, case, verdict)]: the valid base case, every mutation of it alone, and every pair of mutations, whose
    verdict is that of the earlier rule."""
    base = base_case(k)
    muts = [m for m in MUTATIONS if not (k == 1 and m[1] == N.CP_ALIGNMENT)]
    out = [("valid", copy.deepcopy(base), N.CP_VALID)]
    for name, verdict, _ in muts:
        out.append((name, mutated(base, name), verdict))
    for i, (a, va, _) in enumerate(muts):
        for b, _, _ in muts[i + 1:]:
            if {a, b} == {"threshold zero", "threshold one"}:
                continue  # both set the threshold
            out.append((f"{a} & {b}", mutated(base, a, b), va))
    return out


def host_verdict(case):
    return case["proof"].verify_host(case["data_root"], case["commitment"], case["threshold"])


def device_verdicts(ctx, cases):
    return C.verify_commitment_proofs(ctx, [c["proof"] for c in cases], [c["data_root"] for c in cases],
                                      [c["commitment"] for c in cases], [c["threshold"] for c in cases])
