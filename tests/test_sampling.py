"""CPU tests of the sample-proof feature (cda_square_*, cda_nmt_verify): the stack-free index rule the verify kernels
evaluate (csrc/nmt_verify_rule.h, plan::verify_walk) against cda.proof.NMTProof.verify_inclusion, and the argument
checks of the new entry points.  No GPU.
"""
import ctypes
import hashlib
import os
import random
import subprocess

import pytest

import cda
from cda import _native as N
from cda.appconsts import NAMESPACE_SIZE, PARITY_SHARES_NAMESPACE
from cda.proof import NMTProof, _split_point
from cda.wrapper import ErasuredNamespacedMerkleTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = NAMESPACE_SIZE


# ---- the index rule, restated (csrc/nmt_verify_rule.h) ----
def walk(start, end, nnodes):
    """plan::verify_walk: the schedule of nmt Proof.VerifyInclusion by index arithmetic.  None when the proof has
    fewer nodes than the left hull needs, else a list of steps (level, lo, hi, left, right): the span of level
    `level` is nodes [lo, hi) after node `left` was put in front of it (-1: none) and node `right` behind it
    (-1: none; an odd last node is then passed up unchanged), followed by the index of the first node applied above
    the subtree of 2 * splitpoint(end) leaves."""
    lp = rp = bin(start).count("1")
    if nnodes < lp:
        return None
    top = max(1, 2 * _split_point(end))
    lo, hi, steps, level = start, end, [], 0
    while (1 << level) < top:
        left = right = -1
        if lo & 1:
            lp -= 1
            left, lo = lp, lo - 1
        if hi & 1 and rp < nnodes:
            right, rp, hi = rp, rp + 1, hi + 1
        steps.append((level, lo, hi, left, right))
        lo, hi, level = lo >> 1, (hi + 1) >> 1, level + 1
    return steps, rp


def _node(left, right, state):
    if left[NS:2 * NS] > right[:NS]:
        state["bad"] = True
    mx = left[NS:2 * NS] if right[:NS] == PARITY_SHARES_NAMESPACE else right[NS:2 * NS]
    return left[:NS] + mx + hashlib.sha256(b"\x01" + left + right).digest()


def rule_verify(start, end, nodes, namespace, leaves, root):
    """verify_inclusion by the index rule: what cda_nmt_verify computes."""
    if start >= end or end - start != len(leaves):
        return False
    w = walk(start, end, len(nodes))
    if w is None:
        return False
    steps, rp = w
    ns = bytes(namespace)
    span = [ns + ns + hashlib.sha256(b"\x00" + ns + bytes(x)).digest() for x in leaves]
    state = {"bad": False}
    for _, lo, hi, left, right in steps:
        if left >= 0:
            span.insert(0, bytes(nodes[left]))
        if right >= 0:
            span.append(bytes(nodes[right]))
        assert len(span) == hi - lo
        nxt = [_node(span[i], span[i + 1], state) for i in range(0, len(span) - 1, 2)]
        if len(span) & 1:
            nxt.append(span[-1])
        span = nxt
    assert len(span) == 1
    h = span[0]
    for x in nodes[rp:]:
        h = _node(h, bytes(x), state)
    return not state["bad"] and h == bytes(root)


# ---- trees and mutations shared with the GPU test ----
def tree_root(leaf_nodes):
    """nmt root of the leaf nodes (split at the largest power of two below n), hashlib."""
    def rec(lo, hi):
        if hi - lo == 1:
            return leaf_nodes[lo]
        k = _split_point(hi - lo)
        return _node(rec(lo, lo + k), rec(lo + k, hi), {"bad": False})
    return rec(0, len(leaf_nodes))


def make_tree(rng, n):
    """An erasured tree of n leaves (any n): square_size sq Q0 leaves in namespace order, the rest parity."""
    sq = rng.randint(1, n)
    axis_index = rng.choice([0, sq])  # a Q0 axis or an all-parity one
    pool = sorted(bytes([0]) + bytes(rng.getrandbits(8) for _ in range(NS - 1)) for _ in range(rng.randint(1, 3)))
    nss = sorted(rng.choice(pool) for _ in range(n))
    t = ErasuredNamespacedMerkleTree(sq, axis_index)
    t._leaves = [nss[i] + bytes(rng.getrandbits(8) for _ in range(16)) * ((512 - NS) // 16 + 1) for i in range(n)]
    t._leaves = [x[:512] for x in t._leaves]
    return t


def leaf_ns(t, i):
    q0 = i < t.square_size and t.axis_index < t.square_size
    return t._leaves[i][:NS] if q0 else PARITY_SHARES_NAMESPACE


MUTATIONS = ("valid", "drop_last", "drop_first", "append", "swap", "flip_leaf", "flip_node", "flip_root", "wrong_ns",
             "shift", "leaf_order")


def _flip(b, rng):
    i = rng.randrange(len(b) * 8)
    out = bytearray(b)
    out[i >> 3] ^= 1 << (i & 7)
    return bytes(out)


def mutate(rng, kind, t, start, end, root):
    """-> (start, end, nodes, namespace, leaves, root) of one case, or None where the mutation does not apply."""
    p = t.prove_range(start, end)
    nodes, leaves, ns = list(p.nodes), [t._leaves[i] for i in range(start, end)], leaf_ns(t, start)
    n = len(t._leaves)
    if kind == "drop_last":
        if not nodes:
            return None
        nodes.pop()
    elif kind == "drop_first":
        if not nodes:
            return None
        nodes.pop(0)
    elif kind == "append":
        nodes.append(rng.choice(nodes) if nodes else root)
    elif kind == "swap":
        if len(nodes) < 2:
            return None
        i = rng.randrange(len(nodes) - 1)
        nodes[i], nodes[i + 1] = nodes[i + 1], nodes[i]
    elif kind == "flip_leaf":
        i = rng.randrange(len(leaves))
        leaves[i] = _flip(leaves[i], rng)
    elif kind == "flip_node":
        if not nodes:
            return None
        i = rng.randrange(len(nodes))
        nodes[i] = _flip(nodes[i], rng)
    elif kind == "flip_root":
        root = _flip(root, rng)
    elif kind == "wrong_ns":
        ns = _flip(ns, rng)
    elif kind == "shift":
        up, down = end + 1 <= n, start > 0
        if not (up or down):
            return None
        d = 1 if up and (not down or rng.random() < 0.5) else -1
        start, end = start + d, end + d
    elif kind == "leaf_order":
        if len(leaves) < 2:
            return None
        leaves[0], leaves[-1] = leaves[-1], leaves[0]
    return start, end, nodes, ns, leaves, root


def cases(seed, count):
    """`count` cases over trees of 1..32 leaves: every mutation kind in turn, valid proofs in between."""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        n = rng.randint(1, 32)
        t = make_tree(rng, n)
        root = tree_root(t._leaf_nodes())
        for _ in range(8):
            start = rng.randrange(n)
            end = rng.randint(start + 1, min(n, start + rng.choice([1, 1, 2, 3, n])))
            kind = "valid" if rng.random() < 0.4 else rng.choice(MUTATIONS[1:])
            c = mutate(rng, kind, t, start, end, root)
            if c is not None:
                out.append((kind,) + c)
    return out[:count]


def test_index_rule_matches_verify_inclusion():
    """The rule the kernels evaluate gives verify_inclusion's verdict on valid and mutated proofs of trees of 1..32
    leaves (leaf counts that are no power of two included)."""
    accepted = rejected = 0
    kinds = set()
    for kind, start, end, nodes, ns, leaves, root in cases(0x5A3D1E, 3000):
        want = NMTProof(start, end, nodes).verify_inclusion(ns, leaves, root)
        assert rule_verify(start, end, nodes, ns, leaves, root) == want, (kind, start, end, len(nodes))
        accepted += want
        rejected += not want
        kinds.add(kind)
    assert kinds == set(MUTATIONS)
    assert accepted >= 100 and rejected >= 100, (accepted, rejected)


def test_every_valid_single_namespace_proof_verifies():
    """prove_range's own proofs of one-namespace ranges are accepted (so the fuzz's accepted side is not empty by
    construction), for every range of every tree size 1..32."""
    rng = random.Random(7)
    for n in range(1, 33):
        t = make_tree(rng, n)
        root = tree_root(t._leaf_nodes())
        for start in range(n):
            for end in range(start + 1, n + 1):
                ns = leaf_ns(t, start)
                if any(leaf_ns(t, i) != ns for i in range(start, end)):
                    continue
                p = t.prove_range(start, end)
                leaves = t._leaves[start:end]
                assert p.verify_inclusion(ns, leaves, root)
                assert rule_verify(start, end, p.nodes, ns, leaves, root), (n, start, end)


def test_plan_verify_walk_is_the_restated_rule(tmp_path):
    """plan::verify_walk (csrc/plan.cpp, built with plain g++ as the sanitizer builds do) emits the schedule `walk`
    restates, for every range and node count of trees up to 64 leaves."""
    exe = str(tmp_path / "verify_walk_dump")
    csrc = os.path.join(ROOT, "celestia-app_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "san", "verify_walk_dump.cpp"), os.path.join(csrc, "plan.cpp")])
    got = subprocess.check_output([exe, "64"], text=True).splitlines()
    want = []
    for end in range(1, 65):
        for start in range(end):
            for nn in range(0, 14):
                w = walk(start, end, nn)
                if w is None:
                    want.append(f"{start} {end} {nn} reject")
                    continue
                steps, rp = w
                want.append(f"{start} {end} {nn} " + " ".join("%d:%d:%d:%d:%d" % s for s in steps) + f" tail {rp}")
    assert got == want


def test_sampling_entry_points_reject_bad_arguments_without_gpu():
    """Argument checks run before any device work: negative codes, no abort."""
    L = cda.lib()
    assert L.cda_square_open(None, 4, 512, None, None, None, None, None, None) == N.E_ARG
    assert L.cda_square_prove(None, 1, None, 2, None, None, None, 0) == N.E_ARG
    L.cda_square_close(None)  # a null handle is ignored
    assert L.cda_nmt_verify(None, 1, None, None, None, 1, None, 0, None, 1, None) == N.E_ARG
    assert L.cda_nmt_verify_device(None, 1, None, None, None, 1, None, 0, None, 1, None, None) == N.E_ARG
    # the exception barrier covers the new entry points too (test-hooks build)
    H = N.lib(N.HOOKS_LIB_PATH)
    os.environ["CDA_FAULT_INJECT"] = "entry"
    try:
        assert H.cda_square_open(None, 4, 512, None, None, None, None, None, None) == N.E_NOMEM
        assert H.cda_square_prove(None, 1, None, 2, None, None, None, 0) == N.E_NOMEM
        assert H.cda_nmt_verify(None, 1, None, None, None, 1, None, 0, None, 1, None) == N.E_NOMEM
        assert H.cda_nmt_verify_device(None, 1, None, None, None, 1, None, 0, None, 1, None, None) == N.E_NOMEM
    finally:
        del os.environ["CDA_FAULT_INJECT"]


@pytest.mark.parametrize("kernel", ["nmt_verify_cells_kernel", "nmt_verify_ranges_kernel", "square_prove_kernel"])
def test_sampling_kernels_register_budget(kernel, tmp_path):
    """The budget tests/test_hash_kernel_registers.py holds the hash kernels to, for the new kernels: at most 128
    VGPRs (4 waves per SIMD), no spilled VGPR, no private segment -- read from the built library's metadata."""
    import test_hash_kernel_registers as R
    if not (os.path.exists(R.V.OBJDUMP) and os.path.exists(R.READOBJ) and os.path.exists(R.LIB)):
        pytest.skip("needs llvm-objdump, llvm-readobj and the built libcda.so")
    found = {n: m for n, m in R.kernel_metadata(R.LIB, str(tmp_path)).items() if kernel in n}
    assert len(found) == 1, sorted(found)
    (name, m), = found.items()
    print(name, m)
    assert m["vgpr_count"] <= 128 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m


def test_sampling_structs_match_header():
    assert ctypes.sizeof(N.RangeQuery) == 16
    assert ctypes.sizeof(N.NmtProofDesc) == 24
    assert N.RANGE_QUERY_DTYPE.itemsize == 16 and N.NMT_PROOF_DESC_DTYPE.itemsize == 24


def test_sample_namespace_is_the_quadrant_rule():
    from cda import sampling
    share = bytes(range(1, 30)) + bytes(483)
    assert sampling.sample_namespace(4, 0, 1, 2, share) == share[:NS]
    assert sampling.sample_namespace(4, 0, 1, 4, share) == PARITY_SHARES_NAMESPACE
    assert sampling.sample_namespace(4, 1, 1, 5, share) == PARITY_SHARES_NAMESPACE
    assert sampling.sample_namespace(4, 1, 3, 3, share) == share[:NS]
    assert sampling.sample_namespace(4, 0, 4, 0, share) == PARITY_SHARES_NAMESPACE
