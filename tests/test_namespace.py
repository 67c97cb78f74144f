"""CPU tests of namespace data with completeness proofs (cda_square_prove_namespace, cda_nmt_verify_namespace): the
host mirror (wrapper.prove_namespace, NMTProof.verify_namespace) against the rules of DESIGN §18, the C++ rule the
kernels share (csrc/nmt_namespace_rule.h through plan::namespace_bounds / plan::namespace_precheck, built alone under
AddressSanitizer and UBSan) against the mirror over valid and mutated proofs, and the shape of the new ABI.  No GPU.
"""
import ctypes
import hashlib
import os
import random
import subprocess

import pytest

import cda
import test_sampling as TS
from cda import _native as N
from cda.appconsts import NAMESPACE_SIZE, PARITY_SHARES_NAMESPACE
from cda.proof import NMTProof
from cda.wrapper import ErasuredNamespacedMerkleTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "celestia-app_amd", "csrc")
NS = NAMESPACE_SIZE
EMPTY, INCLUSION, ABSENCE = "empty", "inclusion", "absence"
NEW_KERNELS = ["square_prove_namespace_kernel", "namespace_share_offsets_kernel", "namespace_shares_kernel",
               "ns_verify_prep_kernel", "ns_verify_absence_kernel", "ns_verify_combine_kernel"]


# ---- trees, namespaces to ask for, and what the rules say about them ----
def ns_add(ns, d):
    """The namespace d steps after ns as a 29-byte big-endian number; None outside [0, 2^232)."""
    v = int.from_bytes(ns, "big") + d
    return v.to_bytes(NS, "big") if 0 <= v < 1 << (8 * NS) else None


def make_tree6(rng, n):
    """TS.make_tree with up to 6 distinct namespaces, each a run of leaves."""
    sq = rng.randint(1, n)
    axis_index = rng.choice([0, 0, sq])
    pool = sorted(bytes([0]) + bytes(rng.getrandbits(8) for _ in range(NS - 1)) for _ in range(rng.randint(1, 6)))
    nss = sorted(rng.choice(pool) for _ in range(n))
    t = ErasuredNamespacedMerkleTree(sq, axis_index)
    t._leaves = [(nss[i] + bytes(rng.getrandbits(8) for _ in range(16)) * 31)[:512] for i in range(n)]
    return t


def leaf_namespaces(t):
    return [TS.leaf_ns(t, i) for i in range(len(t._leaves))]


def nid_set(t):
    """The namespaces the tests ask a tree for: every present one, one below the minimum, one strictly between each
    adjacent pair, one above the Q0 maximum, and 0xFF x 29."""
    present = sorted(set(leaf_namespaces(t)))
    out = list(present)
    out.append(ns_add(present[0], -1))
    for a, b in zip(present, present[1:]):
        mid = ns_add(a, 1)
        out.append(mid if mid < b else None)
    q0 = [x for x in present if x != PARITY_SHARES_NAMESPACE]
    if q0:
        out.append(ns_add(q0[-1], 1))
    out.append(PARITY_SHARES_NAMESPACE)
    return sorted(set(x for x in out if x is not None))


def kind_by_the_rules(t, nid, root):
    """P1-P3 restated: (kind, start, end)."""
    lns = leaf_namespaces(t)
    if nid < root[:NS] or nid > root[NS:2 * NS]:
        return EMPTY, 0, 0
    if nid in lns:
        return INCLUSION, lns.index(nid), len(lns) - lns[::-1].index(nid)
    start = next(i for i, x in enumerate(lns) if x > nid)
    return ABSENCE, start, start + 1


def proof_kind(p):
    return EMPTY if p.start == p.end else (ABSENCE if p.leaf_hash else INCLUSION)


def trees(seed):
    """Trees of 1..32 leaves, one of each maker per size."""
    rng = random.Random(seed)
    for n in range(1, 33):
        yield TS.make_tree(rng, n)
        yield make_tree6(rng, n)


# ---- the mirror against the rules ----
def test_prove_namespace_kind_and_verify_namespace_accepts():
    """For every tree and every namespace of nid_set: prove_namespace gives the kind, range, nodes and leaf_hash the
    rules say, and verify_namespace accepts the proof with the run's leaves."""
    seen = set()
    for t in trees(0x4E53):
        root = TS.tree_root(t._leaf_nodes())
        assert t._root_node() == root
        for nid in nid_set(t):
            kind, start, end = kind_by_the_rules(t, nid, root)
            p = t.prove_namespace(nid)
            assert (proof_kind(p), p.start, p.end) == (kind, start, end)
            assert p.is_empty() == (kind == EMPTY) and p.is_of_absence() == (kind == ABSENCE)
            if kind == EMPTY:
                assert p.nodes == [] and not p.leaf_hash
            else:
                assert p.nodes == t.prove_range(start, end).nodes
                assert bytes(p.leaf_hash) == (t._leaf_nodes()[start] if kind == ABSENCE else b"")
            leaves = t._leaves[start:end] if kind == INCLUSION else []
            assert p.verify_namespace(nid, leaves, root), (len(t._leaves), kind, start, end)
            seen.add(kind)
    assert seen == {EMPTY, INCLUSION, ABSENCE}
    assert NMTProof(0, 0, []).verify_namespace(bytes(NS), [], bytes(2 * NS) + hashlib.sha256(b"").digest())


def test_partial_run_passes_verify_inclusion_and_fails_verify_namespace():
    """V5: the proof of a strict sub-range of a namespace's run is a valid inclusion proof of those leaves and is
    rejected as a namespace proof -- at either end of the run."""
    checked = 0
    for t in trees(0x5635):
        root = TS.tree_root(t._leaf_nodes())
        for nid in sorted(set(leaf_namespaces(t))):
            _, start, end = kind_by_the_rules(t, nid, root)
            if nid > root[NS:2 * NS] or end - start < 2:
                continue
            for s, e in ((start + 1, end), (start, end - 1), (start + 1, start + 2) if end - start > 2 else (start, end)):
                p = t.prove_range(s, e)
                leaves = t._leaves[s:e]
                assert p.verify_inclusion(nid, leaves, root)
                assert p.verify_namespace(nid, leaves, root) == ((s, e) == (start, end)), (len(t._leaves), s, e)
                checked += (s, e) != (start, end)
    assert checked >= 100


# ---- valid and mutated proofs, shared with the GPU test ----
MUTATIONS = ("valid", "drop_node", "append_node", "swap_nodes", "flip_node", "shift", "widen", "narrow", "swap_lr",
             "absence_prev_leaf", "leaf_hash_on_inclusion", "leaves_on_empty", "leaves_on_absence", "min_gt_max")


def mutate(rng, kind, t, p, leaves, root):
    """-> (start, end, nodes, leaf_hash, leaves, root) of one case, or None where the mutation does not apply."""
    start, end, nodes, lh, leaves = p.start, p.end, list(p.nodes), bytes(p.leaf_hash or b""), list(leaves)
    n, leaf_nodes, nl = len(t._leaves), t._leaf_nodes(), bin(p.start).count("1")
    if kind == "drop_node":
        if not nodes:
            return None
        nodes.pop(rng.randrange(len(nodes)))
    elif kind == "append_node":
        nodes.append(rng.choice(nodes) if nodes else root)
    elif kind == "swap_nodes":
        if len(nodes) < 2:
            return None
        i = rng.randrange(len(nodes) - 1)
        nodes[i], nodes[i + 1] = nodes[i + 1], nodes[i]
    elif kind == "flip_node":
        if not nodes:
            return None
        i = rng.randrange(len(nodes))
        nodes[i] = TS._flip(nodes[i], rng)
    elif kind == "shift":
        up, down = start < end and end + 1 <= n, start > 0
        if not (up or down):
            return None
        d = 1 if up and (not down or rng.random() < 0.5) else -1
        start, end = start + d, end + d
    elif kind == "widen":
        if start == end or lh or (start == 0 and end == n):
            return None
        if start > 0 and (end == n or rng.random() < 0.5):
            start -= 1
            leaves.insert(0, t._leaves[start])
        else:
            leaves.append(t._leaves[end])
            end += 1
        if rng.random() < 0.5:
            nodes = t.prove_range(start, end).nodes
    elif kind == "narrow":
        if lh or end - start < 2:
            return None
        if rng.random() < 0.5:
            start += 1
            leaves.pop(0)
        else:
            end -= 1
            leaves.pop()
        nodes = t.prove_range(start, end).nodes  # a valid inclusion proof of fewer leaves
    elif kind == "swap_lr":
        if nl < 1 or len(nodes) <= nl:
            return None
        i, j = rng.randrange(nl), rng.randrange(nl, len(nodes))
        nodes[i], nodes[j] = nodes[j], nodes[i]
    elif kind == "absence_prev_leaf":
        if not lh or start == 0:
            return None
        lh = leaf_nodes[start - 1]
        if rng.random() < 0.5:  # with the proof that goes with that leaf: the root then matches
            start, end = start - 1, end - 1
            nodes = t.prove_range(start, end).nodes
    elif kind == "leaf_hash_on_inclusion":
        if lh or start == end:
            return None
        lh = leaf_nodes[start]
        if rng.random() < 0.5:
            end, leaves = start + 1, leaves[:1]
            nodes = t.prove_range(start, end).nodes
    elif kind == "leaves_on_empty":
        if start != end:
            return None
        leaves = [t._leaves[0]]
    elif kind == "leaves_on_absence":
        if not lh:
            return None
        leaves = [t._leaves[start]]  # ignored
    elif kind == "min_gt_max":
        if not nodes:
            return None
        i = rng.randrange(len(nodes))
        mn, mx = nodes[i][:NS], nodes[i][NS:2 * NS]
        if mn < mx:
            mn, mx = mx, mn
        elif ns_add(mx, 1) is not None:
            mn = ns_add(mx, 1)
        else:
            mx = ns_add(mn, -1)
        nodes[i] = mn + mx + nodes[i][2 * NS:]
    return start, end, nodes, lh, leaves, root


def cases(seed, count):
    """`count` cases (mutation, proof kind, nid, start, end, nodes, leaf_hash, leaves, root) over trees of 1..32
    leaves and the namespaces of nid_set."""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        n = rng.randint(1, 32)
        t = TS.make_tree(rng, n) if rng.random() < 0.4 else make_tree6(rng, n)
        root = TS.tree_root(t._leaf_nodes())
        nids = nid_set(t)
        for _ in range(8):
            nid = rng.choice(nids)
            p = t.prove_namespace(nid)
            leaves = t._leaves[p.start:p.end] if not p.leaf_hash else []
            kind = "valid" if rng.random() < 0.3 else rng.choice(MUTATIONS[1:])
            c = mutate(rng, kind, t, p, leaves, root)
            if c is not None:
                out.append((kind, proof_kind(p), nid) + c)
    return out[:count]


def mirror_verdict(case):
    _, _, nid, start, end, nodes, lh, leaves, root = case
    return NMTProof(start, end, nodes, lh).verify_namespace(nid, leaves, root)


def check_caps(all_cases, verdicts):
    """The fuzz cannot pass vacuously: both verdicts well represented, every mutation and every proof kind seen."""
    assert sum(verdicts) >= 100 and len(verdicts) - sum(verdicts) >= 100, (sum(verdicts), len(verdicts))
    assert {c[0] for c in all_cases} == set(MUTATIONS)
    assert {c[1] for c in all_cases} == {EMPTY, INCLUSION, ABSENCE}
    # and every proof kind on both sides
    for k in (EMPTY, INCLUSION, ABSENCE):
        got = {v for c, v in zip(all_cases, verdicts) if c[1] == k}
        assert got == {True, False}, k


FUZZ_SEED, FUZZ_COUNT = 0x4E4D54, 2500


def rule_root_ok(start, end, nodes, span, root):
    """V6 by the index rule (TS.walk: what the kernels evaluate), from the leaf nodes `span` of [start, end)."""
    w = TS.walk(start, end, len(nodes))
    if w is None:
        return False
    steps, rp = w
    span, state = list(span), {"bad": False}
    for _, lo, hi, left, right in steps:
        if left >= 0:
            span.insert(0, bytes(nodes[left]))
        if right >= 0:
            span.append(bytes(nodes[right]))
        nxt = [TS._node(span[i], span[i + 1], state) for i in range(0, len(span) - 1, 2)]
        if len(span) & 1:
            nxt.append(span[-1])
        span = nxt
    h = span[0]
    for x in nodes[rp:]:
        h = TS._node(h, bytes(x), state)
    return not state["bad"] and h == bytes(root)


def _hex(items):
    return b"".join(bytes(x) for x in items).hex() or "-"


@pytest.fixture(scope="module")
def rule_dump(tmp_path_factory):
    """tests/san/namespace_rule_dump.cpp + csrc/plan.cpp as a stand-alone executable under ASan and UBSan."""
    exe = str(tmp_path_factory.mktemp("nsr") / "namespace_rule_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "san", "namespace_rule_dump.cpp"), os.path.join(CSRC, "plan.cpp")])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", text=True, capture_output=True)
        assert out.returncode == 0, out.stderr[-2000:]
        got = out.stdout.splitlines()
        assert len(got) == len(lines)
        return got
    return run


def test_cpp_bounds_rule_matches_prove_namespace(rule_dump):
    """plan::namespace_bounds (P1-P3) over every tree and namespace of the mirror test."""
    lines, want = [], []
    for t in trees(0x4E53):
        root = TS.tree_root(t._leaf_nodes())
        lns = leaf_namespaces(t)
        for nid in nid_set(t):
            p = t.prove_namespace(nid)
            lines.append(f"P {nid.hex()} {root.hex()} {len(lns)} {_hex(lns)}")
            want.append(f"{(EMPTY, INCLUSION, ABSENCE).index(proof_kind(p))} {p.start} {p.end}")
    assert rule_dump(lines) == want
    assert {w[0] for w in want} == {"0", "1", "2"}


def test_cpp_verify_rule_matches_verify_namespace(rule_dump):
    """plan::namespace_precheck (V1-V5) followed by V6 by the index rule gives verify_namespace's verdict on valid and
    mutated proofs."""
    cs = cases(FUZZ_SEED, FUZZ_COUNT)
    want = [mirror_verdict(c) for c in cs]
    check_caps(cs, want)
    lines = [f"V {nid.hex()} {start} {end} {len(nodes)} {_hex(nodes)} {lh.hex() or '-'} {len(leaves)} {root.hex()}"
             for _, _, nid, start, end, nodes, lh, leaves, root in cs]
    pre = [int(x) for x in rule_dump(lines)]
    assert set(pre) == {0, 1, 2, 3}
    for c, p, w in zip(cs, pre, want):
        mut, pk, nid, start, end, nodes, lh, leaves, root = c
        if p == 2:
            got = TS.rule_verify(start, end, nodes, nid, leaves, root)
        elif p == 3:
            got = rule_root_ok(start, end, nodes, [lh], root)
        else:
            got = p == 1
        assert got == w, (mut, pk, start, end, len(nodes), p)
    # V1-V5 alone reject something the root would have accepted: the narrowed run
    assert any(p == 0 and c[0] == "narrow" for c, p in zip(cs, pre))


# ---- ABI shape ----
def test_namespace_structs_match_header(tmp_path):
    assert ctypes.sizeof(N.NamespaceQuery) == 40 == N.NAMESPACE_QUERY_DTYPE.itemsize
    assert ctypes.sizeof(N.NamespaceResult) == 24 == N.NAMESPACE_RESULT_DTYPE.itemsize
    assert ctypes.sizeof(N.NmtNsProofDesc) == 32 == N.NMT_NS_PROOF_DESC_DTYPE.itemsize
    for ct, dt in ((N.NamespaceQuery, N.NAMESPACE_QUERY_DTYPE), (N.NamespaceResult, N.NAMESPACE_RESULT_DTYPE),
                   (N.NmtNsProofDesc, N.NMT_NS_PROOF_DESC_DTYPE)):
        for name, _ in ct._fields_:
            assert getattr(ct, name).offset == dt.fields[name][1], name
    src = tmp_path / "sizes.c"
    src.write_text('#include "cda.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu %u %d %d %d\\n", '
                   'sizeof(cda_namespace_query), sizeof(cda_namespace_result), sizeof(cda_nmt_ns_proof_desc), '
                   'CDA_NO_LEAF_HASH, CDA_NSP_EMPTY, CDA_NSP_INCLUSION, CDA_NSP_ABSENCE); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    assert subprocess.check_output([exe], text=True).split() == ["40", "24", "32", str(N.NO_LEAF_HASH), "0", "1", "2"]
    assert (N.NSP_EMPTY, N.NSP_INCLUSION, N.NSP_ABSENCE) == (0, 1, 2)


def test_namespace_entry_points_reject_bad_arguments_without_gpu():
    """Argument checks run before any device work; the exception barrier covers the new entry points."""
    def calls(L):
        total = ctypes.c_uint64(7)
        return [L.cda_square_prove_namespace(None, 1, None, 2, None, None, None, None, 0, None),
                L.cda_square_prove_namespace(None, 1, None, 2, None, None, None, None, 0, ctypes.byref(total)),
                L.cda_nmt_verify_namespace(None, 1, None, None, None, 1, None, 0, None, 0, None, 1, None),
                L.cda_nmt_verify_namespace_device(None, 1, None, None, None, 1, None, 0, None, 0, None, 1, None, None)]
    assert calls(cda.lib()) == [N.E_ARG] * 4
    H = N.lib(N.HOOKS_LIB_PATH)
    os.environ["CDA_FAULT_INJECT"] = "entry"
    try:
        assert calls(H) == [N.E_NOMEM] * 4
    finally:
        del os.environ["CDA_FAULT_INJECT"]
    assert calls(H) == [N.E_ARG] * 4


@pytest.mark.parametrize("kernel", NEW_KERNELS)
def test_namespace_kernels_register_budget(kernel, tmp_path):
    """At most 128 VGPRs (4 waves per SIMD), no spilled VGPR, no private segment, read from the built library's
    metadata; ns_verify_absence_kernel is the one that hashes."""
    import test_hash_kernel_registers as R
    if not (os.path.exists(R.V.OBJDUMP) and os.path.exists(R.READOBJ) and os.path.exists(R.LIB)):
        pytest.skip("needs llvm-objdump, llvm-readobj and the built libcda.so")
    found = {n: m for n, m in R.kernel_metadata(R.LIB, str(tmp_path)).items() if kernel in n}
    assert len(found) == 1, sorted(found)
    (name, m), = found.items()
    print(name, m)
    assert m["vgpr_count"] <= 128 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m


def test_rows_of_namespace_is_the_root_range_rule():
    from cda import namespace as NSP
    a, b, c = bytes(NS - 1) + b"\x02", bytes(NS - 1) + b"\x05", bytes(NS - 1) + b"\x09"
    roots = [a + b + bytes(32), b + c + bytes(32), PARITY_SHARES_NAMESPACE * 2 + bytes(32)]
    assert NSP.rows_of_namespace(roots, b) == [0, 1]
    assert NSP.rows_of_namespace(roots, bytes(NS - 1) + b"\x03") == [0]
    assert NSP.rows_of_namespace(roots, bytes(NS)) == []
    assert NSP.rows_of_namespace(roots, PARITY_SHARES_NAMESPACE) == [2]
