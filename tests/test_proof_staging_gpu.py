"""GPU tests of how the proof calls stage their arguments: cda_nmt_verify, cda_share_proofs_validate,
cda_nmt_verify_namespace and cda_befp_validate, each in its host-buffer and its _device form, and the three provers
cda_square_prove, cda_square_share_proofs and cda_square_prove_namespace.  The host forms carve the context's staging
buffer with one arena and then run what the device forms run; these tests go where that can break: buffers that grow
inside a call, a workspace that held another call's data, sections a call leaves empty.

Everything is a k = 4 square (trees of 8 leaves).  Expected verdicts are the Python mirrors' -- NMTProof.
verify_inclusion, ShareProof.validate, NMTProof.verify_namespace, befp.validate_host -- over proofs from the host
wrapper trees (hashlib); expected proofs are the host trees'.  Every batch tiles a small pool that holds accepted and
rejected proofs (one flipped byte in a node, a share or a root), so no uniform verdict array passes; the one-proof
step of the growth test is two calls, one accepted and one rejected proof.  The verdict buffers start from a sentinel.

Where a section is left out (nroots = 0, nnodes_total = 0, nleaf_hashes = 0, with null pointers) the call returns
CDA_OK and the verdicts are the mirror's for a proof whose section is gone: an index outside a total is a rejected
proof, so a proof whose descriptor still points into the section gets the verdict of that check and
every other proof keeps its own (with nnodes_total = 0 that is the proof without nodes at node offset 0 alone).
tests/test_befp_gpu.py::test_mixed_batch already runs the device form of cda_befp_validate with a null node pointer
when no entry has nodes; nothing else of this is pinned elsewhere.
"""
import copy
import functools
import hashlib

import numpy as np
import pytest

import oracle_lib as O
import test_namespace as TN
from cda import _native as N
from cda import befp, sampling
from cda import proof as P
from cda.appconsts import NAMESPACE_SIZE, PARITY_SHARES_NAMESPACE
from cda.befp import BadEncodingProof
from cda.proof import NMTProof
from test_befp import CODECS, HostSquare, corrupted
from test_namespace_gpu import KINDS, synthetic_ods
from test_share_proofs_gpu import host_error

pytestmark = pytest.mark.gpu
K, W = 4, 8
SENTINEL = 77
SIZES = (300, 1, 700)  # more than one 256-thread block in a fresh context, one proof, then every buffer grows again


def flip(b, i):
    out = bytearray(b)
    out[i % len(out)] ^= 0x10
    return bytes(out)


def u8(rows, n):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(-1, n) if rows else np.zeros((0, n), np.uint8)


@functools.lru_cache(maxsize=None)
def world():
    """The k = 4 block (five namespaces, with gaps between them), its square on the host, and the same square with
    one bad Q3 cell."""
    ods, nss = synthetic_ods(K, 0x51)
    eds = O.extend(ods)
    return ods, nss, eds, HostSquare(eds, K), HostSquare(corrupted(eds, K, W - 1, W - 1, 41), K)


def merkle_proofs(items):
    """RFC-6962 tree over `items` (a power of two of them) -> (root, [cda.proof.Proof of item i])."""
    sha = lambda *p: hashlib.sha256(b"".join(p)).digest()  # noqa: E731
    levels = [[sha(b"\x00", bytes(x)) for x in items]]
    while len(levels[-1]) > 1:
        lv = levels[-1]
        levels.append([sha(b"\x01", lv[i], lv[i + 1]) for i in range(0, len(lv), 2)])
    proofs = [P.Proof(len(items), i, levels[0][i], [levels[h][(i >> h) ^ 1] for h in range(len(levels) - 1)])
              for i in range(len(items))]
    return levels[-1][0], proofs


@functools.lru_cache(maxsize=None)
def host_share_proof(s, e):
    """pkg/proof NewShareInclusionProof of ODS shares [s, e) from the host trees."""
    ods, _, _, sq, _ = world()
    root, row_proofs = merkle_proofs(sq.row_roots + sq.col_roots)
    first, last = s // K, (e - 1) // K
    nmt = []
    for r in range(first, last + 1):
        lo, hi = (s - r * K if r == first else 0), (e - r * K if r == last else K)
        nmt.append(NMTProof(lo, hi, list(sq.trees[0, r].prove_range(lo, hi).nodes)))
    ns = ods[s, :NAMESPACE_SIZE].tobytes()
    rows = range(first, last + 1)
    return P.ShareProof([ods[i].tobytes() for i in range(s, e)], nmt, ns[1:],
                        P.RowProof([sq.row_roots[r] for r in rows], [copy.deepcopy(row_proofs[r]) for r in rows],
                                   first, last), ns[0], root)


# ---- the four verifiers: a pool of cases with the mirror's verdicts, batches that tile it, the two forms ----
class Verifier:
    """pool: the cases; want: the mirror's verdict of each, as the code the call writes.  arrays(cases) -> the call's
    flat arrays; host / device -> the raw verdict array of that form."""

    def batch(self, n, off=0):
        idx = [(off + i) % len(self.pool) for i in range(n)]
        return self.arrays([self.pool[i] for i in idx]), [self.want[i] for i in idx]

    def device(self, ctx, arrays):
        import torch
        dev = torch.device("cuda", 0)
        keep = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev) if len(a) else None
                for a in arrays]
        out = torch.full((len(arrays[0]),), SENTINEL, dtype=getattr(torch, self.out_dtype), device=dev)
        stream = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        self.call_device(ctx, arrays, [t.data_ptr() if t is not None else 0 for t in keep], out.data_ptr(),
                         stream.cuda_stream)
        stream.synchronize()
        return out.cpu().numpy()


class NmtVerify(Verifier):
    name, out_dtype = "nmt_verify", "uint8"
    ROOTS, NODES = 2, 3
    NO_NODES = 7  # the pool's accepted proof without nodes

    def __init__(self):
        _, _, _, sq, _ = world()
        self.pool = []

        def add(axis, index, s, e, node=None, share=None, root=None):
            t = sq.trees[axis, index]
            nodes, leaves = list(t.prove_range(s, e).nodes), list(t._leaves[s:e])
            r = (sq.col_roots if axis else sq.row_roots)[index]
            ns = sampling.sample_namespace(K, axis, index, s, leaves[0])
            if node is not None:
                nodes[node] = flip(nodes[node], 40)
            if share is not None:
                leaves[share] = flip(leaves[share], 300)
            self.pool.append((s, e, nodes, ns, leaves, flip(r, 70) if root else r))
        add(0, 0, 0, 1)
        add(0, 0, 0, 1, node=1)
        add(0, 5, 3, 4)                # a parity row
        add(1, 2, 6, 7, share=0)       # a column through Q2
        add(0, 2, 0, 3)                # three leaves of one namespace: the kernel of the longer proofs
        add(1, 2, 6, 7)
        add(0, 2, 0, 3, share=2)
        add(0, 5, 0, W)                # the whole axis: a proof without nodes
        add(0, 1, 2, 3, root=True)
        self.want = [int(NMTProof(s, e, nodes).verify_inclusion(ns, leaves, root))
                     for s, e, nodes, ns, leaves, root in self.pool]
        assert self.want == [1, 0, 1, 0, 1, 1, 0, 1, 0]

    def arrays(self, cases):
        descs, nodes, leaves = [], [], []
        for i, (s, e, nd, ns, lv, root) in enumerate(cases):
            descs.append((s, e, len(nodes), len(nd), len(leaves), i))
            nodes += nd
            leaves += lv
        return (np.array(descs, N.NMT_PROOF_DESC_DTYPE), u8([c[3] for c in cases], NAMESPACE_SIZE),
                u8([c[5] for c in cases], N.NODE_SIZE), u8(nodes, N.NODE_SIZE), u8(leaves, N.SHARE_SIZE))

    def host(self, ctx, a):
        return ctx.nmt_verify(*a)

    def call_device(self, ctx, a, p, out, stream):
        ctx.nmt_verify_device(len(a[0]), p[0], p[1], p[2], len(a[2]), p[3], len(a[3]), p[4], len(a[4]), out, stream)

    def without(self, section, arrays, want):
        """The mirror's verdicts once `section` is gone: no root, no proof; no nodes, only a proof whose nodes
        [node_off, node_off + nnodes) still lie inside the total, which is the proof without nodes at offset 0."""
        if section == self.ROOTS:
            return [0] * len(want)
        return [w if int(d["node_off"]) + int(d["nnodes"]) == 0 else 0 for w, d in zip(want, arrays[0])]


class NsVerify(Verifier):
    name, out_dtype = "nmt_verify_namespace", "uint8"
    ROOTS, NODES, LEAF_HASHES = 2, 3, 4
    NO_NODES = 4  # the pool's accepted proof without nodes

    def __init__(self):
        _, nss, _, sq, _ = world()
        self.pool, kinds = [], set()

        def add(row, nid, node=None, share=None, root=None, leaf_hash=None, withhold=False):
            t = sq.trees[0, row]
            p = t.prove_namespace(nid)
            kind = TN.proof_kind(p)
            kinds.add(kind)
            nodes, lh, s, e = list(p.nodes), bytes(p.leaf_hash or b""), p.start, p.end
            leaves = list(t._leaves[s:e]) if kind == TN.INCLUSION else []
            if withhold:  # a valid range proof of all but the last share: not a namespace proof
                e -= 1
                nodes, leaves = list(t.prove_range(s, e).nodes), leaves[:-1]
            if node is not None:
                nodes[node] = flip(nodes[node], 50)
            if share is not None:
                leaves[share] = flip(leaves[share], 200)
            if leaf_hash:
                lh = flip(lh, 60)
            r = sq.row_roots[row]
            self.pool.append((nid, s, e, nodes, lh, leaves, flip(r, 75) if root else r))
        between, below = TN.ns_add(nss[0], 1), TN.ns_add(nss[0], -1)
        add(0, nss[3])                      # inclusion: the run that ends the first row
        add(0, nss[3], share=0)
        add(0, between)                     # absence
        add(1, nss[4], withhold=True)
        add(0, below)                       # empty: the root's range excludes it
        add(1, nss[4])
        add(0, between, leaf_hash=True)
        add(2, nss[4], node=0)
        add(5, PARITY_SHARES_NAMESPACE)     # a parity row: the whole axis, a proof without nodes
        add(0, nss[0], root=True)
        add(0, between, node=0)
        assert kinds == {TN.EMPTY, TN.INCLUSION, TN.ABSENCE} and set(KINDS) == kinds
        self.want = [int(NMTProof(s, e, nodes, lh).verify_namespace(nid, leaves, root))
                     for nid, s, e, nodes, lh, leaves, root in self.pool]
        assert self.want[:8] == [1, 0, 1, 0, 1, 1, 0, 0] and self.want[9:] == [0, 0]

    def arrays(self, cases):
        descs, nodes, lhs, leaves = [], [], [], []
        for i, (nid, s, e, nd, lh, lv, root) in enumerate(cases):
            at = N.NO_LEAF_HASH
            if lh:
                at = len(lhs)
                lhs.append(lh)
            descs.append((s, e, len(nodes), len(nd), len(leaves), len(lv), i, at))
            nodes += nd
            leaves += lv
        return (np.array(descs, N.NMT_NS_PROOF_DESC_DTYPE), u8([c[0] for c in cases], NAMESPACE_SIZE),
                u8([c[6] for c in cases], N.NODE_SIZE), u8(nodes, N.NODE_SIZE), u8(lhs, N.NODE_SIZE),
                u8(leaves, N.SHARE_SIZE))

    def host(self, ctx, a):
        return ctx.nmt_verify_namespace(*a)

    def call_device(self, ctx, a, p, out, stream):
        ctx.nmt_verify_namespace_device(len(a[0]), p[0], p[1], p[2], len(a[2]), p[3], len(a[3]), p[4], len(a[4]), p[5],
                                        len(a[5]), out, stream)

    def without(self, section, arrays, want):
        if section == self.ROOTS:
            return [0] * len(want)
        if section == self.NODES:
            return [w if int(d["node_off"]) + int(d["nnodes"]) == 0 else 0 for w, d in zip(want, arrays[0])]
        return [w if d["leaf_hash"] == N.NO_LEAF_HASH else 0 for w, d in zip(want, arrays[0])]


class ShareValidate(Verifier):
    name, out_dtype = "share_proofs_validate", "int32"
    NODES, ROOTS = 4, 7
    # the checks of ShareProof.validate these cases stop at, as include/cda.h numbers them
    CODES = {None: N.SP_VALID, "row proof failed to verify": N.SP_ROW_PROOF,
             "share proof failed to verify": N.SP_SHARE_PROOF}

    def __init__(self):
        good = [host_share_proof(s, e) for s, e in ((7, 8), (6, 16), (3, 6), (0, 1))]
        root = good[0].data_root
        self.roots = [root, flip(root, 9)]

        def tamper(i, fn):
            p = copy.deepcopy(good[i])
            fn(p)
            return p
        self.pool = [
            (good[0], 0),
            (tamper(1, lambda p: p.data.__setitem__(4, flip(p.data[4], 300))), 0),
            (good[1], 0),
            (tamper(0, lambda p: p.share_proofs[0].nodes.__setitem__(0, flip(p.share_proofs[0].nodes[0], 60))), 0),
            (good[2], 0),
            (tamper(2, lambda p: p.row_proof.row_roots.__setitem__(1, flip(p.row_proof.row_roots[1], 80))), 0),
            (good[3], 1),  # against a data root with a flipped byte
            (good[3], 0),
            (tamper(1, lambda p: p.row_proof.proofs[2].aunts.__setitem__(1, flip(p.row_proof.proofs[2].aunts[1], 3))), 0),
        ]
        self.want = [self.CODES[host_error(p, self.roots[r])] for p, r in self.pool]
        V, R, S = N.SP_VALID, N.SP_ROW_PROOF, N.SP_SHARE_PROOF
        assert self.want == [V, S, V, S, V, R, R, V, R]

    def arrays(self, cases):
        a = P.pack_share_proofs([p for p, _ in cases], [r for _, r in cases])
        return (a["descs"], a["rows"], a["row_roots"], a["leaf_hashes"], a["nodes"], a["aunts"], a["leaves"],
                np.frombuffer(b"".join(self.roots), np.uint8).reshape(-1, 32))

    def host(self, ctx, a):
        return ctx.share_proofs_validate(*a)

    def call_device(self, ctx, a, p, out, stream):
        ctx.share_proofs_validate_device(len(a[0]), p[0], p[1], p[2], p[3], len(a[1]), p[4], len(a[4]), p[5],
                                         len(a[5]), p[6], len(a[6]), p[7], len(a[7]), out, stream)

    def without(self, section, arrays, want):
        """No data roots: every descriptor points outside them.  No nodes: the share-proof leg fails in every proof
        the checks before it pass (at k = 4 every row's range proof has a node: the parity half)."""
        if section == self.ROOTS:
            return [N.SP_MALFORMED] * len(want)
        assert arrays[1]["nnodes"].all()
        return [N.SP_SHARE_PROOF if w == N.SP_VALID else w for w in want]


class BefpValidate(Verifier):
    name, out_dtype = "befp_validate", "int32"
    NODES, ROOTS = 3, 4

    def __init__(self):
        _, _, _, good, bad = world()
        # block 2: the honest square's roots with one byte of column root 3 flipped
        cols = list(good.col_roots)
        cols[3] = flip(cols[3], 66)
        self.roots = [good.roots, bad.roots, (good.row_roots, cols)]

        def on(block, p):
            p.block = block
            return p
        sh = good.create(0, 0).shares
        bad_share = (sh[-1][0], flip(sh[-1][1], 100), sh[-1][2])
        bad_node = (sh[2][0], sh[2][1], NMTProof(0, 1, [flip(sh[2][2].nodes[0], 33)] + list(sh[2][2].nodes[1:])))
        self.pool = [
            on(0, good.create(0, 0)),                                      # NO_FRAUD
            on(1, bad.create(0, W - 1)),                                   # FRAUD: every share, a bad parity cell
            on(0, BadEncodingProof(0, 0, list(sh[:K - 1]))),               # TOO_FEW
            on(0, good.create(1, 1, [0, 2, 5, 7])),                        # NO_FRAUD through the decoder
            on(0, BadEncodingProof(0, 0, list(sh[:-1]) + [bad_share])),    # BAD_SHARE: a share byte
            on(1, bad.create(1, W - 1, [0, 1, 2, 3])),                     # FRAUD with the bad cell left out
            on(0, BadEncodingProof(0, 0, list(sh[:2]) + [bad_node] + list(sh[3:]))),  # BAD_SHARE: a node byte
            on(2, good.create(0, 0)),                                      # BAD_SHARE: a root byte
            on(2, good.create(0, 0, [0, 1, 2, 4, 5])),                     # NO_FRAUD: the flipped root is not used
            on(0, BadEncodingProof(2, 0, list(sh))),                       # MALFORMED
        ]
        self.want = [befp.validate_host(p, *self.roots[p.block], codec=CODECS["leopard"]) for p in self.pool]
        assert self.want == [befp.NO_FRAUD, befp.FRAUD, befp.TOO_FEW, befp.NO_FRAUD, befp.BAD_SHARE, befp.FRAUD,
                             befp.BAD_SHARE, befp.BAD_SHARE, befp.NO_FRAUD, befp.MALFORMED]

    def arrays(self, cases):
        return befp.pack(cases, K) + (befp.pack_roots(self.roots),)

    def host(self, ctx, a):
        return ctx.befp_validate(K, *a)

    def call_device(self, ctx, a, p, out, stream):
        ctx.befp_validate_device(K, len(a[0]), p[0], p[1], len(a[1]), p[2], p[3], len(a[3]), p[4], len(a[4]), out,
                                 stream)

    def without(self, section, arrays, want):
        """B1: a proof's block of roots and its entries' nodes lie inside the totals, else MALFORMED; at
        k = 4 every entry has nodes."""
        assert arrays[1]["nnodes"].all()
        return [befp.MALFORMED] * len(want)


@functools.lru_cache(maxsize=None)
def verifier(name):
    return {v.name: v for v in (NmtVerify, ShareValidate, NsVerify, BefpValidate)}[name]()


NAMES = ["nmt_verify", "share_proofs_validate", "nmt_verify_namespace", "befp_validate"]
FORMS = ["host", "device"]


def run(v, form, ctx, arrays):
    return [int(x) for x in getattr(v, form)(ctx, arrays)]


def mixed(want):
    return len(set(want)) > 1


@pytest.fixture
def fresh():
    """A context of its own: every buffer unallocated."""
    import cda
    c = cda.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_buffers_grow_inside_the_call(fresh, name, form):
    """The first call of a context is a batch of 300 (every buffer is allocated in it, after the sizes are known and
    before the first copy), then one proof (an accepted one, then a rejected one), then 700 (every buffer grows)."""
    v = verifier(name)
    rejected = next(i for i, w in enumerate(v.want) if w != v.want[0])
    for n, off in ((SIZES[0], 0), (SIZES[1], 0), (SIZES[1], rejected), (SIZES[2], 3)):
        arrays, want = v.batch(n, off)
        assert mixed(want) or (n == 1 and want == [v.want[off]])
        assert run(v, form, fresh, arrays) == want, (n, off)


@pytest.mark.parametrize("name", NAMES)
def test_host_form_equals_device_form(ctx, name):
    """The same batch through both forms: the verdict arrays are equal byte for byte (and the mirror's)."""
    v = verifier(name)
    arrays, want = v.batch(SIZES[0], 1)
    host, device = v.host(ctx, arrays), v.device(ctx, arrays)
    assert mixed(want) and [int(x) for x in host] == want
    assert host.dtype == device.dtype and host.tobytes() == device.tobytes()


# ---- the provers against the host trees ----
RANGE_POOL = [(0, 0, 0, 1), (1, 2, 6, 7), (0, 5, 3, 4), (0, 2, 0, 3), (1, 7, 0, W), (0, 1, 1, 4), (1, 0, 3, 8),
              (0, 7, 7, 8), (1, 4, 2, 5), (0, 3, 0, W), (1, 3, 4, 5)]
SHARE_RANGE_POOL = [(7, 8), (6, 16), (3, 6), (0, 1), (15, 16), (8, 12), (6, 11), (10, 11)]


def tile(pool, n):
    return [pool[i % len(pool)] for i in range(n)]


def prove_ranges(sq, n, want_shares):
    """cda_square_prove of n queries == prove_range of the host trees and the EDS cells."""
    _, _, _, host, _ = world()
    queries = tile(RANGE_POOL, n)
    counts, nodes, shares = sq.prove(queries, want_shares=want_shares)
    assert (shares is None) == (not want_shares)
    cursor = 0
    for i, (axis, index, s, e) in enumerate(queries):
        want = host.trees[axis, index].prove_range(s, e).nodes
        assert counts[i] == len(want) and [nodes[i, j].tobytes() for j in range(len(want))] == want, queries[i]
        assert not nodes[i, len(want):].any()
        if want_shares:
            assert [x.tobytes() for x in shares[cursor:cursor + e - s]] == host.trees[axis, index]._leaves[s:e]
            cursor += e - s
    assert not want_shares or cursor == len(shares)


def prove_shares(sq, n, want_shares):
    """cda_square_share_proofs of n ranges == the ShareProof the host builds, field by field."""
    ranges = tile(SHARE_RANGE_POOL, n)
    want = {r: host_share_proof(*r) for r in SHARE_RANGE_POOL}
    raw = sq.share_proofs_raw(ranges, want_shares=want_shares)
    assert (raw["shares"] is None) == (not want_shares)
    rows, cursor = raw["rows"], 0
    assert raw["row_off"][0] == 0 and int(raw["row_off"][-1]) == len(rows)
    for i, (s, e) in enumerate(ranges):
        w = want[s, e]
        lo, hi = int(raw["row_off"][i]), int(raw["row_off"][i + 1])
        assert raw["data_root"] == w.data_root and hi - lo == len(w.share_proofs)
        assert (int(rows[lo]["row"]), int(rows[hi - 1]["row"])) == (w.row_proof.start_row, w.row_proof.end_row)
        for j, r in enumerate(range(lo, hi)):
            nmt, mp = w.share_proofs[j], w.row_proof.proofs[j]
            assert (rows[r]["nmt_start"], rows[r]["nmt_end"], rows[r]["nnodes"]) == (nmt.start, nmt.end, len(nmt.nodes))
            assert [raw["nodes"][r, t].tobytes() for t in range(len(nmt.nodes))] == nmt.nodes
            assert not raw["nodes"][r, len(nmt.nodes):].any()
            assert raw["row_roots"][r].tobytes() == w.row_proof.row_roots[j]
            assert (rows[r]["total"], rows[r]["index"], rows[r]["naunts"]) == (mp.total, mp.index, len(mp.aunts))
            assert raw["leaf_hashes"][r].tobytes() == mp.leaf_hash
            assert [raw["aunts"][r, t].tobytes() for t in range(len(mp.aunts))] == mp.aunts
        if want_shares:
            assert [x.tobytes() for x in raw["shares"][cursor:cursor + e - s]] == w.data
            cursor += e - s
    assert not want_shares or cursor == len(raw["shares"])


def namespace_queries():
    _, nss, _, _, _ = world()
    nids = [nss[0], nss[3], nss[4], TN.ns_add(nss[0], 1), TN.ns_add(nss[0], -1), PARITY_SHARES_NAMESPACE,
            TN.ns_add(nss[3], 1)]
    return [(axis, index, nid) for nid in nids for axis, index in ((0, 0), (0, 1), (1, 0), (0, 6), (1, 3))]


def prove_namespaces(sq, n, want_shares):
    """cda_square_prove_namespace of n queries == prove_namespace of the host trees and the EDS cells."""
    _, _, _, host, _ = world()
    queries = tile(namespace_queries(), n)
    results, nodes, leaf_hashes, shares = sq.prove_namespace(queries, want_shares=want_shares)
    assert (shares is None) == (not want_shares)
    cursor, kinds = 0, set()
    for i, (axis, index, nid) in enumerate(queries):
        t = host.trees[axis, index]
        p = t.prove_namespace(nid)
        kind, r = TN.proof_kind(p), results[i]
        kinds.add(kind)
        assert (r["kind"], r["start"], r["end"], r["nnodes"]) == (KINDS[kind], p.start, p.end, len(p.nodes)), queries[i]
        assert [nodes[i, j].tobytes() for j in range(len(p.nodes))] == p.nodes and not nodes[i, len(p.nodes):].any()
        assert leaf_hashes[i].tobytes() == (bytes(p.leaf_hash) if kind == TN.ABSENCE else bytes(N.NODE_SIZE))
        cells = p.end - p.start if kind == TN.INCLUSION else 0
        assert (r["share_off"], r["nshares"]) == (cursor, cells)
        if want_shares:
            assert [x.tobytes() for x in shares[cursor:cursor + cells]] == t._leaves[p.start:p.start + cells]
        cursor += cells
    assert cursor == sq.nshares_total and (not want_shares or cursor == len(shares))
    assert n == 1 or kinds == {TN.EMPTY, TN.INCLUSION, TN.ABSENCE}


PROVERS = {"square_prove": prove_ranges, "square_share_proofs": prove_shares,
           "square_prove_namespace": prove_namespaces}


@pytest.mark.parametrize("n", [1, 300])
@pytest.mark.parametrize("want_shares", [True, False])
@pytest.mark.parametrize("prover", list(PROVERS))
def test_provers_on_a_fresh_context(fresh, prover, want_shares, n):
    ods = world()[0]
    with fresh.open_square(ods) as sq:
        PROVERS[prover](sq, n, want_shares)


# ---- the workspace between calls ----
@pytest.mark.parametrize("order", [[0, 1, 2, 3], [3, 1, 0, 2]])
def test_verdicts_do_not_depend_on_what_the_workspace_held(order):
    """The four verifiers one after another on one context, a prove call of each kind between them, host and device
    forms in turn: every verdict array is the one a fresh context gives (and the mirror's)."""
    import cda
    ods = world()[0]
    batches = {name: verifier(name).batch(SIZES[0] + 11 * i, i) for i, name in enumerate(NAMES)}
    alone = {}
    for name in NAMES:
        c = cda.Context(0)
        v = verifier(name)
        arrays, want = batches[name]
        alone[name] = run(v, "host", c, arrays)
        assert alone[name] == want and mixed(want)
        c.close()
    shared = cda.Context(0)
    try:
        with shared.open_square(ods) as sq:
            provers = list(PROVERS.values())
            for turn, i in enumerate(order + order[::-1]):
                name = NAMES[i]
                v = verifier(name)
                arrays, _ = v.batch(SIZES[0] + 11 * i, i)
                assert run(v, FORMS[turn % 2], shared, arrays) == alone[name], (turn, name)
                provers[turn % 3](sq, 40 + turn, turn % 2 == 0)
    finally:
        shared.close()


# ---- sections left out ----
SECTIONS = [("nmt_verify", "ROOTS"), ("nmt_verify", "NODES"), ("share_proofs_validate", "ROOTS"),
            ("share_proofs_validate", "NODES"), ("nmt_verify_namespace", "ROOTS"), ("nmt_verify_namespace", "NODES"),
            ("nmt_verify_namespace", "LEAF_HASHES"), ("befp_validate", "ROOTS"), ("befp_validate", "NODES")]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,section", SECTIONS)
def test_a_section_left_out(ctx, name, section, form):
    """A count of zero with a null pointer: the call returns CDA_OK (the wrappers raise otherwise) and rejects exactly
    the proofs that need the section; with the section in place the same batch has accepted and rejected proofs."""
    v = verifier(name)
    arrays, want = v.batch(40, getattr(v, "NO_NODES", 2))  # where there is a proof without nodes, it comes first
    assert run(v, form, ctx, arrays) == want and mixed(want)
    at = getattr(v, section)
    cut = list(arrays)
    cut[at] = arrays[at][:0]
    gone = v.without(at, arrays, want)
    assert gone != want
    assert run(v, form, ctx, tuple(cut)) == gone
