"""GPU tests of namespace data with completeness proofs: cda_square_prove_namespace against the host wrapper tree's
prove_namespace (hashlib) byte for byte, and cda_nmt_verify_namespace / _device against NMTProof.verify_namespace.
The inclusion leg is pinned through host verify_inclusion and mainnet block 408, whose row roots hash to the header's
data_hash; the completeness and absence rules are DESIGN §18's (tests/test_namespace.py holds the mirror to them).
"""
import os
import random

import numpy as np
import pytest

import test_namespace as TN
import test_sampling as TS
from cda import _native as N
from cda import namespace as NSP
from cda.appconsts import NAMESPACE_SIZE, PARITY_SHARES_NAMESPACE
from cda.proof import NMTProof
from cda.wrapper import ErasuredNamespacedMerkleTree
from test_inclusion import GOLDEN, mainnet_ods
from test_sampling_gpu import axis_cells, host_tree

pytestmark = pytest.mark.gpu
NS = NAMESPACE_SIZE
KINDS = {TN.EMPTY: N.NSP_EMPTY, TN.INCLUSION: N.NSP_INCLUSION, TN.ABSENCE: N.NSP_ABSENCE}

# run lengths of the namespaces of the synthetic squares, in share order.  k = 4 and 16: the first row holds four
# namespaces, the fourth run ends mid-row, the fifth spans two (k = 4) or thirteen (k = 16) whole rows.
RUNS = {1: [1], 2: [1, 2, 1], 4: [1, 1, 1, 3, 10], 16: [5, 3, 4, 14, 220, 10]}


def synthetic_ods(k, seed):
    """(ods, namespaces): run i of RUNS[k] under namespace 0x00 ‖ 0 x 18 ‖ id, ids 2 apart (a namespace lies between
    every adjacent pair), random payloads."""
    rng = np.random.default_rng(seed)
    ods = rng.integers(0, 256, (k * k, N.SHARE_SIZE), dtype=np.uint8)
    nss, at = [], 0
    for i, n in enumerate(RUNS[k]):
        ns = bytes(NS - 2) + bytes([seed & 0x7F, 2 * i + 2])
        ods[at:at + n, :NS] = np.frombuffer(ns, np.uint8)
        nss.append(ns)
        at += n
    assert at == k * k
    return ods, nss


def query_namespaces(nss):
    out = set(nss) | {TN.ns_add(nss[0], -1), TN.ns_add(nss[-1], 1), PARITY_SHARES_NAMESPACE}
    out |= {TN.ns_add(a, 1) for a in nss[:-1]}
    return sorted(out)


@pytest.mark.parametrize("k", [1, 2, 4, 16])
def test_prove_namespace_every_tree(ctx, k):
    """Every row and every column tree of the 2k x 2k square (the bottom and right halves included) asked for every
    present namespace, one below the first, one between each pair, one above the last and the parity namespace:
    results, nodes (zero padding included), leaf hashes and shares equal the host tree's prove_namespace and the EDS
    cells; share_off is the running sum of nshares and ends at nshares_total; without the shares the proofs are the
    same.  k = 1: proofs of 0 or 1 node; k = 2: nodes on both sides; k = 16: the axis is exactly one 32-lane pass."""
    ods, nss = synthetic_ods(k, 0x30 + k)
    eds = ctx.extend_commit(ods)[0]
    w = 2 * k
    queries = [(axis, index, nid) for axis in (0, 1) for index in range(w) for nid in query_namespaces(nss)]
    with ctx.open_square(ods) as sq:
        results, nodes, leaf_hashes, shares = sq.prove_namespace(queries)
        total = sq.nshares_total
        r2, n2, l2, s2 = sq.prove_namespace(queries, want_shares=False)
        assert s2 is None and sq.nshares_total == total
        assert np.array_equal(r2, results) and np.array_equal(n2, nodes) and np.array_equal(l2, leaf_hashes)
    assert nodes.shape == (len(queries), max(1, 2 * (w.bit_length() - 1)), N.NODE_SIZE)
    trees, cursor, seen, counts = {}, 0, set(), set()
    for i, (axis, index, nid) in enumerate(queries):
        if (axis, index) not in trees:
            trees[axis, index] = host_tree(eds, k, axis, index)
        p = trees[axis, index].prove_namespace(nid)
        kind = TN.proof_kind(p)
        r = results[i]
        ctxt = (k, axis, index, nid.hex(), kind)
        assert (r["kind"], r["start"], r["end"], r["nnodes"]) == (KINDS[kind], p.start, p.end, len(p.nodes)), ctxt
        assert [nodes[i, j].tobytes() for j in range(len(p.nodes))] == p.nodes, ctxt
        assert not nodes[i, len(p.nodes):].any(), ctxt
        assert leaf_hashes[i].tobytes() == (bytes(p.leaf_hash) if kind == TN.ABSENCE else bytes(N.NODE_SIZE)), ctxt
        n = p.end - p.start if kind == TN.INCLUSION else 0
        assert (r["share_off"], r["nshares"]) == (cursor, n), ctxt
        assert np.array_equal(shares[cursor:cursor + n], axis_cells(eds, w, axis, index)[p.start:p.start + n]), ctxt
        cursor += n
        seen.add(kind)
        counts.add(len(p.nodes))
    assert cursor == total == len(shares)
    assert seen == ({TN.EMPTY, TN.INCLUSION} if k == 1 else {TN.EMPTY, TN.INCLUSION, TN.ABSENCE})
    if k == 1:
        assert counts == {0, 1}


def mainnet_namespaces(ods):
    return sorted(set(bytes(x[:NS]) for x in ods))


def test_block_408_namespace_data(ctx):
    """Mainnet block 408 (k = 32: two passes per axis): for each of its 5 namespaces get_shares_by_namespace returns
    exactly the ODS shares of that namespace in order; every returned row verifies on the GPU (completeness included)
    and its inclusion proof verifies on the host against row roots whose DAH is the header's data_hash; a namespace
    absent between ...04 and ...ff gives one ABSENCE proof, on row 11; one below all gives no rows."""
    ods = mainnet_ods()
    k = int(round(len(ods) ** 0.5))
    nss = mainnet_namespaces(ods)
    assert k == 32 and len(nss) == 5
    ods_ns = [bytes(x[:NS]) for x in ods]
    rows_of = {ns: sorted({i // k for i, x in enumerate(ods_ns) if x == ns}) for ns in nss}
    assert rows_of[nss[0]] == list(range(0, 12)) and rows_of[nss[3]] == list(range(11, 23))
    assert rows_of[nss[4]] == list(range(22, 32)) and sum(11 in r for r in rows_of.values()) == 4
    with ctx.open_square(ods) as sq:
        assert sq.dah == np.load(os.path.join(GOLDEN, "mainnet_h408.npz"))["data_hash"].tobytes()
        row_roots = sq.row_roots.copy()
        for ns in nss:
            rows = NSP.get_shares_by_namespace(sq, ns)
            assert [r for r, _, _ in rows] == rows_of[ns]
            got = [s for _, shares, _ in rows for s in shares]
            assert got == [bytes(x) for x, y in zip(ods, ods_ns) if y == ns]
            assert NSP.verify_namespace_data(ctx, ns, rows, row_roots) == [True] * len(rows)
            for r, shares, p in rows:
                assert not p.leaf_hash and p.verify_inclusion(ns, shares, row_roots[r].tobytes())
                assert p.verify_namespace(ns, shares, row_roots[r].tobytes())
            # a server that withholds the last share of the first row: a valid range proof, not a namespace proof
            r, shares, p = rows[0]
            if len(shares) >= 2:
                cut = sq.prove([(0, r, p.start, p.end - 1)], want_shares=False)
                short = NMTProof(p.start, p.end - 1, [cut[1][0, j].tobytes() for j in range(cut[0][0])])
                assert short.verify_inclusion(ns, shares[:-1], row_roots[r].tobytes())
                assert NSP.verify_namespace_data(ctx, ns, [(r, shares[:-1], short)], row_roots) == [False]
        absent = TN.ns_add(nss[1], 1)
        assert nss[1] < absent < nss[2]
        rows = NSP.get_shares_by_namespace(sq, absent)
        assert len(rows) == 1
        r, shares, p = rows[0]
        assert r == 11 and shares == [] and p.leaf_hash and (p.start, p.end) == (365 % k, 365 % k + 1)
        assert p.verify_namespace(absent, [], row_roots[11].tobytes())
        assert NSP.verify_namespace_data(ctx, absent, rows, row_roots) == [True]
        assert NSP.get_shares_by_namespace(sq, TN.ns_add(nss[0], -1)) == []


class NsBatch:
    """A cda_nmt_verify_namespace batch built case by case, with the mirror's verdict of every case."""

    def __init__(self):
        self.descs, self.ns, self.roots, self.nodes, self.leaf_hashes, self.leaves, self.want = [], [], [], [], [], [], []

    def add(self, nid, start, end, nodes, leaf_hash, leaves, root):
        self.want.append(NMTProof(start, end, nodes, leaf_hash).verify_namespace(nid, leaves, root))
        lh = N.NO_LEAF_HASH
        if leaf_hash:
            lh = len(self.leaf_hashes)
            self.leaf_hashes.append(bytes(leaf_hash))
        self.descs.append((start, end, len(self.nodes), len(nodes), len(self.leaves), len(leaves), len(self.roots), lh))
        self.ns.append(bytes(nid))
        self.roots.append(bytes(root))
        self.nodes += [bytes(x) for x in nodes]
        self.leaves += [bytes(x) for x in leaves]

    def arrays(self, order=None):
        def u8(rows, n):
            return np.frombuffer(b"".join(rows), np.uint8).reshape(-1, n)
        descs, ns = np.array(self.descs, N.NMT_NS_PROOF_DESC_DTYPE), u8(self.ns, NS)
        if order is not None:
            descs, ns = descs[order], ns[order]
        return (descs, ns, u8(self.roots, N.NODE_SIZE), u8(self.nodes, N.NODE_SIZE), u8(self.leaf_hashes, N.NODE_SIZE),
                u8(self.leaves, N.SHARE_SIZE))


def test_verdicts_match_mirror(ctx):
    """The valid and mutated proofs of tests/test_namespace.py, every kind mixed in ONE batch with the descriptors in
    shuffled order: every verdict is verify_namespace's."""
    cs = TN.cases(TN.FUZZ_SEED, TN.FUZZ_COUNT)
    batch = NsBatch()
    for _, _, nid, start, end, nodes, lh, leaves, root in cs:
        batch.add(nid, start, end, nodes, lh, leaves, root)
    TN.check_caps(cs, batch.want)
    order = np.random.default_rng(408).permutation(len(cs))
    ok = ctx.nmt_verify_namespace(*batch.arrays(order))
    assert set(ok.tolist()) <= {0, 1}
    wrong = [int(i) for j, i in enumerate(order) if bool(ok[j]) != batch.want[i]]
    assert not wrong, [(cs[i][:2], cs[i][3:5], batch.want[i]) for i in wrong[:8]]


def test_verify_long_namespace_run(ctx):
    """A tree of 1,100 leaves with a 600-leaf run crossing leaf 512 (two chunks of the range kernel, reached through
    the prep kernel's descriptors): the namespace proof verifies; the run narrowed by one at either end is a valid
    inclusion proof and no namespace proof."""
    rng = np.random.default_rng(1100)
    a, b, c = (bytes(NS - 1) + bytes([x]) for x in (3, 5, 9))
    t = ErasuredNamespacedMerkleTree(1100, 0)
    data = rng.integers(0, 256, (1100, N.SHARE_SIZE), dtype=np.uint8)
    for lo, hi, ns in ((0, 300, a), (300, 900, b), (900, 1100, c)):
        data[lo:hi, :NS] = np.frombuffer(ns, np.uint8)
    t._leaves = [bytes(x) for x in data]
    root = TS.tree_root(t._leaf_nodes())
    batch = NsBatch()
    p = t.prove_namespace(b)
    assert (p.start, p.end) == (300, 900)
    batch.add(b, p.start, p.end, p.nodes, b"", t._leaves[300:900], root)
    for s, e in ((301, 900), (300, 899)):
        q = t.prove_range(s, e)
        assert q.verify_inclusion(b, t._leaves[s:e], root)
        batch.add(b, s, e, q.nodes, b"", t._leaves[s:e], root)
    absent = t.prove_namespace(bytes(NS - 1) + bytes([4]))
    assert absent.leaf_hash and absent.start == 300
    batch.add(bytes(NS - 1) + bytes([4]), absent.start, absent.end, absent.nodes, absent.leaf_hash, [], root)
    assert batch.want == [True, False, False, True]
    assert ctx.nmt_verify_namespace(*batch.arrays()).tolist() == [1, 0, 0, 1]


def test_device_forms(ctx):
    """Prove into device buffers, verify there with cda_nmt_verify_namespace_device on the buffers as they lie
    (node_off = q * max_nodes, leaf_hash = q, leaf_off = share_off); a shares_cap too small returns CDA_E_ARG with the
    right total and everything but the shares, and a retry with that total succeeds; descriptors outside the totals
    or with end > 65536 get 0 (CDA_E_ARG for the latter in the host form); a closed or detached handle is refused."""
    import torch
    k, w, mn = 4, 8, 8
    ods, nss = synthetic_ods(k, 0x44)
    eds = ctx.extend_commit(ods)[0]
    queries = [(axis, index, nid) for axis in (0, 1) for index in range(w) for nid in query_namespaces(nss)]
    nq = len(queries)
    dev = torch.device("cuda", 0)
    d_res = torch.zeros(nq * 24, dtype=torch.uint8, device=dev)
    d_nodes = torch.full((nq, mn, N.NODE_SIZE), 0xAB, dtype=torch.uint8, device=dev)
    d_lh = torch.full((nq, N.NODE_SIZE), 0xAB, dtype=torch.uint8, device=dev)
    d_shares = torch.zeros((nq * w, N.SHARE_SIZE), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sq = ctx.open_square(ods)
    try:
        want_res, want_nodes, want_lh, want_shares = sq.prove_namespace(queries)
        total = sq.nshares_total
        assert total > 1
        with pytest.raises(N.CdaError) as e:
            sq.prove_namespace_device(queries, mn, d_res.data_ptr(), d_nodes.data_ptr(), d_lh.data_ptr(),
                                      d_shares.data_ptr(), (total - 1) * N.SHARE_SIZE)
        assert e.value.code == N.E_ARG and sq.nshares_total == total
        torch.cuda.synchronize()
        assert not d_shares.any().item()  # not written
        res = d_res.cpu().numpy().view(N.NAMESPACE_RESULT_DTYPE)
        assert np.array_equal(res, want_res) and np.array_equal(d_lh.cpu().numpy(), want_lh)
        assert sq.prove_namespace_device(queries, mn, d_res.data_ptr(), d_nodes.data_ptr(), d_lh.data_ptr(),
                                         d_shares.data_ptr(), total * N.SHARE_SIZE) == total
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(N.NAMESPACE_RESULT_DTYPE)
        assert np.array_equal(res, want_res) and np.array_equal(d_shares[:total].cpu().numpy(), want_shares)
        nodes8 = d_nodes.cpu().numpy()
        assert np.array_equal(nodes8[:, :want_nodes.shape[1]], want_nodes) and not nodes8[:, want_nodes.shape[1]:].any()
        roots = np.concatenate([sq.row_roots, sq.col_roots])
        # max_nodes below 2 log2(2k), a bad axis, a bad index: refused before any launch
        for bad_q, bad_mn in (([queries[0]], 5), ([(2, 0, nss[0])], mn), ([(0, w, nss[0])], mn)):
            with pytest.raises(N.CdaError) as e:
                sq.prove_namespace_device(bad_q, bad_mn, d_res.data_ptr(), d_nodes.data_ptr(), d_lh.data_ptr())
            assert e.value.code == N.E_ARG
    finally:
        sq.close()
    with pytest.raises(N.CdaError) as e:  # a closed handle
        sq.prove_namespace(queries[:1])
    assert e.value.code == N.E_ARG
    descs = np.zeros(nq + 5, N.NMT_NS_PROOF_DESC_DTYPE)
    for f in ("start", "end", "nnodes"):
        descs[f][:nq] = res[f]
    descs["node_off"][:nq] = np.arange(nq, dtype=np.uint32) * mn
    descs["leaf_off"][:nq], descs["nleaves"][:nq] = res["share_off"], res["nshares"]
    descs["root"][:nq] = [axis * w + index for axis, index, _ in queries]
    descs["leaf_hash"][:nq] = np.where(res["kind"] == N.NSP_ABSENCE, np.arange(nq, dtype=np.uint32), N.NO_LEAF_HASH)
    good = int(np.flatnonzero((res["kind"] == N.NSP_INCLUSION) & (res["nnodes"] > 0))[0])
    gone = int(np.flatnonzero(res["kind"] == N.NSP_ABSENCE)[0])
    extra = [(good, "node_off", nq * mn), (good, "leaf_off", total), (good, "root", len(roots)), (gone, "leaf_hash", nq)]
    for j, (src, field, value) in enumerate(extra):
        descs[nq + j] = descs[src]
        descs[field][nq + j] = value
    descs[nq + 4] = (65536, 65537, 0, 0, 0, 1, 0, N.NO_LEAF_HASH)
    ns = np.stack([np.frombuffer(nid, np.uint8) for _, _, nid in queries] +
                  [np.frombuffer(queries[src][2], np.uint8) for src, _, _ in extra] + [np.zeros(NS, np.uint8)])
    d_descs = torch.from_numpy(descs.view(np.uint8).reshape(-1).copy()).to(dev)
    d_ns = torch.from_numpy(ns.reshape(-1).copy()).to(dev)
    d_roots = torch.from_numpy(roots.reshape(-1).copy()).to(dev)
    d_ok = torch.full((nq + 5,), 7, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    ctx.nmt_verify_namespace_device(nq + 5, d_descs.data_ptr(), d_ns.data_ptr(), d_roots.data_ptr(), len(roots),
                                    d_nodes.data_ptr(), nq * mn, d_lh.data_ptr(), nq, d_shares.data_ptr(), total,
                                    d_ok.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    ok = d_ok.cpu().numpy()
    assert ok[:nq].tolist() == [1] * nq and ok[nq:].tolist() == [0] * 5
    # the same batch through the host form: CDA_E_ARG for the descriptor with end > 65536, the verdicts without it
    host = (ns, roots, nodes8.reshape(-1, N.NODE_SIZE), want_lh, want_shares)
    with pytest.raises(N.CdaError) as e:
        ctx.nmt_verify_namespace(descs, *host)
    assert e.value.code == N.E_ARG
    assert ctx.nmt_verify_namespace(descs[:nq + 4], ns[:nq + 4], *host[1:]).tolist() == [1] * nq + [0] * 4
    # every proof against its tree's host mirror as well
    for i in random.Random(4).sample(range(nq), 24):
        axis, index, nid = queries[i]
        p = NMTProof(int(res["start"][i]), int(res["end"][i]), [nodes8[i, j].tobytes() for j in range(res["nnodes"][i])],
                     want_lh[i].tobytes() if res["kind"][i] == N.NSP_ABSENCE else b"")
        lo = int(res["share_off"][i])
        assert p.verify_namespace(nid, [bytes(x) for x in want_shares[lo:lo + int(res["nshares"][i])]],
                                  roots[axis * w + index].tobytes())
    assert np.array_equal(want_shares[:1], axis_cells(eds, w, 0, 0)[:1])
    # misaligned device pointers are refused before any launch
    L = ctx._L
    assert L.cda_nmt_verify_namespace_device(ctx._h, 1, 4096, 4096, 4096, 1, 4096, 0, 4096, 0, 4097, 1, 4096,
                                             None) == N.E_ARG
    assert L.cda_nmt_verify_namespace_device(ctx._h, 1, 4096, 4096, 4096, 1, 4096, 0, 4098, 1, 4096, 1, 4096,
                                             None) == N.E_ARG


def test_detached_square_refuses_prove_namespace():
    """cda_free of the context detaches its squares: prove_namespace answers CDA_E_ARG, close still works."""
    import cda
    c = cda.Context(0)
    ods, nss = synthetic_ods(2, 0x22)
    sq = c.open_square(ods)
    assert sq.prove_namespace([(0, 0, nss[0])])[0]["kind"][0] == N.NSP_INCLUSION
    c.close()
    with pytest.raises(N.CdaError) as e:
        sq.prove_namespace([(0, 0, nss[0])])
    assert e.value.code == N.E_ARG
    sq.close()


def test_nothing_else_moved(ctx):
    """cda_square_prove and cda_nmt_verify on the same square give identical bytes before and after a
    prove_namespace call (which uses the context's workspace between them)."""
    k = 8
    ods, nss = synthetic_ods(4, 0x55)
    big = np.concatenate([ods] * 4)
    big = big[np.lexsort(big[:, :NS].T[::-1])]  # 64 shares, back in namespace order
    w = 2 * k
    queries = [(axis, index, i, i + 1) for axis in (0, 1) for index in (0, k - 1, k, w - 1) for i in range(w)]
    queries += [(0, 1, 0, w), (1, 2, 3, 9)]
    with ctx.open_square(big) as sq:
        def snapshot():
            counts, nodes, shares = sq.prove(queries)
            descs = np.zeros(len(queries), N.NMT_PROOF_DESC_DTYPE)
            leaf_off, nsx = 0, []
            for i, (axis, index, s, e) in enumerate(queries):
                descs[i] = (s, e, i * nodes.shape[1], counts[i], leaf_off, axis * w + index)
                q0 = s < k and index < k
                nsx.append(shares[leaf_off, :NS].tobytes() if q0 else PARITY_SHARES_NAMESPACE)
                leaf_off += e - s
            ok = ctx.nmt_verify(descs, np.frombuffer(b"".join(nsx), np.uint8),
                                np.concatenate([sq.row_roots, sq.col_roots]), nodes.reshape(-1, N.NODE_SIZE), shares)
            return counts, nodes, shares, ok
        before = snapshot()
        res = sq.prove_namespace([(axis, index, nid) for axis in (0, 1) for index in range(w)
                                  for nid in query_namespaces(nss)])[0]
        assert set(res["kind"].tolist()) == {0, 1, 2}
        after = snapshot()
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert before[3][:-2].all()  # the one-cell proofs, each under its own leaf's namespace
