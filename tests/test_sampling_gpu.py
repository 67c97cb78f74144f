"""GPU tests of the sample proofs: cda_square_open / cda_square_prove against the host wrapper tree (hashlib), and
cda_nmt_verify / cda_nmt_verify_device against cda.proof.NMTProof.verify_inclusion, element by element.

Every comparison of proofs is byte-exact; every comparison of verdicts is with the host function the reference's
share_proof_test.go vectors pin (tests/test_inclusion.py).
"""
import os
import random

import numpy as np
import pytest

import oracle_lib as O
import test_sampling as TS
from cda import _native as N
from cda import sampling
from cda.appconsts import NAMESPACE_SIZE, PARITY_SHARES_NAMESPACE
from cda.proof import NMTProof
from cda.wrapper import ErasuredNamespacedMerkleTree
from test_inclusion import GOLDEN, mainnet_blobs, mainnet_ods

pytestmark = pytest.mark.gpu


def axis_cells(eds, w, axis, index):
    grid = eds.reshape(w, w, N.SHARE_SIZE)
    return grid[:, index] if axis else grid[index]


def host_tree(eds, k, axis, index):
    """wrapper.ErasuredNamespacedMerkleTree fed axis (axis, index) of the EDS: the host (hashlib) prover."""
    t = ErasuredNamespacedMerkleTree(k, index)
    t._leaves = [bytes(x) for x in axis_cells(eds, 2 * k, axis, index)]
    return t


def check_proofs(eds, k, queries, counts, nodes, shares, trees=None):
    """counts / nodes / shares of Square.prove equal prove_range and the EDS cells, query by query."""
    trees = {} if trees is None else trees
    w, cursor = 2 * k, 0
    for i, (axis, index, start, end) in enumerate(queries):
        key = (axis, index)
        if key not in trees:
            trees[key] = host_tree(eds, k, axis, index)
        want = trees[key].prove_range(start, end).nodes
        assert counts[i] == len(want), (k, axis, index, start, end)
        assert [nodes[i, j].tobytes() for j in range(counts[i])] == want, (k, axis, index, start, end)
        assert not nodes[i, counts[i]:].any()
        if shares is not None:
            assert np.array_equal(shares[cursor:cursor + end - start], axis_cells(eds, w, axis, index)[start:end])
            cursor += end - start
    if shares is not None:
        assert cursor == len(shares)


@pytest.mark.parametrize("k", [1, 2, 4, 16])
def test_prove_every_cell(ctx, k):
    """Every cell of the 2k x 2k square against its row root and against its column root (the reference's
    nmt_wrapper_test.go:151-180, for all 4k trees): nodes and counts as prove_range, cells as the EDS, roots and DAH
    as extend_commit.  k = 1: trees of 2 leaves, proofs of 1 node; k = 2: the first size with nodes on both sides."""
    ods = O.gen_ods(k, 0x5A00 + k)
    eds, rr, cr, dah = ctx.extend_commit(ods)
    w = 2 * k
    with ctx.open_square(ods) as sq:
        assert np.array_equal(sq.row_roots, rr) and np.array_equal(sq.col_roots, cr) and sq.dah == dah
        queries = [(axis, index, i, i + 1) for axis in (0, 1) for index in range(w) for i in range(w)]
        counts, nodes, shares = sq.prove(queries)
        assert nodes.shape == (len(queries), max(1, sq.max_nodes), N.NODE_SIZE)
        check_proofs(eds, k, queries, counts, nodes, shares)
        if k == 1:
            assert set(counts) == {1}
        # without the cells: the same proofs
        c2, n2, s2 = sq.prove(queries, want_shares=False)
        assert s2 is None and np.array_equal(c2, counts) and np.array_equal(n2, nodes)


@pytest.mark.parametrize("k", [4, 16])
def test_prove_ranges(ctx, k):
    """Every (start, end) of one Q0 row, one parity row and one column crossing Q0 -> Q2, the full axis included
    (zero nodes)."""
    ods = O.gen_ods(k, 0x5B00 + k)
    eds = ctx.extend_commit(ods)[0]
    w = 2 * k
    with ctx.open_square(ods) as sq:
        queries = [(axis, index, s, e) for axis, index in ((0, 1), (0, k + 1), (1, k - 1))
                   for s in range(w) for e in range(s + 1, w + 1)]
        counts, nodes, shares = sq.prove(queries)
        check_proofs(eds, k, queries, counts, nodes, shares)
        full = [i for i, q in enumerate(queries) if q[2:] == (0, w)]
        assert len(full) == 3 and all(counts[i] == 0 for i in full)


def test_prove_rejects_bad_queries(ctx):
    k = 4
    with ctx.open_square(O.gen_ods(k, 3)) as sq:
        for bad in [(2, 0, 0, 1), (0, 8, 0, 1), (0, 0, 3, 3), (0, 0, 4, 2), (0, 0, 0, 9), (1, 0, 8, 9)]:
            with pytest.raises(N.CdaError) as e:
                sq.prove([(0, 0, 0, 1), bad])
            assert e.value.code == N.E_ARG
        q = np.array([(0, 0, 0, 2)], N.RANGE_QUERY_DTYPE)
        counts, nodes = np.zeros(1, np.int32), np.zeros((1, 6, N.NODE_SIZE), np.uint8)
        small = np.zeros((1, N.SHARE_SIZE), np.uint8)
        L = ctx._L
        assert L.cda_square_prove(sq._h, 1, N._p(q), 5, N._p(counts), N._p(nodes), None, 0) == N.E_ARG  # max_nodes
        assert L.cda_square_prove(sq._h, 1, N._p(q), 6, N._p(counts), N._p(nodes), N._p(small), 512) == N.E_ARG
        assert L.cda_square_prove(sq._h, 1, N._p(q), 6, N._p(counts), N._p(nodes), None, 0) == N.OK


def test_square_isolation(ctx):
    """A retained square is untouched by other work on its context -- another block through extend_commit, blob
    commitments -- and by a second open square."""
    k = 8
    ods_a, ods_b = O.gen_ods(k, 0xA), O.gen_ods(16, 0xB)
    w = 2 * k
    queries = [(axis, index, i, i + 1) for axis in (0, 1) for index in (0, k - 1, k, w - 1) for i in range(w)]
    queries += [(0, 3, 1, w - 1), (1, k, 0, w)]
    a = ctx.open_square(ods_a)
    try:
        before = a.prove(queries)
        eds_b = ctx.extend_commit(ods_b)[0]
        ns, blob = bytes(19) + bytes(range(10)), bytes(range(256)) * 40
        assert ctx.blob_commitments([ns], [blob])[0] == O.blob_commitment(ns, blob)[1]
        ctx.extend_commit_nodes(ods_b)
        with ctx.open_square(ods_b) as b:
            qb = [(axis, index, i, i + 1) for axis in (0, 1) for index in (0, 31) for i in range(32)]
            check_proofs(eds_b, 16, qb, *b.prove(qb))
            after = a.prove(queries)
        again = a.prove(queries)
        for x, y, z in zip(before, after, again):
            assert np.array_equal(x, y) and np.array_equal(x, z)
        check_proofs(ctx.extend_commit(ods_a)[0], k, queries, *before)
    finally:
        a.close()


def test_square_outlives_its_context_safely():
    """cda_free of a context with an open square releases the square's device memory; the handle is then good for
    close alone (prove answers CDA_E_ARG)."""
    import cda
    c = cda.Context(0)
    sq = c.open_square(O.gen_ods(2, 1))
    assert sq.prove([(0, 0, 0, 1)])[0][0] == 2
    c.close()
    counts, nodes = np.zeros(1, np.int32), np.zeros((1, 4, N.NODE_SIZE), np.uint8)
    q = np.array([(0, 0, 0, 1)], N.RANGE_QUERY_DTYPE)
    assert sq._ctx._L.cda_square_prove(sq._h, 1, N._p(q), 4, N._p(counts), N._p(nodes), None, 0) == N.E_ARG
    sq.close()


def test_block_408_proofs(ctx):
    """Mainnet block 408: for the row ranges of its share proofs (the blob's shares, a range inside the blob, and
    row 0 [0, 1): the range of the reference's share_proof_test.go fixture) cda_square_prove gives the NMT proofs
    cda_share_inclusion_proof returns, and cda_nmt_verify accepts them against the block's row roots.  (The fixture's
    own nodes carry 33-byte namespaces, an older namespace size: they stay with the host verifier in
    tests/test_inclusion.py.)"""
    import json
    fx = json.load(open(os.path.join(GOLDEN, "share_proof_fixture.json")))
    assert len(bytes.fromhex(fx["nmt"]["nodes"][0])) != N.NODE_SIZE
    ods = mainnet_ods()
    k = int(round(len(ods) ** 0.5))
    b = mainnet_blobs()[0]
    first = fx["start_row"] * k + fx["nmt"]["start"]
    ranges = [(b["start"], b["start"] + b["n"]), (b["start"] + 5, b["start"] + 40),
              (first, first + fx["nmt"]["end"] - fx["nmt"]["start"])]
    with ctx.open_square(ods) as sq:
        assert sq.dah == np.load(os.path.join(GOLDEN, "mainnet_h408.npz"))["data_hash"].tobytes()
        queries, want, nss = [], [], []
        for start, end in ranges:
            p = ctx.share_inclusion_proof(ods, start, end)
            for i, row in enumerate(p["rows"]):
                queries.append((0, p["start_row"] + i, row["start"], row["end"]))
                want.append(row["nodes"])
                nss.append(ods[start][:NAMESPACE_SIZE].tobytes())
                assert row["row_root"] == sq.row_roots[p["start_row"] + i].tobytes()
        counts, nodes, shares = sq.prove(queries)
        for i, w_nodes in enumerate(want):
            assert [nodes[i, j].tobytes() for j in range(counts[i])] == w_nodes, queries[i]
        descs = np.zeros(len(queries), N.NMT_PROOF_DESC_DTYPE)
        flat, leaf_off = [], 0
        for i, (_, row, s, e) in enumerate(queries):
            descs[i] = (s, e, len(flat), counts[i], leaf_off, row)
            flat += [nodes[i, j] for j in range(counts[i])]
            leaf_off += e - s
        ok = ctx.nmt_verify(descs, np.frombuffer(b"".join(nss), np.uint8), sq.row_roots, np.stack(flat), shares)
        assert ok.tolist() == [1] * len(queries)
        host = [NMTProof(s, e, want[i]).verify_inclusion(nss[i], [bytes(x) for x in shares[d["leaf_off"]:
                                                                       d["leaf_off"] + e - s]],
                                                         sq.row_roots[row].tobytes())
                for i, ((_, row, s, e), d) in enumerate(zip(queries, descs))]
        assert all(host)


class Batch:
    """A cda_nmt_verify batch built case by case, with the host verdict of every case."""

    def __init__(self):
        self.descs, self.ns, self.roots, self.nodes, self.leaves, self.want = [], [], [], [], [], []

    def add(self, start, end, nodes, ns, leaves, root):
        self.want.append(NMTProof(start, end, nodes).verify_inclusion(ns, leaves, root))
        self.descs.append((start, end, len(self.nodes), len(nodes), len(self.leaves), len(self.roots)))
        self.ns.append(bytes(ns))
        self.roots.append(bytes(root))
        self.nodes += [bytes(x) for x in nodes]
        self.leaves += [bytes(x) for x in leaves]

    def arrays(self):
        u8 = lambda rows, n: np.frombuffer(b"".join(rows), np.uint8).reshape(-1, n)  # noqa: E731
        return (np.array(self.descs, N.NMT_PROOF_DESC_DTYPE), u8(self.ns, NAMESPACE_SIZE), u8(self.roots, N.NODE_SIZE),
                u8(self.nodes, N.NODE_SIZE), u8(self.leaves, N.SHARE_SIZE))


def square_cases(ctx, batch, k, seed):
    """Proofs of a k x k block's square, ranges of length 1, 2, 3 and 2k on Q0, parity and crossing axes; under the
    range's first leaf's namespace (a range over two namespaces is then a proof the host rejects)."""
    ods = O.gen_ods(k, seed)
    eds = ctx.extend_commit(ods)[0]
    w = 2 * k
    with ctx.open_square(ods) as sq:
        queries = []
        for axis in (0, 1):
            for index in (0, k - 1, k, w - 1):
                queries += [(axis, index, s, s + n) for n in (1, 2, 3, w) for s in range(0, w - n + 1)]
        counts, nodes, shares = sq.prove(queries)
        cursor = 0
        roots = (sq.row_roots, sq.col_roots)
        for i, (axis, index, s, e) in enumerate(queries):
            cells = [bytes(x) for x in shares[cursor:cursor + e - s]]
            cursor += e - s
            ns = sampling.sample_namespace(k, axis, index, s, cells[0])
            batch.add(s, e, [nodes[i, j].tobytes() for j in range(counts[i])], ns, cells, roots[axis][index].tobytes())
    return eds


def test_verify_matches_host_verdict(ctx):
    """The mutation set of tests/test_sampling.py (trees of 1..32 leaves, leaf counts that are no power of two), proofs
    from squares of k = 2 and k = 8, and descriptors that point outside the totals, in ONE batch: every verdict is
    verify_inclusion's."""
    batch = Batch()
    for kind, start, end, nodes, ns, leaves, root in TS.cases(0xC0DE, 1200):
        batch.add(start, end, nodes, ns, leaves, root)
    n_mut = len(batch.want)
    square_cases(ctx, batch, 2, 21)
    square_cases(ctx, batch, 8, 22)
    descs, ns, roots, nodes, leaves = batch.arrays()
    want = list(batch.want)
    # descriptors outside the totals (verdict 0, nothing read through them), copies of a proof the host accepts
    good = next(i for i, d in enumerate(descs) if want[i] and d["nnodes"] > 0)
    extra = []
    for field, value in (("node_off", len(nodes) - descs[good]["nnodes"] + 1), ("node_off", 0xFFFFFFF0),
                         ("leaf_off", len(leaves)), ("leaf_off", 0xFFFFFFFF), ("root", len(roots)),
                         ("nnodes", len(nodes) + 1), ("end", int(descs[good]["start"]))):
        d = descs[good].copy()
        d[field] = value
        extra.append(d)
    d = descs[good].copy()
    d["end"] = d["start"] + len(leaves) + 1  # leaf_off + (end - start) past the total
    extra.append(d)
    descs = np.concatenate([descs, np.array(extra, N.NMT_PROOF_DESC_DTYPE)])
    ns = np.concatenate([ns, np.repeat(ns[good:good + 1], len(extra), 0)])
    want += [False] * len(extra)
    ok = ctx.nmt_verify(descs, ns, roots, nodes, leaves)
    assert set(ok.tolist()) <= {0, 1}
    wrong = [i for i in range(len(want)) if bool(ok[i]) != want[i]]
    assert not wrong, [(i, descs[i], want[i]) for i in wrong[:8]]
    assert sum(want[:n_mut]) >= 100 and n_mut - sum(want[:n_mut]) >= 100, (sum(want[:n_mut]), n_mut)
    assert sum(want[n_mut:]) >= 100  # the squares' own proofs


def synthetic_tree(n, seed):
    """(leaves, leaf nodes, root) of an all-parity erasured tree of n leaves: hashlib."""
    rng = np.random.default_rng(seed)
    t = ErasuredNamespacedMerkleTree(1, 1)
    t._leaves = [bytes(x) for x in rng.integers(0, 256, (n, N.SHARE_SIZE), dtype=np.uint8)]
    return t, TS.tree_root(t._leaf_nodes())


@pytest.mark.parametrize("n,ranges", [
    (1500, [(0, 1500), (500, 1030), (511, 513), (512, 1024), (1023, 1500), (1, 2), (1499, 1500), (0, 513)]),
    (65536, [(1, 65536), (33000, 65535)]),
])
def test_verify_long_ranges(ctx, n, ranges):
    """Ranges longer than one 512-leaf chunk of the range kernel (chunk boundaries inside, at and off the range's
    ends; a leaf count that is no power of two) and the widest axis (65,536 leaves: all 128 chunk roots in use),
    valid and with one leaf flipped, against the host verdict."""
    t, root = synthetic_tree(n, n)
    batch = Batch()
    rng = random.Random(n)
    for s, e in ranges:
        p = t.prove_range(s, e)
        leaves = t._leaves[s:e]
        batch.add(s, e, p.nodes, PARITY_SHARES_NAMESPACE, leaves, root)
        if n > 4096:
            continue  # one host verification of the widest axis costs as much as the rest of the test
        bad = list(leaves)
        i = rng.randrange(len(bad))
        bad[i] = TS._flip(bad[i], rng)
        batch.add(s, e, p.nodes, PARITY_SHARES_NAMESPACE, bad, root)
        if p.nodes:
            batch.add(s, e, p.nodes[:-1], PARITY_SHARES_NAMESPACE, leaves, root)
    ok = ctx.nmt_verify(*batch.arrays())
    assert [bool(x) for x in ok] == batch.want
    assert any(batch.want)


def test_verify_rejects_wide_end_and_bad_pointers(ctx):
    """end > 65536: CDA_E_ARG in the host form, verdict 0 in the device form (test_pipeline_k128 covers that form)."""
    d = np.array([(0, 65537, 0, 0, 0, 0)], N.NMT_PROOF_DESC_DTYPE)
    with pytest.raises(N.CdaError) as e:
        ctx.nmt_verify(d, np.zeros((1, NAMESPACE_SIZE), np.uint8), np.zeros((1, 90), np.uint8),
                       np.zeros((0, 90), np.uint8), np.zeros((1, 512), np.uint8))
    assert e.value.code == N.E_ARG
    assert ctx._L.cda_nmt_verify(ctx._h, 1, None, None, None, 0, None, 0, None, 0, None) == N.E_ARG
    assert ctx._L.cda_nmt_verify_device(ctx._h, 1, None, None, None, 0, None, 0, None, 0, None, None) == N.E_ARG
    # misaligned device pointers are refused before any launch
    assert ctx._L.cda_nmt_verify_device(ctx._h, 1, 4096, 4096, 4096, 1, 4096, 0, 4097, 1, 4096, None) == N.E_ARG
    assert ctx._L.cda_nmt_verify_device(ctx._h, 1, 4096, 4096, 4098, 1, 4096, 0, 4096, 1, 4096, None) == N.E_ARG


def test_sample_proofs_and_verify_samples(ctx):
    """cda.sampling end to end: cells proved against row and column roots verify; a cell under the wrong root, a
    corrupted cell and a cell claimed at another position do not."""
    k = 4
    ods = O.gen_ods(k, 77)
    coords = [(r, c) for r in range(2 * k) for c in range(2 * k)]
    with ctx.open_square(ods) as sq:
        samples = sampling.sample_proofs(sq, coords, 0) + sampling.sample_proofs(sq, coords, 1)
        rr, cr = sq.row_roots, sq.col_roots
    assert all(sampling.verify_samples(ctx, samples, rr, cr))
    axis, index, pos, share, proof = samples[5]
    bad = [(axis, (index + 1) % (2 * k), pos, share, proof),
           (axis, index, pos, share[:100] + bytes([share[100] ^ 1]) + share[101:], proof),
           (axis, index, pos + 1, share, NMTProof(pos + 1, pos + 2, proof.nodes))]
    assert sampling.verify_samples(ctx, bad + samples[:3], rr, cr) == [False] * 3 + [True] * 3


def test_pipeline_k128(ctx):
    """The workload's own size, without the proofs leaving the GPU: open a k = 128 square, prove all 65,536 cells on
    the row axis into device memory, verify them there with cda_nmt_verify_device: all 1; 256 random proofs also pass
    verify_inclusion on the host; one byte flipped in each of 16 random cells on the device: exactly those 16 turn 0;
    a descriptor with end > 65536 gets 0."""
    import torch
    k, w = 128, 256
    nq, mn = w * w, 16
    ods = O.gen_ods(k, 0x128)
    dev = torch.device("cuda", 0)
    d_counts = torch.zeros(nq, dtype=torch.int32, device=dev)
    d_nodes = torch.zeros((nq, mn, N.NODE_SIZE), dtype=torch.uint8, device=dev)
    d_shares = torch.zeros((nq, N.SHARE_SIZE), dtype=torch.uint8, device=dev)
    q = np.zeros(nq, N.RANGE_QUERY_DTYPE)
    q["index"], q["start"] = np.divmod(np.arange(nq, dtype=np.uint32), w)
    q["end"] = q["start"] + 1
    torch.cuda.synchronize()
    with ctx.open_square(ods) as sq:
        sq.prove_device(q, mn, d_counts.data_ptr(), d_nodes.data_ptr(), d_shares.data_ptr(), d_shares.numel())
        roots = np.concatenate([sq.row_roots, sq.col_roots])
    counts = d_counts.cpu().numpy()
    assert (counts == 8).all()
    descs = np.zeros(nq + 1, N.NMT_PROOF_DESC_DTYPE)
    descs["start"][:nq], descs["end"][:nq] = q["start"], q["end"]
    descs["node_off"][:nq] = np.arange(nq, dtype=np.uint32) * mn
    descs["nnodes"][:nq] = counts
    descs["leaf_off"][:nq] = np.arange(nq, dtype=np.uint32)
    descs["root"][:nq] = q["index"]
    descs[nq] = (65536, 65537, 0, 8, 0, 0)  # wider than any axis: verdict 0 in the device form
    ns = np.full((nq + 1, NAMESPACE_SIZE), 0xFF, np.uint8)
    q0 = (q["index"] < k) & (q["start"] < k)
    eds_q0 = ods.reshape(k, k, N.SHARE_SIZE)[:, :, :NAMESPACE_SIZE].reshape(-1, NAMESPACE_SIZE)
    ns[:nq][q0] = eds_q0
    d_descs = torch.from_numpy(descs.view(np.uint8).reshape(-1)).to(dev)
    d_ns = torch.from_numpy(ns.reshape(-1)).to(dev)
    d_roots = torch.from_numpy(roots.reshape(-1)).to(dev)
    d_ok = torch.full((nq + 1,), 7, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()

    def verify():
        ctx.nmt_verify_device(nq + 1, d_descs.data_ptr(), d_ns.data_ptr(), d_roots.data_ptr(), len(roots),
                              d_nodes.data_ptr(), nq * mn, d_shares.data_ptr(), nq, d_ok.data_ptr(),
                              stream.cuda_stream)
        stream.synchronize()
        return d_ok.cpu().numpy()

    ok = verify()
    assert ok[:nq].all() and set(ok[:nq].tolist()) == {1} and ok[nq] == 0
    rng = np.random.default_rng(128)
    pick = rng.choice(nq, 256, replace=False)
    idx = torch.from_numpy(pick.astype(np.int64)).to(dev)
    h_nodes, h_shares = d_nodes[idx].cpu().numpy(), d_shares[idx].cpu().numpy()
    for j, i in enumerate(pick):
        p = NMTProof(int(q["start"][i]), int(q["end"][i]), [h_nodes[j, t].tobytes() for t in range(8)])
        assert p.verify_inclusion(ns[i].tobytes(), [h_shares[j].tobytes()], roots[q["index"][i]].tobytes()), i
    flip = rng.choice(nq, 16, replace=False)
    cols = rng.integers(0, N.SHARE_SIZE, 16)
    fi, fc = torch.from_numpy(flip.astype(np.int64)).to(dev), torch.from_numpy(cols.astype(np.int64)).to(dev)
    d_shares[fi, fc] ^= 0x40
    torch.cuda.synchronize()
    ok2 = verify()
    assert sorted(np.flatnonzero(ok2[:nq] == 0).tolist()) == sorted(flip.tolist()) and ok2[nq] == 0
