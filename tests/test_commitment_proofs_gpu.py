"""GPU tests of the blob commitment proofs: cda_square_commitment_proofs against the host prover over the
oracle's trees, byte for byte; Square.commitments against GetCommitment; cda_commitment_proofs_verify and _device
against CommitmentProof.verify_host, verdict by verdict, on every path of the fold kernels.
"""
import copy

import numpy as np
import pytest

import commitment_cases as K
import oracle_lib as O
from cda import _native as N
from cda import commitment as C
from cda import inclusion as I
from cda.appconsts import NAMESPACE_SIZE
from test_inclusion import mainnet_blobs, mainnet_ods
from test_square import mainnet_txs

pytestmark = pytest.mark.gpu


def check_prover(sq, host, blobs, threshold):
    """One call for `blobs`: every record, node, subtree root, aunt and commitment equals the host prover's."""
    k = host.k
    lg = (2 * k).bit_length() - 1
    raw = sq.commitment_proofs_raw(blobs, threshold)
    assert raw["data_root"] == host.dah == sq.dah
    assert raw["row_off"][0] == 0 and int(raw["row_off"][-1]) == len(raw["rows"])
    assert raw["nodes"].shape[1:] == (max(1, 2 * lg), N.NODE_SIZE) and raw["aunts"].shape[1:] == (lg + 1, 32)
    ns = bytes(NAMESPACE_SIZE)
    got = C.proofs_from_raw(raw, [ns] * len(blobs))
    root_cursor = 0
    for i, (start, n) in enumerate(blobs):
        want, commitment = host.prove(start, n, ns, threshold)
        assert got[i] == want, (k, threshold, start, n)
        assert raw["commitments"][i].tobytes() == commitment, (k, threshold, start, n)
        for r in range(int(raw["row_off"][i]), int(raw["row_off"][i + 1])):
            rec = raw["rows"][r]
            assert rec["node_off"] == r * raw["nodes"].shape[1] and rec["aunt_off"] == r * (lg + 1)
            assert rec["root_off"] == root_cursor and rec["row"] == rec["index"] and rec["pad_"] == 0
            assert not raw["nodes"][r, rec["nnodes"]:].any()
            root_cursor += int(rec["nroots"])
    assert root_cursor == len(raw["subtree_roots"])
    assert sq.commitments(blobs, threshold) == [x.tobytes() for x in raw["commitments"]]
    return raw


@pytest.mark.parametrize("k", [1, 2, 4])
def test_prover_every_aligned_blob(ctx, k):
    """k = 1, 2, 4 under thresholds 1, 2 and 64: every (start, len) a blob may have, one call per threshold."""
    ods = O.gen_ods(k, 0xC400 + k)
    host = K.HostSquare(ods)
    with ctx.open_square(ods) as sq:
        for threshold in (1, 2, 64):
            blobs = K.aligned_blobs(k, threshold)
            assert blobs and (0, k * k) in blobs
            check_prover(sq, host, blobs, threshold)


def special_blobs(k, threshold):
    """len = k^2, and blobs whose first row starts at k - W and whose last row is one share (0, 1 and k - 2 full rows
    between)."""
    out = [(0, k * k)]
    for m in (0, 1, k - 2):
        for W in (1 << i for i in range(k.bit_length())):
            n = W + m * k + 1
            if I.sub_tree_width(n, threshold) == W:
                out.append((k - W, n))
                break
    return out


@pytest.mark.parametrize("k", [8, 16])
def test_prover_sampled_blobs(ctx, k):
    """200 blobs per threshold, always with a first row that starts at k - W, a last row of one share and len = k^2."""
    ods = O.gen_ods(k, 0xC500 + k)
    host = K.HostSquare(ods)
    rng = np.random.default_rng(0xC5 + k)
    with ctx.open_square(ods) as sq:
        for threshold in (1, 2, 64):
            blobs = special_blobs(k, threshold)
            assert len(blobs) >= 3
            while len(blobs) < 200:
                n = int(rng.integers(1, k * k + 1)) if rng.random() < 0.5 else int(rng.integers(1, 3 * k))
                W = I.sub_tree_width(n, threshold)
                s = int(rng.integers(0, (k * k - n) // W + 1)) * W
                blobs.append((s, n))
            check_prover(sq, host, blobs, threshold)


def test_block_408_all_blobs_one_call(ctx):
    """Mainnet block 408: the commitments are the PFBs', the data root is the header's data_hash, and the proofs
    verify on the host and on the device."""
    data_hash = mainnet_txs()[1]
    ods, blobs = mainnet_ods(), mainnet_blobs()
    ranges = [(b["start"], b["n"]) for b in blobs]
    with ctx.open_square(ods) as sq:
        raw = sq.commitment_proofs_raw(ranges, 64)
        proofs = sq.commitment_proofs(ranges, [b["ns"] for b in blobs], 64)
        assert sq.commitments(ranges, 64) == [b["commitment"] for b in blobs]
    assert raw["data_root"] == data_hash
    assert [x.tobytes() for x in raw["commitments"]] == [b["commitment"] for b in blobs]
    for p, b in zip(proofs, blobs):
        assert p.verify_host(data_hash, b["commitment"], 64) == N.CP_VALID
    assert C.verify_commitment_proofs(ctx, proofs, data_hash, [b["commitment"] for b in blobs]) == [0] * len(blobs)


def test_commitments_equal_get_commitment_and_rejections(ctx):
    """Square.commitments equals inclusion.get_commitment per blob; an unaligned start, len = 0, a range past the ODS
    and a capacity one too small each give E_ARG before any device work: the device's free memory stays as it was."""
    import torch
    k = 8
    ods = O.gen_ods(k, 0xC600)
    cacher, dah = I.EDSSubTreeRootCacher.from_shares(list(ods), ctx)
    blobs = [(0, 1), (5, 3), (8, 17), (0, 64), (62, 2), (16, 40)]
    with ctx.open_square(ods) as sq:
        assert sq.commitments(blobs, 64) == [I.get_commitment(cacher, dah, s, n, 64, ctx) for s, n in blobs]
        assert sq.commitments([(8, 17), (0, 64)], 2) == [I.get_commitment(cacher, dah, s, n, 2, ctx)
                                                         for s, n in [(8, 17), (0, 64)]]
        good = sq.commitment_proofs_raw(blobs, 64)
        nrows, nroots = sq.commitment_proof_sizes(blobs, 64)
        assert (nrows, nroots) == (len(good["rows"]), len(good["subtree_roots"]))
        many = [(0, 1)] * 20000  # what staging these would take is far more than an allocation granule
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        for threshold, bad in ((1, (1, 2)), (64, (3, 0)), (64, (60, 5)), (64, (64, 1)), (0, (0, 1))):
            for call in (sq.commitments, sq.commitment_proofs_raw):
                with pytest.raises(N.CdaError) as e:
                    call(many + [bad], threshold)
                assert e.value.code == N.E_ARG, (threshold, bad)
        q = sq.blob_ranges(many)
        out = {name: np.zeros(shape, np.uint8) for name, shape in
               (("rows", (len(many) * 56,)), ("nodes", (len(many), 8, 90)), ("sub", (len(many), 90)),
                ("rr", (len(many), 90)), ("lh", (len(many), 32)), ("au", (len(many), 5, 32)), ("com", (len(many), 32)))}
        off, root = np.zeros(len(many) + 1, np.uint32), np.zeros(32, np.uint8)

        def call(max_nodes=8, rows_cap=len(many), roots_cap=len(many)):
            return ctx._L.cda_square_commitment_proofs(sq._h, len(q), N._p(q), 64, max_nodes, rows_cap, roots_cap,
                                                       N._p(off), N._p(out["rows"]), N._p(out["nodes"]), N._p(out["sub"]),
                                                       N._p(out["rr"]), N._p(out["lh"]), N._p(out["au"]),
                                                       N._p(out["com"]), N._p(root))
        assert call(max_nodes=7) == N.E_ARG
        assert call(rows_cap=len(many) - 1) == N.E_ARG
        assert call(roots_cap=len(many) - 1) == N.E_ARG
        assert not out["rows"].any() and not out["com"].any()  # nothing was written
        torch.cuda.synchronize()
        assert abs(torch.cuda.mem_get_info(0)[0] - free0) <= 2 << 20  # one allocation granule
        again = sq.commitment_proofs_raw(blobs, 64)
        for name in good:
            assert np.array_equal(good[name], again[name]), name


# ---- the verifier ----
def packed(cases):
    roots, coms = [c["data_root"] for c in cases], [c["commitment"] for c in cases]
    a = C.pack_commitment_proofs([c["proof"] for c in cases], list(range(len(cases))), list(range(len(cases))),
                                 [c["threshold"] for c in cases])
    a["data_roots"] = np.frombuffer(b"".join(roots), np.uint8).reshape(-1, 32)
    a["commitments"] = np.frombuffer(b"".join(coms), np.uint8).reshape(-1, 32)
    return a


ARRAYS = ("descs", "rows", "row_roots", "leaf_hashes", "nodes", "subtree_roots", "aunts", "data_roots", "commitments")


def host_form(ctx, a):
    return ctx.commitment_proofs_verify(*[a[name] for name in ARRAYS]).tolist()


def to_device(a):
    import torch
    dev = torch.device("cuda", 0)
    d = {name: torch.from_numpy(np.ascontiguousarray(a[name]).view(np.uint8).reshape(-1).copy()).to(dev)
         for name in ARRAYS}
    d["verdicts"] = torch.full((len(a["descs"]),), -1, dtype=torch.int32, device=dev)
    return d


def enqueue_device_form(ctx, a, d, stream=None):
    ctx.commitment_proofs_verify_device(len(a["descs"]), d["descs"].data_ptr(), d["rows"].data_ptr(),
                                        d["row_roots"].data_ptr(), d["leaf_hashes"].data_ptr(), len(a["rows"]),
                                        d["nodes"].data_ptr(), len(a["nodes"]), d["subtree_roots"].data_ptr(),
                                        len(a["subtree_roots"]), d["aunts"].data_ptr(), len(a["aunts"]),
                                        d["data_roots"].data_ptr(), len(a["data_roots"]), d["commitments"].data_ptr(),
                                        len(a["commitments"]), d["verdicts"].data_ptr(),
                                        stream.cuda_stream if stream is not None else None)


def device_form(ctx, a):
    import torch
    d = to_device(a)
    torch.cuda.synchronize()
    enqueue_device_form(ctx, a, d)
    torch.cuda.synchronize()
    return d["verdicts"].cpu().numpy().tolist()


def check_cases(ctx, cases, want=None):
    """Both forms give the host verifier's verdicts (and `want`, where the caller states them)."""
    host = [K.host_verdict(c) for c in cases]
    if want is not None:
        assert host == want
    a = packed(cases)
    assert host_form(ctx, a) == host
    assert device_form(ctx, a) == host
    return host


@pytest.mark.parametrize("k", [2, 8, 16])
def test_verifier_mutations(ctx, k):
    """The CPU test's mutation set: the valid proof, each of the nine verdicts by one named mutation, and every pair
    with the earlier rule's verdict, in one batch per form."""
    cases = K.mutation_cases(k)
    got = check_cases(ctx, [c for _, c, _ in cases], [w for _, _, w in cases])
    assert set(got) == set(range(10))


def test_verifier_batches_with_every_verdict(ctx):
    """Batches of 1, 31, 33 and 257 proofs with all ten verdicts mixed, and each verdict alone in a batch of one."""
    pool = [(c, w) for label, c, w in K.mutation_cases(8) if " & " not in label]
    assert sorted(w for _, w in pool) == list(range(10))
    for c, w in pool:
        check_cases(ctx, [c], [w])
    rng = np.random.default_rng(0xB7)
    for n in (31, 33, 257):
        pick = list(range(10)) + rng.integers(0, 10, n - 10).tolist()
        rng.shuffle(pick)
        check_cases(ctx, [pool[i][0] for i in pick], [pool[i][1] for i in pick])


def test_verifier_malformed_descriptors(ctx):
    """Descriptors and row records that point outside the totals are malformed and nothing is read through them; two
    descriptors that share row records are both malformed; the other proofs of the batch keep their verdicts."""
    base = K.base_case(8)
    a = packed([base, K.mutated(base, "commitment byte"), base, base])
    assert host_form(ctx, a) == [0, N.CP_COMMITMENT, 0, 0]
    nrows = len(a["rows"])
    for field, value in (("row_off", nrows), ("row_off", 0xFFFFFFFF), ("nrows", nrows + 1), ("nrows", 0xFFFFFFFF),
                         ("nrows", 0), ("data_root", 4), ("commitment", 4), ("commitment", 0xFFFFFFFF),
                         ("subtree_root_threshold", 0)):
        b = copy.deepcopy(a)
        b["descs"][2][field] = value
        assert host_form(ctx, b) == [0, N.CP_COMMITMENT, N.CP_MALFORMED, 0], (field, value)
        assert device_form(ctx, b) == [0, N.CP_COMMITMENT, N.CP_MALFORMED, 0], (field, value)
    for field in ("node_off", "nnodes", "root_off", "nroots", "aunt_off", "naunts"):
        b = copy.deepcopy(a)
        b["rows"][int(a["descs"][2]["row_off"]) + 1][field] = 0xFFFFFFF0
        assert host_form(ctx, b) == [0, N.CP_COMMITMENT, N.CP_MALFORMED, 0], field
    b = copy.deepcopy(a)
    b["descs"][2]["row_off"] = a["descs"][0]["row_off"]  # proof 0's records
    assert host_form(ctx, b) == [N.CP_MALFORMED, N.CP_COMMITMENT, N.CP_MALFORMED, 0]
    assert device_form(ctx, b) == [N.CP_MALFORMED, N.CP_COMMITMENT, N.CP_MALFORMED, 0]
    b["descs"][2]["row_off"] = a["descs"][0]["row_off"] + 1  # overlapping one of them
    b["descs"][2]["nrows"] = 1
    assert host_form(ctx, b) == [N.CP_MALFORMED, N.CP_COMMITMENT, N.CP_MALFORMED, 0]
    # misaligned device pointers are refused before any launch
    args = [ctx._h, 1, 4096, 4096, 4096, 4096, 1, 4096, 1, 4096, 1, 4096, 1, 4096, 1, 4096, 1, 4096, None]
    for at, ptr in ((3, 4100), (2, 4098), (9, 4097), (15, 4098)):
        bad = list(args)
        bad[at] = ptr
        assert ctx._L.cda_commitment_proofs_verify_device(*bad) == N.E_ARG, at


def uniform_square(k, seed):
    ods = O.gen_ods(k, seed)
    ods[:, :NAMESPACE_SIZE] = ods[0, :NAMESPACE_SIZE]  # one namespace: every range is a blob's
    return ods, ods[0, :NAMESPACE_SIZE].tobytes()


def cases_from_square(ctx, ods, ns, blobs, threshold):
    with ctx.open_square(ods) as sq:
        raw = sq.commitment_proofs_raw(blobs, threshold)
        proofs = C.proofs_from_raw(raw, [ns] * len(blobs))
    return [{"proof": p, "data_root": raw["data_root"], "commitment": raw["commitments"][i].tobytes(),
             "threshold": threshold} for i, p in enumerate(proofs)]


def flip_subtree_root(case, row, j):
    out = copy.deepcopy(case)
    roots = out["proof"].rows[row].subtree_roots
    roots[j] = K._flip(roots[j], 75)  # a digest byte: the namespace stays
    return out


def test_fold_paths_k64(ctx):
    """Rows on each side of the boundary between the chain kernel and the workgroup kernel, at k = 64: one root (a
    full row at W = 64; one share), a tail alone (tiles 2, 1 under W = 4; 4, 2, 1 under W = 32), one W-sized root plus
    a tail (two nodes at log2 W: the workgroup's smallest), 64 roots in a row (threshold 64, W = 1), and rows of
    several W-sized roots with a tail.  A digest byte flipped in a root of each kind fails that proof at C7."""
    k = 64
    ods, ns = uniform_square(k, 0xC764)
    t64 = cases_from_square(ctx, ods, ns, [(0, 1), (64, 64), (130, 61), (4 * k, 4 * k - 3), (9 * k + 5, 1)], 64)
    t1 = cases_from_square(ctx, ods, ns, [(0, k * k), (60, 7), (8, 5), (16, 13), (32, 21), (64, 51)], 1)
    t16 = cases_from_square(ctx, ods, ns, [(0, 7 * k + 7), (16, 130)], 16)
    assert [I.sub_tree_width(n, 1) for n in (k * k, 7, 5, 13, 21, 51)] == [64, 4, 4, 4, 8, 8]
    assert [I.sub_tree_width(n, 16) for n in (7 * k + 7, 130)] == [32, 16]
    assert [z for _, z in C.subtree_tiles(0, 3, 4)] == [2, 1] and len(t1[1]["proof"].rows[1].subtree_roots) == 2
    cases = t64 + t1 + t16
    assert len(cases[1]["proof"].rows[0].subtree_roots) == 64
    check_cases(ctx, cases, [0] * len(cases))
    bad = [flip_subtree_root(t64[1], 0, 63), flip_subtree_root(t64[3], 3, 0), flip_subtree_root(t1[0], 63, 0),
           flip_subtree_root(t1[1], 1, -1), flip_subtree_root(t1[1], 0, 0), flip_subtree_root(t1[2], 0, -1),
           flip_subtree_root(t1[3], 0, 0), flip_subtree_root(t1[4], 0, -1), flip_subtree_root(t1[5], 0, 6),
           flip_subtree_root(t16[0], 7, 1), flip_subtree_root(t16[0], 2, 1), flip_subtree_root(t16[1], 2, 1),
           flip_subtree_root(t64[0], 0, 0), flip_subtree_root(t64[2], 0, 30)]
    check_cases(ctx, bad + cases[:3], [N.CP_SUBTREE_ROOTS] * len(bad) + [0] * 3)


def test_fold_row_longer_than_one_chunk(ctx):
    """A hostile W = 1 descriptor at k = 1024, the smallest square in which a row has more level-log2 W nodes than the
    workgroup kernel's 512-node chunk: 1022 subtree roots [1, 1023) of one row, with a left hull node in front and
    nodes behind.  The tree is made on the host (the oracle's levels over synthetic leaf nodes); no square is
    extended.  Valid; a root of the second chunk, the first root and a proof node flipped: C7 each."""
    k, row = 1024, 5
    rng = np.random.default_rng(0xC71)
    ns = bytes(NAMESPACE_SIZE - 1) + b"\x07"
    leaves = np.zeros((2 * k, N.NODE_SIZE), np.uint8)
    leaves[:, 58:] = rng.integers(0, 256, (2 * k, 32), dtype=np.uint8)
    leaves[:k, :58] = np.frombuffer(ns * 2, np.uint8)
    leaves[k:, :58] = 0xFF
    tree = O.tree_levels(leaves)
    roots = [bytes(rng.integers(0, 256, N.NODE_SIZE, dtype=np.uint8)) for _ in range(4 * k)]
    roots[row] = tree[-1].tobytes()
    data_root, proofs = C.merkle_proofs(roots)
    threshold = 1 << 20
    proof, commitment = C.prove_host({row: tree}, roots, k, row * k + 1, k - 2, ns, threshold, proofs)
    assert len(proof.rows) == 1 and len(proof.rows[0].subtree_roots) == 1022 > 512
    assert len(proof.rows[0].nmt.nodes) == 1 + 2
    case = {"proof": proof, "data_root": data_root, "commitment": commitment, "threshold": threshold}
    late, first, node = flip_subtree_root(case, 0, 800), flip_subtree_root(case, 0, 0), K.mutated(case, "node digest byte")
    check_cases(ctx, [case, late, first, node, case], [0] + [N.CP_SUBTREE_ROOTS] * 3 + [0])


def test_k128_batch(ctx):
    """k = 128, threshold 64: a full-square blob (128 rows of one root), a blob of k + 1 shares and a one-share blob."""
    k = 128
    ods, ns = uniform_square(k, 0xC780)
    blobs = [(0, k * k), (3 * k + 124, k + 1), (77 * k + 19, 1)]
    cases = cases_from_square(ctx, ods, ns, blobs, 64)
    assert [len(c["proof"].rows) for c in cases] == [128, 2, 1]
    assert [len(c["proof"].subtree_roots()) for c in cases] == [128, 1 + 31 + 1, 1]
    a = packed(cases + [flip_subtree_root(cases[0], 127, 0), K.mutated(cases[1], "aunt byte")])
    want = [0, 0, 0, N.CP_SUBTREE_ROOTS, N.CP_ROW_PROOF]
    assert [K.host_verdict(c) for c in cases] == [0, 0, 0]
    assert host_form(ctx, a) == want and device_form(ctx, a) == want


def test_device_form_on_four_streams_and_isolation(ctx):
    """Four batches enqueued on four streams before any is waited for, each with its own verdicts; the same batches
    give the same verdicts after other calls on the context have used its workspace."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0xC74)
    pool = [(c, w) for label, c, w in K.mutation_cases(8) if " & " not in label]
    batches = []
    for n in (7, 33, 64, 129):
        pick = rng.integers(0, 10, n).tolist()
        batches.append((packed([pool[i][0] for i in pick]), [pool[i][1] for i in pick]))
    dd = [to_device(a) for a, _ in batches]
    streams = [torch.cuda.Stream(dev) for _ in batches]
    torch.cuda.synchronize()
    for (a, _), d, s in zip(batches, dd, streams):
        enqueue_device_form(ctx, a, d, s)
    for s in streams:
        s.synchronize()
    assert [d["verdicts"].cpu().numpy().tolist() for d in dd] == [w for _, w in batches]
    ctx.extend_commit(O.gen_ods(16, 0xB1))
    ns, blob = bytes(19) + bytes(range(10)), bytes(range(256)) * 40
    assert ctx.blob_commitments([ns], [blob])[0] == O.blob_commitment(ns, blob)[1]
    ods, uns = uniform_square(8, 0xC75)
    other = cases_from_square(ctx, ods, uns, [(0, 64), (3, 9)], 64)
    assert host_form(ctx, packed(other)) == [0, 0]
    for (a, want), d in zip(batches, dd):
        assert host_form(ctx, a) == want
        d["verdicts"].fill_(-1)
        torch.cuda.synchronize()
        enqueue_device_form(ctx, a, d)
        torch.cuda.synchronize()
        assert d["verdicts"].cpu().numpy().tolist() == want


def test_after_cda_free():
    """The prover on a square whose context was freed returns E_ARG, and close after cda_free is safe."""
    import cda
    c = cda.Context(0)
    sq = c.open_square(O.gen_ods(4, 0xC76))
    assert len(sq.commitments([(0, 2), (4, 9)])) == 2
    assert len(sq.commitment_proofs_raw([(0, 2)])["rows"]) == 1
    c.close()
    for call in (sq.commitments, sq.commitment_proofs_raw):
        with pytest.raises(N.CdaError) as e:
            call([(0, 2)])
        assert e.value.code == N.E_ARG
    sq.close()


def test_prove_verify_round_trip_on_device(ctx):
    """Proofs go from cda_square_commitment_proofs to cda_commitment_proofs_verify_device in device memory as they lie
    (node_off = r * max_nodes with the padded slots, aunt_off = r * log2(4k), the commitments and the data root where
    the prover wrote them): only the per-proof descriptors are made on the host, from the ranges alone.  The device
    outputs equal the host outputs; all valid; one byte flipped on the device in a subtree root of one proof, an aunt
    of another, a node of a third and the commitment of a fourth: exactly those fail, each at its rule; a byte flipped
    in a padded node slot changes nothing."""
    import torch
    dev = torch.device("cuda", 0)
    k, threshold = 8, 2
    ods, ns = uniform_square(k, 0xC77)
    blobs = [(s, n) for s, n in K.aligned_blobs(k, threshold) if s % 5 == 0 and n in (1, 3, 9, 17, 40, 64)]
    assert len(blobs) > 20 and (0, 64) in blobs
    with ctx.open_square(ods) as sq:
        host = sq.commitment_proofs_raw(blobs, threshold)
        nrows, nroots = sq.commitment_proof_sizes(blobs, threshold)
        mn, na = sq.max_nodes, (4 * k).bit_length() - 1
        z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        d = {"row_off": z((len(blobs) + 1) * 4), "rows": z(nrows * N.COMMITMENT_ROW_DTYPE.itemsize),
             "nodes": z(nrows, mn, N.NODE_SIZE), "subtree_roots": z(nroots, N.NODE_SIZE),
             "row_roots": z(nrows, N.NODE_SIZE), "leaf_hashes": z(nrows, 32), "aunts": z(nrows, na, 32),
             "commitments": z(len(blobs), 32), "data_root": z(32)}
        torch.cuda.synchronize()
        sq.commitment_proofs_device(blobs, threshold, mn, nrows, nroots, d["row_off"].data_ptr(), d["rows"].data_ptr(),
                                    d["nodes"].data_ptr(), d["subtree_roots"].data_ptr(), d["row_roots"].data_ptr(),
                                    d["leaf_hashes"].data_ptr(), d["aunts"].data_ptr(), d["commitments"].data_ptr(),
                                    d["data_root"].data_ptr())
    assert np.array_equal(d["row_off"].cpu().numpy().view(np.uint32), host["row_off"])
    assert np.array_equal(d["rows"].cpu().numpy().view(N.COMMITMENT_ROW_DTYPE), host["rows"])
    for name in ("nodes", "subtree_roots", "row_roots", "leaf_hashes", "aunts", "commitments"):
        assert np.array_equal(d[name].cpu().numpy(), host[name]), name
    assert d["data_root"].cpu().numpy().tobytes() == host["data_root"]
    descs = np.zeros(len(blobs), N.COMMITMENT_PROOF_DESC_DTYPE)
    row_off = [0]
    for i, (s, n) in enumerate(blobs):
        rows = C.blob_rows(k, s, n)
        descs[i] = (row_off[-1], len(rows), rows[0][0], rows[-1][0], 0, i, threshold, np.frombuffer(ns, np.uint8), 0)
        row_off.append(row_off[-1] + len(rows))
    assert row_off == host["row_off"].tolist()
    d_descs = torch.from_numpy(descs.view(np.uint8).reshape(-1).copy()).to(dev)
    d_verdicts = torch.full((len(blobs),), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()

    def verify():
        ctx.commitment_proofs_verify_device(len(blobs), d_descs.data_ptr(), d["rows"].data_ptr(),
                                            d["row_roots"].data_ptr(), d["leaf_hashes"].data_ptr(), nrows,
                                            d["nodes"].data_ptr(), nrows * mn, d["subtree_roots"].data_ptr(), nroots,
                                            d["aunts"].data_ptr(), nrows * na, d["data_root"].data_ptr(), 1,
                                            d["commitments"].data_ptr(), len(blobs), d_verdicts.data_ptr(),
                                            stream.cuda_stream)
        stream.synchronize()
        return d_verdicts.cpu().numpy().tolist()
    assert verify() == [0] * len(blobs)
    rec = host["rows"]
    r4, r9, r13 = row_off[4], row_off[9], row_off[13]
    assert int(rec[r13]["nnodes"]) < mn
    d["nodes"][r13, mn - 1, 70] ^= 1  # a padded slot: no proof reads it
    torch.cuda.synchronize()
    assert verify() == [0] * len(blobs)
    d["subtree_roots"][int(rec[r4]["root_off"]), 75] ^= 1
    d["aunts"][r9, 2, 5] ^= 1
    d["nodes"][r13, 0, 70] ^= 1
    d["commitments"][17, 3] ^= 1
    torch.cuda.synchronize()
    want = [0] * len(blobs)
    want[4], want[9], want[13], want[17] = N.CP_SUBTREE_ROOTS, N.CP_ROW_PROOF, N.CP_SUBTREE_ROOTS, N.CP_COMMITMENT
    assert verify() == want


def test_root_count_limit_of_one_proof(ctx):
    """C0's count limit on the device, by a hostile batch whose row records all point at one modest array of 1,024
    subtree roots: 257 records of 1,024 roots are 263,168 > 262,144 roots, malformed and not read through; 256
    records are exactly the limit, pass C0 and fail at the next rule that breaks (C1: the proof says one row).  The
    host verifier says the same of the same proofs."""
    from cda.proof import NMTProof, Proof, RowProof
    per, nsub = 1024, 1024
    sub = np.random.default_rng(0xC78).integers(0, 256, (nsub, N.NODE_SIZE), dtype=np.uint8)
    counts = (257, 256)
    rows = np.zeros(sum(counts), N.COMMITMENT_ROW_DTYPE)
    rows["nmt_end"], rows["nroots"], rows["total"] = 1, per, 4
    descs = np.zeros(2, N.COMMITMENT_PROOF_DESC_DTYPE)
    descs[0] = (0, counts[0], 0, 0, 0, 0, 64, np.zeros(29, np.uint8), 0)
    descs[1] = (counts[0], counts[1], 0, 0, 0, 0, 64, np.zeros(29, np.uint8), 0)
    a = {"descs": descs, "rows": rows, "row_roots": np.zeros((len(rows), N.NODE_SIZE), np.uint8),
         "leaf_hashes": np.zeros((len(rows), 32), np.uint8), "nodes": np.zeros((0, N.NODE_SIZE), np.uint8),
         "subtree_roots": sub, "aunts": np.zeros((0, 32), np.uint8), "data_roots": np.zeros((1, 32), np.uint8),
         "commitments": np.zeros((1, 32), np.uint8)}
    want = [N.CP_MALFORMED, N.CP_ROW_COUNT]
    node = sub[0].tobytes()
    for n, w in zip(counts, want):
        proof = C.CommitmentProof(bytes(29), [C.CommitmentRow([node] * per, NMTProof(0, 1, []))] * n,
                                  RowProof([bytes(N.NODE_SIZE)] * n, [Proof(4, 0, bytes(32), [])] * n, 0, 0))
        assert proof.verify_host(bytes(32), bytes(32), 64) == w
    assert host_form(ctx, a) == want
    assert device_form(ctx, a) == want
