"""GPU tests of reading a retained square back: cda_square_index against cda.blob.index_host, record for
record and commitment for commitment (the host's come from CreateCommitment over the parsed bytes, the device's from
the retained tree nodes), cda_square_read against the host strip, byte for byte with guard bytes around every output,
and the blob service calls on mainnet block 408 and on a square rebuilt from samples.
"""
import ctypes
import threading

import numpy as np
import pytest

import blob_cases as K
import oracle_lib as O
from cda import _native as N
from cda import blob as B
from cda import commitment as C
from cda import sampling
from cda import square as S
from test_inclusion import mainnet_blobs, mainnet_ods
from test_square import mainnet_txs

pytestmark = pytest.mark.gpu


def readable(seqs, k):
    return seqs[seqs["start"].astype(np.int64) + seqs["nshares"].astype(np.int64) <= k * k]


def check_square(ctx, sq, ods, k, threshold=64):
    """Index, commitments, summary and the payload of every sequence that lies inside the square equal the host's."""
    want_seqs, want_com, want_sum = B.index_host(list(ods), k, threshold, ctx=ctx)
    seqs, com, summary = sq.index(threshold)
    assert summary == want_sum
    assert seqs.tobytes() == want_seqs.tobytes()
    assert np.array_equal(com, want_com)
    nocom, none, s2 = sq.index(threshold, commitments=False)
    assert none is None and s2 == summary and nocom.tobytes() == seqs.tobytes()
    inside = readable(seqs, k)
    got = sq.read(inside)
    want = [B.strip_host(list(ods), int(s["start"]), int(s["nshares"]), int(s["seq_len"]),
                         s["kind"] != N.SEQ_KIND_BLOB) for s in inside]
    assert got == want
    return seqs, com, summary


# ---- index: synthetic squares ----
@pytest.mark.parametrize("k", [1, 2, 4, 8, 16])
def test_index_synthetic(ctx, k):
    ods, info = K.synthetic_square(k)
    with ctx.open_square(ods) as sq:
        seqs, com, summary = check_square(ctx, sq, ods, k)
        assert not seqs["status"].any() and summary["norphans"] == 0
        blobs = seqs[seqs["kind"] == N.SEQ_KIND_BLOB]
        assert sorted(blobs["start"].tolist()) == sorted(i for idx in info["pfb_share_indexes"] for i in idx)
        assert B.parse_txs(sq) == B.parse_txs(B.HostSquare(list(ods)))


def test_index_blob_across_scan_blocks(ctx):
    """k = 64: one blob from share 64 to past share 2,304, so its continuation shares and the padding behind it look
    back over several workgroups of the scan; then the same blob with a start bit set far inside it (share 2,100):
    the BROKEN bit reaches the record from another workgroup."""
    ods = K.long_blob_square()
    with ctx.open_square(ods) as sq:
        seqs, _, summary = check_square(ctx, sq, ods, 64)
        blob = seqs[seqs["kind"] == N.SEQ_KIND_BLOB][0]
        assert blob["start"] < 256 and blob["start"] + blob["nshares"] > 2304 and summary["norphans"] == 0
    bad = ods.copy()
    bad[2100, 29] |= 1
    rc, eds, _, _, _ = O.extend_commit(bad)
    assert rc == 0
    with ctx.open_square_eds(eds) as sq:
        seqs, _, _ = check_square(ctx, sq, bad, 64)
        assert seqs[seqs["start"] == blob["start"]][0]["status"] & N.SEQ_BROKEN


def test_index_k128_mix(ctx):
    """The k = 128 mix: 32 blobs placed by NextShareIndex; every commitment equals CreateCommitment of the bytes read
    back, which are the bytes that went in; all sequences in one read call."""
    ods, blobs = K.mix_square()
    assert len(blobs) == 32
    with ctx.open_square(ods) as sq:
        seqs, com, summary = check_square(ctx, sq, ods, 128)
        assert summary["nseq"] == 34 and not seqs["status"].any()
        found = seqs[seqs["kind"] == N.SEQ_KIND_BLOB]
        assert [(int(s["start"]), int(s["nshares"]), s["ns"].tobytes()) for s in found] == [b[:3] for b in blobs]
        assert sq.read(found) == [b[3] for b in blobs]
        got, flagged = B.get_all(sq, [blobs[3][2], blobs[17][2]])
        assert flagged == [] and [(b.start, b.data) for b in got] == [(blobs[i][0], blobs[i][3]) for i in (3, 17)]
        assert sq.commitments([(b.start, b.nshares) for b in got]) == [b.commitment for b in got]


# ---- index: block 408 ----
def test_index_block_408_both_ways(ctx):
    ods = mainnet_ods()
    with ctx.open_square(ods) as sq:
        seqs, com, _ = check_square(ctx, sq, ods, 32)
        eds = ctx.extend_commit(ods)[0]
    (want,) = mainnet_blobs()
    assert com[2].tobytes() == want["commitment"] and len(seqs) == 3
    with ctx.open_square_eds(eds) as sq:
        again, com2, _ = check_square(ctx, sq, ods, 32)
    assert again.tobytes() == seqs.tobytes() and np.array_equal(com, com2)


# ---- index: hostile squares ----
def hostile_cases():
    names = [m[0] for m in K.MUTATIONS]
    out = [(n,) for n in names] + [(a, b) for i, a in enumerate(names) for b in names[i + 1:]]
    return out


def test_index_hostile_squares(ctx):
    """Each status bit from one named mutation of a valid k = 8 square, every pair of mutations, an orphan run at share
    0, a square of continuation shares only and a k = 4 square whose last blob claims shares past k^2: statuses, never
    an error, equal to the host's; and the device's free memory is what it was."""
    import torch
    squares = [(K.mutated(8, *names), names) for names in hostile_cases()]
    squares += [({"ods": K.orphan_run_square(), "k": 8, "threshold": 64}, ("orphan run",)),
                ({"ods": K.continuation_only_square(), "k": 8, "threshold": 64}, ("continuations only",)),
                (K.mutated(4, K.MUTATIONS[0][0]), ("k = 4 truncated",))]
    squares += [({"ods": ods, "k": 8, "threshold": 64}, ("huge length",)) for ods in K.huge_length_squares()]
    seen = 0
    for case, names in squares:
        rc, eds, _, _, _ = O.extend_commit(case["ods"])
        assert rc == 0, names
        with ctx.open_square_eds(eds) as sq:
            seqs, _, summary = check_square(ctx, sq, case["ods"], case["k"], case["threshold"])
        bits = int(np.bitwise_or.reduce(seqs["status"])) if len(seqs) else 0
        for name in names:
            bit = next((b for n, b, _ in K.MUTATIONS if n == name), 0)
            assert bits & bit == bit, names
        seen |= bits
        if names == ("orphan run",):
            assert summary["first_orphan"] == 0 and summary["norphans"] >= 2
        if names == ("continuations only",):
            assert summary["nseq"] == 0 and summary["norphans"] == 64
        if names == ("k = 4 truncated",):
            assert seqs[-1]["start"] + seqs[-1]["nshares"] > 16
        if names == ("huge length",):  # the claim is millions of shares: truncated, never a clean one-share blob
            big = seqs[seqs["seq_len"] >= 0xFFFFFFFE]
            assert len(big) >= 1 and (big["status"] & N.SEQ_TRUNCATED).all() and (big["nshares"] > 8000000).all()
    assert seen == 31
    # every workspace has its size by now: a second pass over all of them leaves the device's free memory the same
    edss = [O.extend_commit(case["ods"])[1] for case, _ in squares]
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    for (case, _), eds in zip(squares, edss):
        with ctx.open_square_eds(eds) as sq:
            seqs, _, _ = sq.index(case["threshold"])
            sq.read(readable(seqs, case["k"]))
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] == free1


# ---- index: output and cap forms ----
def test_index_cap_and_device_outputs(ctx):
    import torch
    dev = torch.device("cuda", 0)
    ods, _ = K.synthetic_square(8)
    with ctx.open_square(ods) as sq:
        seqs, com, summary = sq.index(64)
        nseq = len(seqs)
        assert nseq >= 5
        # cap < nseq: exactly cap records and commitments, nothing after them
        cap = 3
        recs = np.full((cap + 2) * 48, 0xAB, np.uint8)
        coms = np.full((cap + 2, 32), 0xAB, np.uint8)
        s = N.SquareSummary()
        assert ctx._L.cda_square_index(sq._h, 64, cap, N._p(recs), N._p(coms), ctypes.byref(s)) == N.OK
        assert s.nseq == nseq
        assert recs[:cap * 48].tobytes() == seqs[:cap].tobytes() and (recs[cap * 48:] == 0xAB).all()
        assert np.array_equal(coms[:cap], com[:cap]) and (coms[cap:] == 0xAB).all()
        # Square.index retries once when its first guess was too small
        again, com2, _ = sq.index(64, cap=1)
        assert again.tobytes() == seqs.tobytes() and np.array_equal(com2, com)
        # cap == 0 and no records: the summary alone
        s = N.SquareSummary()
        assert ctx._L.cda_square_index(sq._h, 0, 0, None, None, ctypes.byref(s)) == N.OK
        assert (s.nseq, s.npadding, s.norphans) == (nseq, summary["npadding"], 0)
        # outputs in device memory
        d_recs = torch.full(((nseq + 1) * 48,), 0xAB, dtype=torch.uint8, device=dev)
        d_com = torch.full((nseq + 1, 32), 0xAB, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        s = N.SquareSummary()
        V = ctypes.c_void_p
        assert ctx._L.cda_square_index(sq._h, 64, nseq, V(d_recs.data_ptr()), V(d_com.data_ptr()),
                                       ctypes.byref(s)) == N.OK
        got = d_recs.cpu().numpy()
        assert got[:nseq * 48].tobytes() == seqs.tobytes() and (got[nseq * 48:] == 0xAB).all()
        got = d_com.cpu().numpy()
        assert np.array_equal(got[:nseq], com) and (got[nseq:] == 0xAB).all()
        # rejections: nothing written
        for args in ((sq._h, 0, 1, N._p(recs), N._p(coms), ctypes.byref(s)), (sq._h, 64, 1, None, None, ctypes.byref(s)),
                     (sq._h, 64, 1, N._p(recs), None, None), (None, 64, 1, N._p(recs), None, ctypes.byref(s))):
            before = recs.copy()
            assert ctx._L.cda_square_index(*args) == N.E_ARG
            assert np.array_equal(recs, before)


# ---- read: lengths and offsets ----
BLOB_LENGTHS = [1, 477, 478, 479, 959, 960, 961, 478 + 2 * 482]  # 478, 960 and 1,442 end exactly at a share's end
COMPACT_LENGTHS = [474, 475, 952]
GUARD = 64


def read_cases(k):
    """(start, nshares, seq_len, compact) of every length at every phase 0..15, spread over the square."""
    out = []
    for compact, lengths in ((0, BLOB_LENGTHS), (1, COMPACT_LENGTHS)):
        for n in lengths:
            need = (S.compact_shares_needed(n) if compact else B.inclusion.sparse_shares_needed(n))
            for phase in range(16):
                start = (len(out) * 5) % (k * k - need + 1)
                out.append((start, need, n, compact, phase))
    return out


def layout(cases, base_addr):
    """Offsets with GUARD bytes on both sides of every output and (base_addr + offset) % 16 == phase."""
    offs, cursor = [], 0
    for _, _, n, _, phase in cases:
        at = cursor + GUARD
        at += (phase - (base_addr + at)) % 16
        offs.append(at)
        cursor = at + n + GUARD
    return np.array(offs, np.uint64), cursor + 16


def check_outputs(buf, cases, offs, ods):
    mask = np.ones(len(buf), bool)
    for (start, need, n, compact, _), off in zip(cases, offs):
        off = int(off)
        assert buf[off:off + n].tobytes() == B.strip_host(list(ods), start, need, n, bool(compact)), (start, n, compact)
        mask[off:off + n] = False
    assert (buf[mask] == 0xA5).all()  # guards and gaps as they were


def test_read_lengths_and_offsets(ctx):
    import torch
    dev = torch.device("cuda", 0)
    k = 4
    ods = O.gen_ods(k, 0xB1EAD)
    cases = read_cases(k)
    q = np.array([c[:4] for c in cases], N.SEQUENCE_RANGE_DTYPE)
    with ctx.open_square(ods) as sq:
        # device memory: the kernel writes at these very phases
        size = layout(cases, 0)[1] + 16 * len(cases)  # room for every phase shift
        d = torch.full((size,), 0xA5, dtype=torch.uint8, device=dev)
        offs, total = layout(cases, d.data_ptr())
        assert total <= size
        assert all((d.data_ptr() + int(o)) % 16 == c[4] for o, c in zip(offs, cases))
        torch.cuda.synchronize()
        sq.read_device(q, offs, size, d.data_ptr())
        check_outputs(d.cpu().numpy(), cases, offs, ods)
        # host memory
        h = np.full(size, 0xA5, np.uint8)
        offs, total = layout(cases, h.ctypes.data)
        assert total <= size
        assert ctx._L.cda_square_read(sq._h, len(q), N._p(q), N._p(offs), len(h), N._p(h)) == N.OK
        check_outputs(h, cases, offs, ods)
        # Square.read packs them back to back
        assert sq.read(q) == [B.strip_host(list(ods), c[0], c[1], c[2], bool(c[3])) for c in cases]


def test_read_row_boundary_k2(ctx):
    """A blob of two shares at shares 1 and 2 of a k = 2 square: its second share lies in the next row of the EDS."""
    data = bytes(range(256)) * 3 + b"tail"
    shares = S.compact_shares(S.TX_NAMESPACE, [b"tx" * 50]) + S.sparse_shares(K.blob_ns(3), data)
    shares += [S.padding_share(S.TAIL_PADDING_NAMESPACE)]
    ods = K.ods_array(shares)
    assert len(ods) == 4
    with ctx.open_square(ods) as sq:
        seqs, _, _ = check_square(ctx, sq, ods, 2)
        assert (int(seqs[1]["start"]), int(seqs[1]["nshares"])) == (1, 2) and sq.read(seqs[1:2]) == [data]
        assert B.get_all(sq)[0][0].data == data


def test_read_rejections(ctx):
    ods, _ = K.synthetic_square(4)
    with ctx.open_square(ods) as sq:
        out = np.full(4096, 0xA5, np.uint8)

        def call(q, off, cap=len(out), handle=sq._h, data=out):
            q = np.array([q], N.SEQUENCE_RANGE_DTYPE)
            off = np.array([off], np.uint64)
            return ctx._L.cda_square_read(handle, 1, N._p(q), N._p(off), cap, N._p(data) if data is not None else None)
        assert call((0, 1, 100, 1), 0) == N.OK and (out[100:] == 0xA5).all()
        out[:] = 0xA5
        for q, off, kw in [((15, 2, 10, 0), 0, {}), ((16, 1, 10, 0), 0, {}), ((0, 1, 479, 0), 0, {}),
                           ((0, 1, 475, 1), 0, {}), ((0, 0, 1, 0), 0, {}), ((0, 2, 500, 0), 4000, {}),
                           ((0, 1, 0xFFFFFFFE, 0), 0, {"cap": 1 << 33}), ((0, 16, 0xFFFFFFFF, 1), 0, {"cap": 1 << 33}),
                           ((0, 1, 10, 0), 5000, {}), ((0, 1, 10, 0), 0, {"cap": 9}), ((0, 1, 10, 0), 0, {"handle": None}),
                           ((0, 1, 10, 0), 0, {"data": None})]:
            assert call(q, off, **kw) == N.E_ARG, (q, off, kw)
        assert (out == 0xA5).all()
        assert call((0, 4, 0, 0), 4096) == N.OK and (out == 0xA5).all()  # nothing to copy, at the very end


# ---- service level ----
def test_blob_service_on_block_408(ctx):
    data_hash = mainnet_txs()[1]
    (want,) = mainnet_blobs()
    with ctx.open_square(mainnet_ods()) as sq:
        assert sq.dah == data_hash
        b = B.get(sq, want["ns"], want["commitment"])
        assert (b.data, b.start, b.nshares, b.share_version) == (want["data"], want["start"], want["n"], want["version"])
        assert B.included(sq, want["ns"], want["commitment"])
        proof = B.get_proof(sq, want["ns"], want["commitment"])
        assert proof.verify_host(data_hash, want["commitment"], 64) == N.CP_VALID
        assert C.verify_commitment_proofs(ctx, [proof], data_hash, [want["commitment"]]) == [N.CP_VALID]
        flipped = want["commitment"][:5] + bytes([want["commitment"][5] ^ 0x40]) + want["commitment"][6:]
        assert not B.included(sq, want["ns"], flipped)
        assert not B.included(sq, K.blob_ns(77), want["commitment"])
        for call in (B.get, B.get_proof):
            with pytest.raises(B.BlobNotFound):
                call(sq, want["ns"], flipped)
        normal, pfbs, idx = B.parse_txs(sq)
        txs = mainnet_txs()[0]
        assert normal == [t for t in txs if S.unmarshal_blob_tx(t) is None] and idx == [[want["start"]]]


def test_blobs_of_a_rebuilt_square(ctx):
    """A square made by sampling.rebuild from proved samples (Q0 and three cells in ten of the rest) gives the blobs of
    the square the samples came from."""
    k = 8
    ods, _ = K.synthetic_square(k)
    w = 2 * k
    rng = np.random.default_rng(0xB1B)
    keep = rng.random((w, w)) < 0.3
    keep[:k, :k] = True
    coords = [(int(r), int(c)) for r, c in zip(*np.nonzero(keep))]
    with ctx.open_square(ods) as src:
        want, flagged = B.get_all(src)
        assert want and flagged == []
        samples = sampling.sample_proofs(src, coords, 0)
        rr, cr, dah = src.row_roots.copy(), src.col_roots.copy(), src.dah
    sq, _, _ = sampling.rebuild(ctx, samples, rr, cr)
    with sq:
        assert sq.dah == dah
        got, flagged = B.get_all(sq)
        assert got == want and flagged == []
        check_square(ctx, sq, ods, k)


# ---- concurrency and lifetime ----
def test_three_threads_on_one_square(ctx):
    ods, blobs = K.mix_square()
    with ctx.open_square(ods) as sq:
        seqs, com, summary = sq.index(64)
        datas = sq.read(seqs)
        ranges = [(int(s["start"]), int(s["start"]) + min(int(s["nshares"]), 3)) for s in seqs[2:8]]
        proofs = sq.share_proofs_raw(ranges)
        errors = []

        def indexer():
            try:
                for _ in range(4):
                    s2, c2, m2 = sq.index(64)
                    assert s2.tobytes() == seqs.tobytes() and np.array_equal(c2, com) and m2 == summary
                    assert sq.read(s2[:6]) == datas[:6]
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        def prover():
            try:
                for _ in range(8):
                    again = sq.share_proofs_raw(ranges)
                    assert all(np.array_equal(again[x], proofs[x]) for x in ("rows", "nodes", "shares", "aunts"))
            except Exception as e:  # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=f) for f in (indexer, indexer, prover)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert errors == []


def test_after_cda_free():
    """Index and read on a square whose context was freed return E_ARG, and close after cda_free is safe."""
    import cda
    c = cda.Context(0)
    ods, _ = K.synthetic_square(4)
    sq = c.open_square(ods)
    seqs, _, _ = sq.index(64)
    assert len(sq.read(seqs)) == len(seqs)
    c.close()
    for call in (lambda: sq.index(64), lambda: sq.read(seqs)):
        with pytest.raises(N.CdaError) as e:
            call()
        assert e.value.code == N.E_ARG
    sq.close()
