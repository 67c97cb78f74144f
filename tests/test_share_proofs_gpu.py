"""GPU tests of the share proofs to the data root: cda_square_share_proofs against cda_share_inclusion_proof (itself
pinned to the oracle by tests/test_inclusion_gpu.py), field by field and byte-exact, and cda_share_proofs_validate /
_device against cda.proof.ShareProof.validate, message by message.
"""
import copy

import numpy as np
import pytest

import oracle_lib as O
from cda import _native as N
from cda import proof as P
from cda import square as S
from cda.appconsts import NAMESPACE_SIZE
from test_inclusion import mainnet_blobs, mainnet_ods
from test_share_proofs import mainnet_txs

pytestmark = pytest.mark.gpu


def all_ranges(k):
    return [(s, e) for s in range(k * k) for e in range(s + 1, k * k + 1)]


def check_against_reference(ctx, ods, k, ranges, raw):
    """Every field cda_square_share_proofs wrote for `ranges` equals cda_share_inclusion_proof's for the same range
    of the same ODS; the shares equal the ODS."""
    lg = (2 * k).bit_length() - 1
    assert raw["row_off"][0] == 0 and len(raw["row_off"]) == len(ranges) + 1
    assert raw["nodes"].shape[1:] == (max(1, 2 * lg), N.NODE_SIZE) and raw["aunts"].shape[1:] == (lg + 1, 32)
    cursor = 0
    for i, (s, e) in enumerate(ranges):
        want = ctx.share_inclusion_proof(ods, s, e)
        lo, hi = int(raw["row_off"][i]), int(raw["row_off"][i + 1])
        assert hi - lo == len(want["rows"]) == want["end_row"] - want["start_row"] + 1, (k, s, e)
        assert raw["data_root"] == want["data_root"]
        for j, row in enumerate(want["rows"]):
            r, rec = lo + j, raw["rows"][lo + j]
            assert (rec["row"], rec["index"], rec["total"]) == (want["start_row"] + j, want["start_row"] + j,
                                                                 want["total"]), (k, s, e, j)
            assert (rec["nmt_start"], rec["nmt_end"], rec["nnodes"]) == (row["start"], row["end"],
                                                                         len(row["nodes"])), (k, s, e, j)
            assert rec["node_off"] == r * raw["nodes"].shape[1] and rec["aunt_off"] == r * (lg + 1)
            assert rec["naunts"] == lg + 1 == len(row["aunts"]) and rec["pad_"] == 0
            assert [raw["nodes"][r, t].tobytes() for t in range(rec["nnodes"])] == row["nodes"], (k, s, e, j)
            assert not raw["nodes"][r, rec["nnodes"]:].any()
            assert raw["row_roots"][r].tobytes() == row["row_root"]
            assert raw["leaf_hashes"][r].tobytes() == row["leaf_hash"]
            assert [raw["aunts"][r, t].tobytes() for t in range(lg + 1)] == row["aunts"], (k, s, e, j)
        assert np.array_equal(raw["shares"][cursor:cursor + e - s], ods[s:e]), (k, s, e)
        cursor += e - s
    assert cursor == len(raw["shares"]) and int(raw["row_off"][-1]) == len(raw["rows"])


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_every_range_one_launch(ctx, k):
    """Every share range of the square (1, 10, 136 and 2,080 ranges) in ONE call per k.  k = 1: 2 aunts and a 1-node
    proof; k = 2: the first proofs of two rows; k = 4: first / middle / last rows."""
    ods = O.gen_ods(k, 0x5C00 + k)
    ranges = all_ranges(k)
    assert len(ranges) == {1: 1, 2: 10, 4: 136, 8: 2080}[k]
    with ctx.open_square(ods) as sq:
        raw = sq.share_proofs_raw(ranges)
        assert raw["data_root"] == sq.dah
        check_against_reference(ctx, ods, k, ranges, raw)
        if k == 1:
            assert raw["aunts"].shape[1] == 2 and raw["rows"]["nnodes"].tolist() == [1]
        # without the shares: the same proofs
        raw2 = sq.share_proofs_raw(ranges, want_shares=False)
        assert raw2["shares"] is None
        for name in ("row_off", "rows", "nodes", "row_roots", "leaf_hashes", "aunts", "data_root"):
            assert np.array_equal(raw2[name], raw[name]), name


@pytest.mark.parametrize("k", [4, 32])
def test_whole_square(ctx, k):
    """TestAllSharesInclusionProof (pkg/proof/proof_test.go:234-260): (0, k*k) proves k rows of [0, k), each with
    exactly one node (the parity half of its row), and validates."""
    ods = O.gen_ods(k, 0x5D00 + k)
    ods[:, :NAMESPACE_SIZE] = ods[0, :NAMESPACE_SIZE]  # one namespace, as the reference's test square
    with ctx.open_square(ods) as sq:
        raw = sq.share_proofs_raw([(0, k * k)])
        assert raw["row_off"].tolist() == [0, k] and raw["rows"]["nnodes"].tolist() == [1] * k
        assert raw["rows"]["nmt_start"].tolist() == [0] * k and raw["rows"]["nmt_end"].tolist() == [k] * k
        assert np.array_equal(raw["shares"], ods)
        if k == 4:
            check_against_reference(ctx, ods, k, [(0, k * k)], raw)
        proof, = sq.share_proofs([(0, k * k)])
        proof.validate(sq.dah)
        assert P.validate_share_proofs(ctx, [proof], sq.dah) == [None]


def test_block_408_every_tx_and_the_blob(ctx):
    """Mainnet block 408: ONE call proves the shares of each of its 274 txs (find_tx_share_range; the BlobTx under
    PAY_FOR_BLOB) and the PFB's blob; every proof validates against the header's data_hash on the host and on the
    GPU.  new_tx_inclusion_proof through the retained square returns the same proofs."""
    txs, data_hash = mainnet_txs()
    ods = mainnet_ods()
    b = mainnet_blobs()[0]
    ranges = S.tx_share_ranges(txs, 128, 64) + [(b["start"], b["start"] + b["n"])]
    nss = [S.PAY_FOR_BLOB_NAMESPACE if S.unmarshal_blob_tx(t) is not None else S.TX_NAMESPACE for t in txs]
    nss.append(ods[b["start"], :NAMESPACE_SIZE].tobytes())
    assert len(ranges) == 275 and nss.count(S.PAY_FOR_BLOB_NAMESPACE) == 1
    with ctx.open_square(ods) as sq:
        assert sq.dah == data_hash
        proofs = sq.share_proofs(ranges, nss)
        for i in (0, 137, 273):
            got = P.new_tx_inclusion_proof(txs, i, square=sq, max_square_size=128, subtree_root_threshold=64)
            assert got == proofs[i]
        assert P.new_share_inclusion_proof([bytes(x) for x in ods], nss[-1], *ranges[-1], square=sq) == proofs[-1]
    for p, (s, e) in zip(proofs, ranges):
        assert p.data == [ods[i].tobytes() for i in range(s, e)]
        p.validate(data_hash)
    assert P.validate_share_proofs(ctx, proofs, data_hash) == [None] * len(proofs)
    # against another root every one fails at the row proof, on the host and on the GPU alike
    errs = P.validate_share_proofs(ctx, proofs[:4], bytes(32))
    assert [str(x) for x in errs] == ["row proof failed to verify"] * 4


def test_k128_ranges(ctx):
    """k = 128: the first share, the last share, 500 shares crossing rows and the whole square in one call."""
    k = 128
    ods = O.gen_ods(k, 0x5E80)
    ranges = [(0, 1), (k * k - 1, k * k), (3 * k + 77, 3 * k + 577), (0, k * k)]
    with ctx.open_square(ods) as sq:
        raw = sq.share_proofs_raw(ranges)
    assert raw["row_off"].tolist() == [0, 1, 2, 7, 7 + k]
    check_against_reference(ctx, ods, k, ranges, raw)


def _device_outputs(sq, ranges, dev):
    import torch
    k = sq.k
    nrows, nshares = sq.share_proof_sizes(k, ranges)
    mn, na = max(1, sq.max_nodes), (4 * k).bit_length() - 1
    z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    d = {"row_off": z((len(ranges) + 1) * 4), "rows": z(nrows * N.SHARE_ROW_DTYPE.itemsize),
         "nodes": z(nrows, mn, N.NODE_SIZE), "row_roots": z(nrows, N.NODE_SIZE), "leaf_hashes": z(nrows, 32),
         "aunts": z(nrows, na, 32), "shares": z(nshares, N.SHARE_SIZE), "data_root": z(32)}
    torch.cuda.synchronize()
    sq.share_proofs_device(ranges, mn, nrows, d["row_off"].data_ptr(), d["rows"].data_ptr(), d["nodes"].data_ptr(),
                           d["row_roots"].data_ptr(), d["leaf_hashes"].data_ptr(), d["aunts"].data_ptr(),
                           d["shares"].data_ptr(), d["shares"].numel(), d["data_root"].data_ptr())
    return d


def _assert_device_equals_host(d, raw):
    assert np.array_equal(d["row_off"].cpu().numpy().view(np.uint32), raw["row_off"])
    assert np.array_equal(d["rows"].cpu().numpy().view(N.SHARE_ROW_DTYPE), raw["rows"])
    for name in ("nodes", "row_roots", "leaf_hashes", "aunts", "shares"):
        assert np.array_equal(d[name].cpu().numpy(), raw[name]), name
    assert d["data_root"].cpu().numpy().tobytes() == raw["data_root"]


def test_device_outputs_and_isolation(ctx):
    """Outputs in device memory equal outputs in host memory, and the call gives the same after other work on the
    context: another extend_commit, blob commitments, the node export, a second open square."""
    import torch
    dev = torch.device("cuda", 0)
    k = 8
    ods_a, ods_b = O.gen_ods(k, 0xA1), O.gen_ods(16, 0xB1)
    ranges = [(0, 1), (5, 23), (k * k - 9, k * k), (0, k * k), (17, 18)]
    a = ctx.open_square(ods_a)
    try:
        before = a.share_proofs_raw(ranges)
        _assert_device_equals_host(_device_outputs(a, ranges, dev), before)
        ctx.extend_commit(ods_b)
        ns, blob = bytes(19) + bytes(range(10)), bytes(range(256)) * 40
        assert ctx.blob_commitments([ns], [blob])[0] == O.blob_commitment(ns, blob)[1]
        ctx.extend_commit_nodes(ods_b)
        with ctx.open_square(ods_b) as b:
            rb = [(3, 40), (255, 256)]
            check_against_reference(ctx, ods_b, 16, rb, b.share_proofs_raw(rb))
            after = a.share_proofs_raw(ranges)
        again = a.share_proofs_raw(ranges)
        for name in before:
            assert np.array_equal(before[name], after[name]) and np.array_equal(before[name], again[name]), name
        _assert_device_equals_host(_device_outputs(a, ranges, dev), before)
        check_against_reference(ctx, ods_a, k, ranges, before)
    finally:
        a.close()


def test_rejections(ctx):
    """CDA_E_ARG before any launch for a bad range or a capacity too small; a later good call still works; a
    detached handle answers CDA_E_ARG."""
    import cda
    k = 4
    ods = O.gen_ods(k, 9)
    with ctx.open_square(ods) as sq:
        good = sq.share_proofs_raw([(1, 7)])
        for bad in [(3, 3), (5, 2), (0, k * k + 1), (k * k, k * k + 1)]:
            with pytest.raises(N.CdaError) as e:
                sq.share_proofs_raw([(0, 1), bad])
            assert e.value.code == N.E_ARG, bad
        q = np.array([(1, 7)], N.SHARE_RANGE_DTYPE)  # two rows, six shares, max_nodes 6, 4 aunts
        off, rows = np.zeros(2, np.uint32), np.zeros(2, N.SHARE_ROW_DTYPE)
        nodes, rr = np.zeros((2, 6, N.NODE_SIZE), np.uint8), np.zeros((2, N.NODE_SIZE), np.uint8)
        lh, au = np.zeros((2, 32), np.uint8), np.zeros((2, 4, 32), np.uint8)
        sh, root = np.zeros((6, N.SHARE_SIZE), np.uint8), np.zeros(32, np.uint8)

        def call(max_nodes=6, rows_cap=2, shares_cap=6 * N.SHARE_SIZE):
            return ctx._L.cda_square_share_proofs(sq._h, 1, N._p(q), max_nodes, rows_cap, N._p(off), N._p(rows),
                                                  N._p(nodes), N._p(rr), N._p(lh), N._p(au), N._p(sh), shares_cap,
                                                  N._p(root))
        assert call(max_nodes=5) == N.E_ARG
        assert call(rows_cap=1) == N.E_ARG
        assert call(shares_cap=6 * N.SHARE_SIZE - 1) == N.E_ARG
        assert not rows["total"].any() and not sh.any()  # nothing was written
        assert call() == N.OK
        assert np.array_equal(rows, good["rows"]) and np.array_equal(sh, good["shares"]) and \
            np.array_equal(nodes, good["nodes"]) and root.tobytes() == good["data_root"] == sq.dah
    c = cda.Context(0)
    sq = c.open_square(ods)
    assert len(sq.share_proofs_raw([(0, 2)])["rows"]) == 1
    c.close()
    with pytest.raises(N.CdaError) as e:
        sq.share_proofs_raw([(0, 2)])
    assert e.value.code == N.E_ARG
    sq.close()


# ---- validate ----
def host_error(proof, root):
    try:
        proof.validate(root)
        return None
    except P.ProofError as e:
        return str(e)


def _flip(b, i=7):
    out = bytearray(b)
    out[i % len(out)] ^= 0x10
    return bytes(out)


def tampers(proof, root, k):
    """(name, proof, root) for one tamper at a time of a valid proof."""
    out = []

    def case(name, fn, new_root=None):
        p = copy.deepcopy(proof)
        fn(p)
        out.append((name, p, new_root or root))
    last = len(proof.share_proofs) - 1
    case("share byte", lambda p: p.data.__setitem__(0, _flip(p.data[0], 300)))
    case("last share byte", lambda p: p.data.__setitem__(-1, _flip(p.data[-1], 511)))
    case("node byte", lambda p: p.share_proofs[last].nodes.__setitem__(0, _flip(p.share_proofs[last].nodes[0], 60)))
    case("row root byte", lambda p: p.row_proof.row_roots.__setitem__(0, _flip(p.row_proof.row_roots[0], 80)))
    case("row root namespace byte", lambda p: p.row_proof.row_roots.__setitem__(last, _flip(p.row_proof.row_roots[last], 3)))
    case("leaf hash byte", lambda p: setattr(p.row_proof.proofs[0], "leaf_hash", _flip(p.row_proof.proofs[0].leaf_hash)))
    case("aunt byte", lambda p: p.row_proof.proofs[last].aunts.__setitem__(1, _flip(p.row_proof.proofs[last].aunts[1])))
    case("data root byte", lambda p: None, _flip(root))
    case("namespace byte", lambda p: setattr(p, "namespace_id", _flip(p.namespace_id, 20)))
    case("namespace version", lambda p: setattr(p, "namespace_version", p.namespace_version ^ 1))
    for d in (1, -1):
        case(f"index {d:+d}", lambda p, d=d: setattr(p.row_proof.proofs[0], "index", p.row_proof.proofs[0].index + d))
    for t in (4 * k + 1, 4 * k - 1, 2 * 4 * k, 0, -1):
        case(f"total {t}", lambda p, t=t: setattr(p.row_proof.proofs[last], "total", t))
    case("aunt dropped", lambda p: p.row_proof.proofs[0].aunts.pop())
    case("first aunt dropped", lambda p: p.row_proof.proofs[0].aunts.pop(0))
    case("aunt added", lambda p: p.row_proof.proofs[0].aunts.append(bytes(32)))
    case("101 aunts", lambda p: setattr(p.row_proof.proofs[0], "aunts", [bytes(32)] * 101))
    for ds, de in ((1, 0), (0, -1), (0, 1), (1, 1), (-1, -1)):
        def shift(p, ds=ds, de=de):
            p.share_proofs[0].start += ds
            p.share_proofs[0].end += de
        case(f"nmt range {ds:+d} {de:+d}", shift)

    def negative(p):  # the same length, so that the count check passes and the sign check is reached
        sp = p.share_proofs[0]
        sp.start, sp.end = -1, sp.end - sp.start - 1
    case("negative start", negative)

    def empty(p):  # the first row proves nothing and its shares are gone: counts match, the range check is reached
        sp = p.share_proofs[0]
        del p.data[:sp.end - sp.start]
        sp.end = sp.start
    case("empty range", empty)

    case("share proof dropped", lambda p: p.share_proofs.pop())
    case("row root dropped", lambda p: p.row_proof.row_roots.pop())
    case("row proof dropped", lambda p: p.row_proof.proofs.pop())
    case("row record dropped", lambda p: (p.share_proofs.pop(), p.row_proof.row_roots.pop(), p.row_proof.proofs.pop()))
    case("end row + 1", lambda p: setattr(p.row_proof, "end_row", p.row_proof.end_row + 1))
    case("start row + 1", lambda p: setattr(p.row_proof, "start_row", p.row_proof.start_row + 1))
    case("share dropped", lambda p: p.data.pop())
    case("share added", lambda p: p.data.append(p.data[0]))
    case("node dropped", lambda p: p.share_proofs[last].nodes.pop())
    case("node added", lambda p: p.share_proofs[0].nodes.append(p.share_proofs[0].nodes[0]))
    return out


def test_validate_exhaustive_k4_and_tampers(ctx):
    """Every proof of the exhaustive k = 4 batch gets verdict 0 (and validates on the host); then one tamper at a
    time of a one-row, a two-row and a three-row proof, all in one batch: each verdict maps to the very message the
    host ShareProof.validate raises (None where the tamper leaves the proof valid)."""
    k = 4
    ods = O.gen_ods(k, 0x5F04)
    ods[:, :NAMESPACE_SIZE] = ods[0, :NAMESPACE_SIZE]  # one namespace: every range is a proof the reference builds
    ranges = all_ranges(k)
    with ctx.open_square(ods) as sq:
        proofs = sq.share_proofs(ranges)
        root = sq.dah
    assert P.validate_share_proofs(ctx, proofs, root) == [None] * len(proofs)
    for p in proofs:
        p.validate(root)
    cases = []
    for r in ((5, 7), (2, 7), (3, 14)):
        cases += tampers(proofs[ranges.index(r)], root, k)
    got = P.validate_share_proofs(ctx, [c[1] for c in cases], [c[2] for c in cases])
    want = [host_error(c[1], c[2]) for c in cases]
    wrong = [(c[0], w, str(g)) for c, w, g in zip(cases, want, got) if (None if g is None else str(g)) != w]
    assert not wrong, wrong[:6]
    # every check of Validate is reached by some tamper, and some tampers leave the proof valid
    seen = {w for w in want}
    for frag in ("number of share proofs", "number of shares", "index cannot be negative", "total must be positive",
                 "number of rows", "number of proofs", "row proof failed", "share proof failed"):
        assert any(w and frag in w for w in seen), frag


def test_validate_reference_case_shapes(ctx):
    """The cases of TestShareProofValidate / TestRowProofValidate (tests/test_inclusion.py runs them on the
    reference's 33-byte-namespace vector, which the 29-byte C records cannot hold) on a proof of a k = 4 square: empty
    row proof, mismatched row roots / proofs / rows, fewer share proofs, more shares, an incorrect root, tampered
    data.  (A ShareProof without data, "empty share proof", has no flat form: host only.)"""
    k = 4
    ods = O.gen_ods(k, 0x5F05)
    ods[:, :NAMESPACE_SIZE] = ods[0, :NAMESPACE_SIZE]
    with ctx.open_square(ods) as sq:
        sp, = sq.share_proofs([(1, 3)])
        root = sq.dah
    cases = [P.ShareProof([], [], sp.namespace_id, P.RowProof([], [], 0, 0), sp.namespace_version)]
    for field in ("row_roots", "proofs"):
        c = copy.deepcopy(sp)
        setattr(c.row_proof, field, [])
        cases.append(c)
    c = copy.deepcopy(sp)
    c.row_proof.end_row = 10
    cases.append(c)
    c = copy.deepcopy(sp)
    c.share_proofs = []
    cases.append(c)
    c = copy.deepcopy(sp)
    c.data = c.data + [c.data[0]]
    cases.append(c)
    c = copy.deepcopy(sp)
    c.data[0] = _flip(c.data[0], 100)
    cases.append(c)
    roots = [root] * len(cases) + [bytes(32)]
    cases.append(copy.deepcopy(sp))
    cases.append(sp)
    roots.append(root)
    got = P.validate_share_proofs(ctx, cases, roots)
    want = [host_error(c, r) for c, r in zip(cases, roots)]
    assert [None if g is None else str(g) for g in got] == want
    assert all(w is not None for w in want[:-1]) and want[-1] is None


def test_validate_mixed_batch_two_squares(ctx):
    """One batch with the proofs of two squares (k = 2 and k = 8) and two data roots, interleaved; each proof against
    the other square's root fails at the row proof."""
    proofs, roots = [], []
    dah = {}
    for k in (2, 8):
        ods = O.gen_ods(k, 0x5F10 + k)
        ods[:, :NAMESPACE_SIZE] = ods[0, :NAMESPACE_SIZE]
        with ctx.open_square(ods) as sq:
            rs = all_ranges(k) if k == 2 else [(0, 1), (7, 9), (0, 64), (13, 50), (63, 64)]
            proofs += sq.share_proofs(rs)
            roots += [sq.dah] * len(rs)
            dah[k] = sq.dah
    order = np.random.default_rng(5).permutation(len(proofs))
    proofs, roots = [proofs[i] for i in order], [roots[i] for i in order]
    assert P.validate_share_proofs(ctx, proofs, roots) == [None] * len(proofs)
    swapped = [dah[2] if r == dah[8] else dah[8] for r in roots]
    assert [str(x) for x in P.validate_share_proofs(ctx, proofs, swapped)] == ["row proof failed to verify"] * len(proofs)


def _descs_for(raw, ranges, k, ns, data_root=0):
    """The per-proof descriptors of the proofs cda_square_share_proofs wrote for `ranges` (all that validate needs
    beyond the arrays as they lie)."""
    d = np.zeros(len(ranges), N.SHARE_PROOF_DESC_DTYPE)
    leaf = 0
    for i, (s, e) in enumerate(ranges):
        lo, n = int(raw["row_off"][i]), int(raw["row_off"][i + 1] - raw["row_off"][i])
        d[i] = (lo, n, n, n, leaf, e - s, s // k, (e - 1) // k, data_root, np.frombuffer(ns, np.uint8), 0)
        leaf += e - s
    return d


def test_validate_malformed_descriptors(ctx):
    """A descriptor that points outside the totals gets the malformed verdict and nothing is read through it; two
    proofs that share row records are both malformed; a row record whose nodes or aunts lie outside the totals fails
    its leg; the good proofs of the same batch stay valid."""
    k = 4
    ods = O.gen_ods(k, 0x5F06)
    ods[:, :NAMESPACE_SIZE] = ods[0, :NAMESPACE_SIZE]
    ranges = [(0, 3), (2, 11), (5, 6), (9, 16)]
    with ctx.open_square(ods) as sq:
        raw = sq.share_proofs_raw(ranges)
    ns = ods[0, :NAMESPACE_SIZE].tobytes()
    descs = _descs_for(raw, ranges, k, ns)
    nrows, nleaves = len(raw["rows"]), len(raw["shares"])
    roots = np.frombuffer(raw["data_root"], np.uint8).reshape(1, 32)

    def run(descs, rows=raw["rows"]):
        return ctx.share_proofs_validate(descs, rows, raw["row_roots"], raw["leaf_hashes"], raw["nodes"], raw["aunts"],
                                         raw["shares"], roots).tolist()
    assert run(descs) == [0, 0, 0, 0]
    for field, value in (("row_off", nrows), ("row_off", 0xFFFFFFFF), ("nshare_proofs", nrows + 1),
                         ("nrow_roots", 0xFFFFFFFF), ("nrow_proofs", nrows + 1), ("leaf_off", nleaves),
                         ("leaf_off", 0xFFFFFFF0), ("nleaves", nleaves + 1), ("data_root", 1),
                         ("data_root", 0xFFFFFFFF)):
        d = descs.copy()
        d[2][field] = value
        assert run(d) == [0, 0, N.SP_MALFORMED, 0], (field, value)
    d = descs.copy()
    d[2]["row_off"] = d[1]["row_off"] + 1  # inside proof 1's records
    assert run(d) == [0, N.SP_MALFORMED, N.SP_MALFORMED, 0]
    for field, leg in (("node_off", N.SP_SHARE_PROOF), ("nnodes", N.SP_SHARE_PROOF), ("aunt_off", N.SP_ROW_PROOF),
                       ("naunts", N.SP_ROW_PROOF)):
        rows = raw["rows"].copy()
        rows[int(descs[1]["row_off"])][field] = 0xFFFFFFF0
        assert run(descs, rows) == [0, leg, 0, 0], field
    assert ctx._L.cda_share_proofs_validate(ctx._h, 1, None, None, None, None, 0, None, 0, None, 0, None, 0, None, 0,
                                            None) == N.E_ARG
    # misaligned device pointers are refused before any launch
    assert ctx._L.cda_share_proofs_validate_device(ctx._h, 1, 4096, 4096, 4096, 4096, 1, 4096, 1, 4096, 1, 4097, 1,
                                                   4096, 1, 4096, None) == N.E_ARG
    assert ctx._L.cda_share_proofs_validate_device(ctx._h, 1, 4096, 4100, 4096, 4096, 1, 4096, 1, 4096, 1, 4096, 1,
                                                   4096, 1, 4096, None) == N.E_ARG


def test_prove_validate_round_trip_on_device(ctx):
    """Proofs go from cda_square_share_proofs to cda_share_proofs_validate_device in device memory as they lie: only
    the per-proof descriptors are made on the host (from the ranges alone).  All valid; one byte flipped on the device
    in a share of one proof, in a row root of another and in an aunt of a third: exactly those fail, each at its
    leg."""
    import torch
    dev = torch.device("cuda", 0)
    k = 8
    ods = O.gen_ods(k, 0x5F07)
    ods[:, :NAMESPACE_SIZE] = ods[0, :NAMESPACE_SIZE]
    ranges = [(s, e) for s in range(0, k * k, 5) for e in (s + 1, min(k * k, s + 11), k * k)]
    with ctx.open_square(ods) as sq:
        d = _device_outputs(sq, ranges, dev)
        host = sq.share_proofs_raw(ranges)
    _assert_device_equals_host(d, host)
    row_off = [0]
    for s, e in ranges:
        row_off.append(row_off[-1] + (e - 1) // k - s // k + 1)
    descs = _descs_for({"row_off": np.array(row_off)}, ranges, k, ods[0, :NAMESPACE_SIZE].tobytes())
    nrows, nshares = row_off[-1], sum(e - s for s, e in ranges)
    d_descs = torch.from_numpy(descs.view(np.uint8).reshape(-1).copy()).to(dev)
    d_verdicts = torch.full((len(ranges),), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()

    def validate():
        ctx.share_proofs_validate_device(len(ranges), d_descs.data_ptr(), d["rows"].data_ptr(),
                                         d["row_roots"].data_ptr(), d["leaf_hashes"].data_ptr(), nrows,
                                         d["nodes"].data_ptr(), nrows * d["nodes"].shape[1], d["aunts"].data_ptr(),
                                         nrows * d["aunts"].shape[1], d["shares"].data_ptr(), nshares,
                                         d["data_root"].data_ptr(), 1, d_verdicts.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        return d_verdicts.cpu().numpy().tolist()
    assert validate() == [0] * len(ranges)
    share_of = np.cumsum([0] + [e - s for s, e in ranges])
    d["shares"][int(share_of[4]), 100] ^= 1
    d["row_roots"][row_off[9], 70] ^= 1
    d["aunts"][row_off[13], 2, 5] ^= 1
    torch.cuda.synchronize()
    want = [0] * len(ranges)
    want[4], want[9], want[13] = N.SP_SHARE_PROOF, N.SP_ROW_PROOF, N.SP_ROW_PROOF
    assert validate() == want
