"""GPU tests of a square rebuilt from proved samples: cda_samples_assemble_device and cda_square_rebuild
against the rule's Python mirror cda.sampling.assemble_host and the oracle's Repair, byte for byte;
cda_square_open_eds_device against cda_square_open_eds; argument checks; one run at the workload's size."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib as O
from cda import _native as N
from cda import befp, sampling
from cda import proof as P
from cda.proof import NMTProof
from cda.sampling import CONFLICT, DUPLICATE, MALFORMED, PLACED, REJECTED
from test_rebuild import OracleSquare, cell_of, flipped, two_tree_square

pytestmark = pytest.mark.gpu


# ---- rule parity ----
def mixed_samples(sq, n):
    """n samples of the two-tree square `sq` (cell (k - 1, k) contested) that meet every line of the rule early, then
    every cell by both axes for as long as n lasts (again from the start when n is larger).  -> (samples, beyond): the
    index of the sample whose descriptor the device form gets with node_off + nnodes beyond the total (the mirror sees
    a proof that is a node short instead: REJECTED either way), or None when n is too small to hold it."""
    k, w = sq.k, sq.w
    border = [(r, c) for r in (k - 1, k) for c in (k - 1, k)]
    a, i, j, share, proof = sq.sample(0, w - 1, 0)
    head = [sq.sample(0, k - 1, k),                               # the contested cell by its row ...
            (a, i, j, flipped(share), proof),                     # a corrupted share
            (a, (i + 1) % w, j, share, proof),                    # under the wrong root
            (a, i, j, share, NMTProof(j, j + 1, proof.nodes[:-1])),  # `beyond`
            (2, i, j, share, proof), (a, w, j, share, proof), (a, i, w, share, proof),
            sq.sample(1, k, k - 1),                               # ... and by its column: CONFLICT
            sq.sample(0, w - 1, w - 1), sq.sample(1, w - 1, w - 1),  # a duplicate pair, row first
            sq.sample(1, 0, w - 1), sq.sample(0, w - 1, 0)]          # and column first (cell (w - 1, 0))
    head += [sq.sample(axis, *((c, r) if axis else (r, c))) for r, c in border for axis in (0, 1)]
    head += [sq.sample(0, w - 1, c) for c in range(w)] + [sq.sample(1, w - 1, r) for r in range(w)]
    every = sq.every_cell_twice()
    if n == len(every):  # "every cell on both axes": exactly that, shuffled
        order = np.random.default_rng(n).permutation(n)
        return [every[t] for t in order], None
    samples = (head + every * (1 + n // len(every)))[:n]
    return samples, (3 if n > 3 else None)


def device_arrays(samples, beyond):
    descs, shares, nodes = sampling.pack_sample_descs(samples)
    if beyond is not None:
        descs["node_off"][beyond], descs["nnodes"][beyond] = 0xFFFFFFF0, 32  # the sum wraps in 32 bits, not in 64
    return descs, shares, nodes


@functools.lru_cache(maxsize=None)
def parity_square(k):
    return two_tree_square(k, 0x22C0 + k, k - 1, k)


@pytest.mark.parametrize("k", [1, 2, 4, 16])
def test_rule_parity(ctx, k):
    """Statuses, presence map and square of the device form (four streams) equal assemble_host's byte for byte; the
    host form's statuses too, and its square and presence map are the oracle's Repair of assemble_host's."""
    import torch
    dev = torch.device("cuda", 0)
    sq = parity_square(k)
    w, cells = 2 * k, 4 * k * k
    roots = np.concatenate([sq.row_roots, sq.col_roots])
    d_roots = torch.from_numpy(roots.reshape(-1)).to(dev)
    streams = [torch.cuda.Stream(dev) for _ in range(4)]
    runs = []
    torch.cuda.synchronize()
    for t, n in enumerate((1, 31, 33, 65, 8 * k * k)):
        samples, beyond = mixed_samples(sq, n)
        assert len(samples) == n
        descs, shares, nodes = device_arrays(samples, beyond)
        d = dict(descs=torch.from_numpy(descs.view(np.uint8).reshape(-1)).to(dev),
                 shares=torch.from_numpy(shares.reshape(-1)).to(dev), nodes=torch.from_numpy(nodes.reshape(-1).copy()).to(dev),
                 eds=torch.full((cells * N.SHARE_SIZE,), 0xEE, dtype=torch.uint8, device=dev),
                 present=torch.full((cells,), 7, dtype=torch.uint8, device=dev),
                 statuses=torch.full((n,), 9, dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()
        ctx.samples_assemble_device(k, n, d["descs"].data_ptr(), d["shares"].data_ptr(), d["nodes"].data_ptr(),
                                    len(nodes), d_roots.data_ptr(), d["eds"].data_ptr(), d["present"].data_ptr(),
                                    d["statuses"].data_ptr(), streams[t % 4].cuda_stream)
        runs.append((samples, descs, shares, nodes, d))
    torch.cuda.synchronize()
    seen = set()
    for samples, descs, shares, nodes, d in runs:
        want_eds, want_present, want = sampling.assemble_host(samples, sq.row_roots, sq.col_roots)
        n = len(samples)
        seen |= set(want.tolist())
        assert d["statuses"].cpu().numpy().tolist() == want.tolist(), (k, n)
        assert np.array_equal(d["present"].cpu().numpy(), want_present), (k, n)
        assert np.array_equal(d["eds"].cpu().numpy().reshape(cells, N.SHARE_SIZE), want_eds), (k, n)
        # the host form: the same statuses, then rsmt2d's Repair of that square
        orc, o_eds, o_present, o_axis, o_index = O.repair(want_eds, want_present, sq.row_roots, sq.col_roots)
        rc, handle, statuses, present, eds, err = ctx.rebuild_square_status(descs, shares, nodes, sq.row_roots,
                                                                            sq.col_roots, want_eds=True)
        assert statuses.tolist() == want.tolist(), (k, n)
        assert rc == orc and handle is None and rc in (N.E_UNREPAIRABLE, N.E_BYZANTINE), (k, n, rc, orc)
        if rc == N.E_BYZANTINE:
            assert (err.axis, err.index) == (o_axis, o_index), (k, n)
        assert np.array_equal(present, o_present), (k, n)
        assert np.array_equal(eds[o_present == 1], o_eds[o_present == 1]), (k, n)
        if rc == N.E_UNREPAIRABLE:  # every decode that ran was accepted: what is not present was never written
            assert not eds[o_present == 0].any(), (k, n)
            if np.array_equal(o_present, want_present):  # Repair decoded nothing: the assembled square itself
                assert np.array_equal(eds, want_eds)
    if k > 1:
        assert seen == {PLACED, DUPLICATE, CONFLICT, REJECTED, MALFORMED}
    # nothing present is legal
    none = np.zeros(0, N.SAMPLE_DESC_DTYPE)
    rc, handle, statuses, present, eds, err = ctx.rebuild_square_status(none, np.zeros((0, 512), np.uint8),
                                                                        np.zeros((0, 90), np.uint8), sq.row_roots,
                                                                        sq.col_roots, want_eds=True)
    assert rc == N.E_UNREPAIRABLE and handle is None and not present.any() and not eds.any()


# ---- rebuild parity with the oracle ----
MASKS = [(0.6, 1), (0.6, 2), (0.5, 3), (0.25, 4), (0.2, 5), "q0"]
MASK_OK = [True, True, True, False, False, True]


@functools.lru_cache(maxsize=None)
def header(k):
    """An honest block as its producer sees it: (ods, eds, row_roots, col_roots, dah) by the oracle."""
    ods = O.gen_ods(k, 0x22D0 + k)
    rc, eds, rr, cr, dah = O.extend_commit(ods)
    assert rc == 0
    return ods, eds, rr, cr, bytes(dah)


def kept_cells(k, mask):
    w = 2 * k
    if mask == "q0":
        keep = np.zeros((w, w), bool)
        keep[:k, :k] = True
        return keep.reshape(-1)
    frac, seed = mask
    return np.random.default_rng(1000 * k + seed).random(w * w) < frac


def samples_by_random_axis(square, cells, w, rng, both=()):
    """Each cell by its row or its column proof, at random (cells of `both` by both), in a random order."""
    coords = [(int(c) // w, int(c) % w) for c in cells]
    by_col = rng.random(len(coords)) < 0.5
    rows = [rc for rc, col in zip(coords, by_col) if not col or rc in both]
    cols = [rc for rc, col in zip(coords, by_col) if col or rc in both]
    samples = (sampling.sample_proofs(square, rows, 0) if rows else []) + \
        (sampling.sample_proofs(square, cols, 1) if cols else [])
    return [samples[t] for t in rng.permutation(len(samples))]


def with_extras(samples, rng):
    """10 % more (one at the least): corrupted copies and plain copies in turn, put in at random places."""
    out = list(samples)
    assert out, "no cell kept: the case checks nothing"
    for e, t in enumerate(rng.choice(len(samples), max(1, len(samples) // 10), replace=False)):
        a, i, j, share, proof = samples[t]
        extra = samples[t] if e % 2 else (a, i, j, flipped(share, int(rng.integers(0, 512))), proof)
        out.insert(int(rng.integers(0, len(out) + 1)), extra)
    return out


@pytest.mark.parametrize("mask", range(len(MASKS)), ids=[str(m) for m in MASKS])
@pytest.mark.parametrize("k", [2, 4, 8, 16])
def test_rebuild_matches_the_oracle(ctx, k, mask):
    ods, eds, rr, cr, dah = header(k)
    w = 2 * k
    keep = kept_cells(k, MASKS[mask])
    present0 = keep.astype(np.uint8)
    sparse = eds * present0[:, None]
    orc, o_eds, o_present, _, _ = O.repair(sparse, present0, rr, cr)
    assert orc == (0 if MASK_OK[mask] else N.E_UNREPAIRABLE), (k, MASKS[mask], orc)  # the case is what it says it is
    rng = np.random.default_rng(7000 * k + mask)
    with ctx.open_square(ods) as src:
        assert src.dah == dah
        samples = with_extras(samples_by_random_axis(src, np.flatnonzero(keep), w, rng), rng)
    if MASK_OK[mask]:
        sq, statuses, present, got = sampling.rebuild(ctx, samples, rr, cr, want_eds=True)
        with sq:
            assert np.array_equal(sq.row_roots, rr) and np.array_equal(sq.col_roots, cr) and sq.dah == dah
            assert np.array_equal(got, o_eds) and np.array_equal(got, eds) and present.all()
            cells = rng.choice(w * w, min(32, w * w), replace=False)
            for axis, index, pos, share, proof in samples_by_random_axis(sq, cells, w, rng):
                root = (cr if axis else rr)[index].tobytes()
                assert share == eds.reshape(w, w, 512)[(pos, index) if axis else (index, pos)].tobytes()
                assert proof.verify_inclusion(sampling.sample_namespace(k, axis, index, pos, share), [share], root)
            end = 2  # the shares from 1 on that share 1's namespace: a ShareProof is of one namespace
            while end < min(k * k, k + 2) and ods[end, :29].tobytes() == ods[1, :29].tobytes():
                end += 1
            sp, = sq.share_proofs([(1, end)])
            sp.validate(dah)
            assert P.validate_share_proofs(ctx, [sp], dah) == [None]
    else:
        with pytest.raises(N.CdaError) as e:
            sampling.rebuild(ctx, samples, rr, cr, want_eds=True)
        assert e.value.code == N.E_UNREPAIRABLE
        present, got, statuses = e.value.present, e.value.eds, e.value.statuses
        assert np.array_equal(present, o_present)
        assert np.array_equal(got[present == 1], o_eds[present == 1]) and not got[present == 0].any()
        rc, handle, _, _, _, _ = ctx.rebuild_square_status(*sampling.pack_sample_descs(samples), rr, cr)
        assert rc == N.E_UNREPAIRABLE and handle is None
    counts = np.bincount(statuses, minlength=5)
    assert counts[PLACED] == keep.sum() and counts[MALFORMED] == 0 and counts[CONFLICT] == 0
    assert counts[REJECTED] + counts[DUPLICATE] == len(samples) - keep.sum() and counts[REJECTED] > 0


def test_byzantine_square_and_its_fraud_proof(ctx):
    """k = 8, a Q1 cell altered before commitment; that cell and three more of its row are withheld, so rsmt2d decodes
    the row and finds it does not hash to its root.  The samples the node holds are the fraud proof."""
    k, w = 8, 16
    row, col = 3, 11
    bad = O.extend(O.gen_ods(k, 0x22E0))
    bad.reshape(w, w, 512)[row, col, 77] ^= 0x04
    keep = np.ones((w, w), bool)
    keep[row, [col, 0, 5, 14]] = False
    keep = keep.reshape(-1)
    rng = np.random.default_rng(0x22E1)
    with ctx.open_square_eds(bad) as src:
        rr, cr = src.row_roots.copy(), src.col_roots.copy()
        both = {(r, c) for r in range(w) for c in range(w) if r == row or c == col}
        samples = samples_by_random_axis(src, np.flatnonzero(keep), w, rng, both=both)
    present0 = keep.astype(np.uint8)
    orc, o_eds, o_present, o_axis, o_index = O.repair(bad * present0[:, None], present0, rr, cr)
    assert orc == N.E_BYZANTINE and (o_axis, o_index) == (0, row)
    with pytest.raises(N.CdaError) as e:
        sampling.rebuild(ctx, samples, rr, cr, want_eds=True)
    err = e.value
    assert (err.code, err.axis, err.index) == (N.E_BYZANTINE, o_axis, o_index)
    assert np.array_equal(err.present, o_present)
    assert np.array_equal(err.eds[o_present == 1], o_eds[o_present == 1])
    assert set(err.statuses.tolist()) == {PLACED, DUPLICATE}
    fraud = befp.from_samples(samples, err.axis, err.index, k)
    assert [p for p, _, _ in fraud.shares] == [c for c in range(w) if keep[row * w + c]]
    assert befp.validate(ctx, [fraud], [(rr, cr)]) == [befp.FRAUD]
    assert befp.validate(ctx, [befp.from_samples(samples, 1, col, k)], [(rr, cr)]) == [befp.FRAUD]


# ---- cda_square_open_eds_device, isolation, lifetime ----
def prove_every_cell(sq):
    w = 2 * sq.k
    return sq.prove([(axis, i, j, j + 1) for axis in (0, 1) for i in range(w) for j in range(w)])


@pytest.mark.parametrize("k", [4, 16])
def test_open_square_eds_device(ctx, k):
    import torch
    dev = torch.device("cuda", 0)
    ods, eds, rr, cr, dah = header(k)
    d_eds = torch.from_numpy(eds.reshape(-1)).to(dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with ctx.open_square_eds(eds) as a, ctx.open_square_eds_device(k, d_eds.data_ptr(), stream.cuda_stream) as b:
        d_eds.zero_()  # the handle has its own copy
        torch.cuda.synchronize()
        assert np.array_equal(b.row_roots, a.row_roots) and np.array_equal(b.col_roots, a.col_roots)
        assert np.array_equal(b.row_roots, rr) and np.array_equal(b.col_roots, cr) and a.dah == b.dah == dah
        for x, y in zip(prove_every_cell(a), prove_every_cell(b)):
            assert np.array_equal(x, y)


def test_rebuilt_square_isolation_and_lifetime():
    """A rebuilt square is untouched by later work on its context (another rebuild among it), and cda_free of the
    context leaves its handle good for close alone."""
    import cda
    c = cda.Context(0)
    k, w = 4, 8
    ods, eds, rr, cr, dah = header(k)
    rng = np.random.default_rng(0x22F0)
    with c.open_square(ods) as src:
        samples = samples_by_random_axis(src, np.flatnonzero(kept_cells(k, (0.6, 1))), w, rng)
    sq, _, _ = sampling.rebuild(c, samples, rr, cr)
    before = prove_every_cell(sq)
    ods2, eds2, rr2, cr2, dah2 = header(16)
    assert np.array_equal(c.extend_commit(ods2)[0], eds2)
    ns, blob = bytes(19) + bytes(range(10)), bytes(range(256)) * 40
    assert c.blob_commitments([ns], [blob])[0] == O.blob_commitment(ns, blob)[1]
    with c.open_square(ods2) as src2:
        s2 = samples_by_random_axis(src2, np.flatnonzero(kept_cells(16, (0.6, 2))), 32, rng)
    with sampling.rebuild(c, s2, rr2, cr2)[0] as other:
        assert other.dah == dah2
        after = prove_every_cell(sq)
    with pytest.raises(N.CdaError):
        sampling.rebuild(c, s2[:100], rr2, cr2)
    again = prove_every_cell(sq)
    for x, y, z in zip(before, after, again):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert np.array_equal(before[2][:w * w], eds)
    c.close()
    counts, nodes = np.zeros(1, np.int32), np.zeros((1, 6, N.NODE_SIZE), np.uint8)
    q = np.array([(0, 0, 0, 1)], N.RANGE_QUERY_DTYPE)
    assert sq._ctx._L.cda_square_prove(sq._h, 1, N._p(q), 6, N._p(counts), N._p(nodes), None, 0) == N.E_ARG
    sq.close()


# ---- argument checks ----
def test_argument_checks_leak_nothing(ctx):
    import torch
    dev = torch.device("cuda", 0)
    k, w = 16, 32  # a handle of this size is a third of an allocation granule: eight leaked ones show
    ods, eds, rr, cr, dah = header(k)
    with ctx.open_square(ods) as src:
        samples = sampling.sample_proofs(src, [(r, c) for r in range(w) for c in range(w)], 0)
    descs, shares, nodes = sampling.pack_sample_descs(samples)
    n, nn = len(descs), len(nodes)
    L, V = ctx._L, ctypes.c_void_p
    statuses, present, out_dah = np.zeros(n, np.uint8), np.zeros(w * w, np.uint8), np.zeros(32, np.uint8)
    err = N.ErrInfo()

    def rebuild(k=k, n=n, descs=descs, shares=shares, nodes=nodes, rr=rr, cr=cr, out=True, statuses=statuses,
                dah=out_dah):
        h = V()
        rc = L.cda_square_rebuild(ctx._h, k, n, N._p(descs), N._p(shares), N._p(nodes), nn, N._p(rr), N._p(cr),
                                  ctypes.byref(h) if out else None, N._p(statuses), N._p(present), None, N._p(dah),
                                  ctypes.byref(err))
        assert rc != N.OK and h.value is None
        return rc
    d = dict(descs=torch.from_numpy(descs.view(np.uint8).reshape(-1)).to(dev),
             shares=torch.zeros(n * 512 + 16, dtype=torch.uint8, device=dev),
             nodes=torch.from_numpy(nodes.reshape(-1).copy()).to(dev),
             roots=torch.from_numpy(np.concatenate([rr, cr]).reshape(-1)).to(dev),
             eds=torch.zeros(w * w * 512 + 16, dtype=torch.uint8, device=dev),
             present=torch.zeros(w * w, dtype=torch.uint8, device=dev),
             statuses=torch.zeros(n, dtype=torch.uint8, device=dev))
    ptr = {name: t.data_ptr() for name, t in d.items()}

    def assemble(k=k, **moved):
        p = dict(ptr, **moved)
        return L.cda_samples_assemble_device(ctx._h, k, n, V(p["descs"]), V(p["shares"]), V(p["nodes"]), nn,
                                             V(p["roots"]), V(p["eds"]), V(p["present"]), V(p["statuses"]), None)

    def open_device(k=k, d_eds=ptr["eds"], out=True):
        h = V()
        rc = L.cda_square_open_eds_device(ctx._h, k, V(d_eds), ctypes.byref(h) if out else None, N._p(rr), N._p(cr),
                                          N._p(out_dah), ctypes.byref(err), None)
        assert rc != N.OK and h.value is None
        return rc
    assert rebuild(n=10) == N.E_UNREPAIRABLE  # the context's workspace has its size from here on
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    for kw in (dict(out=False), dict(descs=None), dict(shares=None), dict(nodes=None), dict(rr=None), dict(cr=None),
               dict(statuses=None), dict(dah=None)):
        assert rebuild(**kw) == N.E_ARG, kw
    assert rebuild(k=3) == N.E_NOT_POW2 and rebuild(k=1024) == N.E_UNSUPPORTED
    for name in ptr:
        assert assemble(**{name: 0}) == N.E_ARG, name
        assert assemble(**{name: ptr[name] + (8 if name in ("shares", "eds") else 2)}) == N.E_ARG, name
    assert assemble(k=3) == N.E_NOT_POW2 and assemble(k=1024) == N.E_UNSUPPORTED
    assert open_device(d_eds=0) == N.E_ARG and open_device(out=False) == N.E_ARG
    assert open_device(d_eds=ptr["eds"] + 8) == N.E_ARG
    assert open_device(k=3) == N.E_NOT_POW2 and open_device(k=1024) == N.E_UNSUPPORTED
    # a failed repair releases the handle's memory too
    for _ in range(8):
        assert rebuild(n=10) == N.E_UNREPAIRABLE
    torch.cuda.synchronize()
    assert abs(torch.cuda.mem_get_info(dev)[0] - free0) <= 2 << 20  # one allocation granule


# ---- the workload's size ----
def test_device_chain_k128(ctx):
    """k = 128 without the square leaving the GPU: all 65,536 cells proved on the row axis into device memory, a
    fixed-seed half of them assembled, repaired and retained there; the roots and the data root are the source's."""
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
    with ctx.open_square(ods) as src:
        src.prove_device(q, mn, d_counts.data_ptr(), d_nodes.data_ptr(), d_shares.data_ptr(), d_shares.numel())
        rr, cr, dah = src.row_roots.copy(), src.col_roots.copy(), src.dah
    assert (d_counts.cpu().numpy() == 8).all()
    pick = np.flatnonzero(np.random.default_rng(128).random(nq) < 0.5)
    n = len(pick)
    descs = np.zeros(n, N.SAMPLE_DESC_DTYPE)
    descs["index"], descs["pos"] = q["index"][pick], q["start"][pick]
    descs["node_off"], descs["nnodes"] = pick.astype(np.uint32) * mn, 8
    d_descs = torch.from_numpy(descs.view(np.uint8).reshape(-1)).to(dev)
    d_picked = d_shares[torch.from_numpy(pick.astype(np.int64)).to(dev)].contiguous()
    d_roots = torch.from_numpy(np.concatenate([rr, cr]).reshape(-1)).to(dev)
    d_eds = torch.empty(nq * N.SHARE_SIZE, dtype=torch.uint8, device=dev)
    d_present = torch.empty(nq, dtype=torch.uint8, device=dev)
    d_statuses = torch.empty(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    ctx.samples_assemble_device(k, n, d_descs.data_ptr(), d_picked.data_ptr(), d_nodes.data_ptr(), nq * mn,
                                d_roots.data_ptr(), d_eds.data_ptr(), d_present.data_ptr(), d_statuses.data_ptr(),
                                stream.cuda_stream)
    stream.synchronize()
    present = d_present.cpu().numpy()
    assert (d_statuses.cpu().numpy() == PLACED).all() and np.array_equal(np.flatnonzero(present), pick)
    rc, present, err = ctx.repair_device(k, d_eds.data_ptr(), present, rr, cr, stream.cuda_stream)
    assert rc == N.OK and present.all()
    with ctx.open_square_eds_device(k, d_eds.data_ptr(), stream.cuda_stream) as sq:
        assert np.array_equal(sq.row_roots, rr) and np.array_equal(sq.col_roots, cr) and sq.dah == dah
