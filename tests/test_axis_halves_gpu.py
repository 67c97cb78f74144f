"""GPU tests of the row and column halves: cda_axis_halves_verify (both forms), cda_square_axis_halves,
cda_axis_halves_assemble_device and cda_square_rebuild_axes against the rule's Python mirrors cda.rows.verify_host and
assemble_host (the oracle's codec and tree) and the oracle's Repair, byte for byte."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib as O
from cda import _native as N
from cda import proof as P
from cda import rows, sampling
from cda.rows import BAD_ROOT, CONFLICT, DUPLICATE, MALFORMED, PLACED, AxisHalf
from test_axis_halves import (CODEC, block, conflict_pair, descending_half, every_half, flipped_half, half_of,
                              named_malformed)

pytestmark = pytest.mark.gpu
GUARD = 64


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def guarded(nbytes, fill):
    """A device buffer of nbytes behind and before 64 guard bytes: (whole tensor, address of the inside)."""
    import torch
    t = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=torch.device("cuda", 0))
    return t, t.data_ptr() + GUARD


def inside(t, fill):
    a = t.cpu().numpy()
    assert (a[:GUARD] == fill).all() and (a[-GUARD:] == fill).all(), "a guard byte was written"
    return a[GUARD:-GUARD]


def verify_device(ctx, k, descs, shares, roots, want_axes=True):
    """cda_axis_halves_verify_device on a stream of its own, statuses and axes between guard bytes."""
    import torch
    n = len(descs)
    d_descs, d_shares, d_roots = up(descs), up(shares), up(roots)
    d_st, p_st = guarded(n, 0x77)
    d_ax, p_ax = guarded(n * 2 * k * 512 if want_axes else 0, 0x99)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.axis_halves_verify_device(k, n, d_descs.data_ptr(), d_shares.data_ptr(), d_roots.data_ptr(), len(roots), p_st,
                                  p_ax if want_axes else 0, stream.cuda_stream)
    stream.synchronize()
    return inside(d_st, 0x77), inside(d_ax, 0x99).reshape(n, 2 * k, 512) if want_axes else None


@functools.lru_cache(maxsize=None)
def big_block(ctx, k):
    ods = O.gen_ods(k, 0x26B0 + k)
    eds, rr, cr, dah = ctx.extend_commit(ods)
    return ods, eds, rr, cr, dah


def check_verify(ctx, k, halves, rr, cr):
    want, want_axes = rows.verify_host(halves, rr, cr, CODEC)
    got, axes = rows.verify(ctx, halves, rr, cr, want_axes=True)
    assert got.tolist() == want.tolist()
    good = want == PLACED
    assert np.array_equal(axes[good], want_axes[good])
    assert rows.verify(ctx, halves, rr, cr).tolist() == want.tolist()  # axes_or_null left out
    descs, shares = rows.pack(halves, k)
    d_got, d_axes = verify_device(ctx, k, descs, shares, rows.pack_roots(rr, cr))
    assert d_got.tolist() == want.tolist() and np.array_equal(d_axes[good], want_axes[good])
    assert verify_device(ctx, k, descs, shares, rows.pack_roots(rr, cr), want_axes=False)[0].tolist() == want.tolist()
    return want


# ---- verify ----
@pytest.mark.parametrize("k", [1, 2, 4, 16, 32])
def test_verify_every_half_and_the_named_bad_ones(ctx, k):
    """Every half of every axis, both sides (k = 32: a subset), with the named bad halves among them: the neighbours
    keep their statuses."""
    _, eds, rr, cr, _ = block(k)
    w = 2 * k
    halves = every_half(eds, k)
    if k == 32:
        halves = halves[::5]
    assert {(h.axis, h.side) for h in halves} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    bad = list(named_malformed(eds, k).values()) + [flipped_half(halves[1]), flipped_half(halves[-1], k - 1, 511)]
    if k >= 4:
        bad.append(descending_half(eds, k))
    mixed = list(halves)
    for t, h in enumerate(bad):
        mixed.insert(1 + 2 * t, h)
    want = check_verify(ctx, k, mixed, rr, cr)
    assert np.bincount(want, minlength=5).tolist() == [len(halves), 0, 0, len(bad) - 4, 4]
    # a flipped root
    bad_rr = rr.copy()
    bad_rr[w - 1, 40] ^= 0x02
    want = check_verify(ctx, k, halves, bad_rr, cr)
    assert [h for h, s in zip(halves, want) if s == BAD_ROOT] == [h for h in halves if (h.axis, h.index) == (0, w - 1)]


@pytest.mark.parametrize("k,n", [(128, 16), (256, 4)])
def test_verify_widest_gf8_and_gf16(ctx, k, n):
    _, eds, rr, cr, _ = big_block(ctx, k)
    rng = np.random.default_rng(k)
    halves = [half_of(eds, k, t & 1, int(rng.integers(0, 2 * k)), (t >> 1) & 1) for t in range(n)]
    halves[2] = flipped_half(halves[2], k - 1, 300)
    want = check_verify(ctx, k, halves, rr, cr)
    assert want.tolist() == [PLACED, PLACED, BAD_ROOT] + [PLACED] * (n - 3)


def test_verify_two_blocks_in_one_call_and_nothing(ctx):
    k = 4
    a, b = block(k), block(k, seed=0x26C0)
    ha, hb = every_half(a[1], k)[::3], every_half(b[1], k)[1::3]
    da, sa = rows.pack(ha, k)
    db, sb = rows.pack(hb, k, root_off=4 * k)
    dx, sx = rows.pack(ha[:2], k, root_off=4 * k)       # under the other block's roots
    dm, sm = rows.pack(ha[:2], k, root_off=4 * k + 1)   # roots outside the total
    roots = np.concatenate([rows.pack_roots(a[2], a[3]), rows.pack_roots(b[2], b[3])])
    descs, shares = np.concatenate([da, db, dx, dm]), np.concatenate([sa, sb, sx, sm])
    want = [PLACED] * (len(ha) + len(hb)) + [BAD_ROOT] * 2 + [MALFORMED] * 2
    assert ctx.axis_halves_verify(k, descs, shares, roots).tolist() == want
    assert verify_device(ctx, k, descs, shares, roots)[0].tolist() == want
    wrap = np.array([(0, 0, 0, 0xFFFFFFFF), (0, 0, 0, 0xFFFFFFF0)], N.AXIS_HALF_DESC_DTYPE)  # the sum wraps in 32 bits
    assert ctx.axis_halves_verify(k, wrap, shares[:2], roots).tolist() == [MALFORMED] * 2
    assert len(ctx.axis_halves_verify(k, descs[:0], shares[:0], roots)) == 0
    ctx.axis_halves_verify_device(k, 0, 0, 0, 0, 0, 0)


# ---- serve ----
@pytest.mark.parametrize("k", [1, 2, 8])
def test_served_halves_are_the_squares_cells_and_verify(ctx, k):
    import torch
    ods, eds, rr, cr, dah = block(k)
    w = 2 * k
    queries = [(axis, index, side) for axis in (0, 1) for index in range(w) for side in (0, 1)]
    want = np.stack([half_of(eds, k, *q).shares for q in queries])
    for sq in (ctx.open_square(ods), ctx.open_square_eds(eds)):
        with sq:
            got = sq.axis_halves(queries)
            assert np.array_equal(got, want)
            d_out, p_out = guarded(want.nbytes, 0x55)
            sq.axis_halves(queries, d_shares=p_out, shares_cap=want.nbytes)
            torch.cuda.synchronize()
            assert np.array_equal(inside(d_out, 0x55), want.reshape(-1))
            halves = rows.halves_of(sq, queries[::3])
            assert rows.verify(ctx, halves, sq.row_roots, sq.col_roots).tolist() == [PLACED] * len(halves)
            for bad in ((2, 0, 0), (0, w, 0), (1, 0, 2)):
                with pytest.raises(N.CdaError) as e:
                    sq.axis_halves([bad])
                assert e.value.code == N.E_ARG
            q = np.array([(0, 0, 0, 0)], N.AXIS_HALF_DESC_DTYPE)
            assert ctx._L.cda_square_axis_halves(sq._h, 1, N._p(q), N._p(got), k * 512 - 1) == N.E_ARG


# ---- assemble ----
def assemble_device(ctx, k, descs, shares, roots):
    """cda_axis_halves_assemble_device on a stream of its own over poisoned outputs: (eds, present, statuses)."""
    import torch
    dev = torch.device("cuda", 0)
    n, cells = len(descs), 4 * k * k
    d_eds = torch.full((cells * 512,), 0xEE, dtype=torch.uint8, device=dev)
    d_present = torch.full((cells,), 7, dtype=torch.uint8, device=dev)
    d_st, p_st = guarded(n, 0x77)
    d_descs, d_shares, d_roots = up(descs), up(shares), up(roots)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    ctx.axis_halves_assemble_device(k, n, d_descs.data_ptr() if n else 0, d_shares.data_ptr() if n else 0,
                                    d_roots.data_ptr(), d_eds.data_ptr(), d_present.data_ptr(), p_st,
                                    stream.cuda_stream)
    stream.synchronize()
    return d_eds.cpu().numpy().reshape(cells, 512), d_present.cpu().numpy(), inside(d_st, 0x77)


def check_assemble(ctx, k, halves, rr, cr):
    descs, shares = rows.pack(halves, k)
    got = assemble_device(ctx, k, descs, shares, rows.pack_roots(rr, cr))
    want = rows.assemble_host(halves, rr, cr, CODEC)
    assert got[2].tolist() == want[2].tolist()
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    return want


@pytest.mark.parametrize("k", [1, 2, 4, 16])
def test_assemble_every_status_and_the_shuffle(ctx, k):
    _, eds, rr, cr, _ = block(k)
    w = 2 * k
    rng = np.random.default_rng(k)
    halves = [half_of(eds, k, int(a), int(i), int(s)) for a, i, s in
              zip(rng.integers(0, 2, 3 * k + 2), rng.integers(0, w, 3 * k + 2), rng.integers(0, 2, 3 * k + 2))]
    halves += [half_of(eds, k, halves[0].axis, halves[0].index, 1 - halves[0].side), halves[1],
               flipped_half(halves[0]), AxisHalf(0, 0, 0, halves[0].shares, root_off=1)]
    halves += list(named_malformed(eds, k).values())
    base = check_assemble(ctx, k, halves, rr, cr)
    assert {PLACED, DUPLICATE, BAD_ROOT, MALFORMED} == set(base[2].tolist())
    assert base[2][-8:-4].tolist() == [DUPLICATE, DUPLICATE, BAD_ROOT, MALFORMED]
    order = np.random.default_rng(k + 100).permutation(len(halves))
    again = check_assemble(ctx, k, [halves[t] for t in order], rr, cr)
    assert np.array_equal(again[0], base[0]) and np.array_equal(again[1], base[1])
    assert sorted(again[2].tolist()) == sorted(base[2].tolist())
    none = check_assemble(ctx, k, [], rr, cr)
    assert not none[0].any() and not none[1].any()


@pytest.mark.parametrize("k", [1, 2, 8])
def test_assemble_conflict_in_both_orders_and_its_repair(ctx, k):
    row_a, col_b, rr, cr, eds_a, eds_b = conflict_pair(k)
    w = 2 * k
    extra = [half_of(eds_a, k, 0, i, i & 1) for i in range(1, k)]  # k rows of A in all
    for pair, first in (([row_a, col_b], eds_a), ([col_b, row_a], eds_b)):
        eds, present, statuses = check_assemble(ctx, k, pair + extra, rr, cr)
        assert statuses.tolist() == [PLACED, CONFLICT] + [PLACED] * (k - 1)
        assert np.array_equal(eds.reshape(w, w, 512)[0, 0], first.reshape(w, w, 512)[0, 0])
        # the chain returns whatever rsmt2d's Repair makes of the assembled state
        orc, o_eds, o_present, o_axis, o_index = O.repair(eds, present, rr, cr)
        descs, shares = rows.pack(pair + extra, k)
        rc, sq, st, got_present, got_eds, err = ctx.square_rebuild_axes(descs, shares, rr, cr, want_eds=True)
        assert rc == orc and st.tolist() == statuses.tolist()
        if rc == N.OK:
            sq.close()
        else:
            assert sq is None and np.array_equal(got_present, o_present)
            assert np.array_equal(got_eds[o_present == 1], o_eds[o_present == 1])
            if rc == N.E_BYZANTINE:
                assert (err.axis, err.index) == (o_axis, o_index)


# ---- rebuild ----
def check_rebuilt(ctx, k, halves, ods, eds, rr, cr, dah):
    w = 2 * k
    sq, statuses, present, got = rows.rebuild(ctx, halves, rr, cr, want_eds=True)
    with sq:
        assert np.array_equal(sq.row_roots, rr) and np.array_equal(sq.col_roots, cr) and sq.dah == dah
        assert np.array_equal(got, eds) and present.all()
        rng = np.random.default_rng(k)
        coords = [(int(c) // w, int(c) % w) for c in rng.choice(w * w, min(8, w * w), replace=False)]
        for axis in (0, 1):
            for a, index, pos, share, proof in sampling.sample_proofs(sq, coords, axis):
                assert share == eds.reshape(w, w, 512)[(pos, index) if axis else (index, pos)].tobytes()
                assert proof.verify_inclusion(sampling.sample_namespace(k, axis, index, pos, share), [share],
                                              (cr if axis else rr)[index].tobytes())
        end = 2  # the shares from 1 on that share 1's namespace: a ShareProof is of one namespace
        while end < min(k * k, k + 2) and ods[end, :29].tobytes() == ods[1, :29].tobytes():
            end += 1
        sp, = sq.share_proofs([(1, end)])
        sp.validate(dah)
        assert P.validate_share_proofs(ctx, [sp], dah) == [None]
    return statuses


@pytest.mark.parametrize("k", [2, 8, 32])
def test_rebuild_from_rows_columns_and_a_mix(ctx, k):
    ods, eds, rr, cr, dah = block(k)
    w = 2 * k
    rng = np.random.default_rng(0x26D0 + k)
    pick = lambda n: [int(i) for i in rng.permutation(w)[:n]]  # noqa: E731
    from_rows = [half_of(eds, k, 0, i, int(rng.integers(0, 2))) for i in pick(k)]
    from_cols = [half_of(eds, k, 1, i, int(rng.integers(0, 2))) for i in pick(k)]
    mix = from_rows + [half_of(eds, k, 1, i, 1) for i in pick(k // 2)] + [flipped_half(from_cols[0]), from_rows[0]]
    mix = [mix[t] for t in rng.permutation(len(mix))]
    for halves in (from_rows, from_cols, mix):
        statuses = check_rebuilt(ctx, k, halves, ods, eds, rr, cr, dah)
        assert statuses.tolist() == rows.assemble_host(halves, rr, cr, CODEC)[2].tolist()
    # fewer than k rows with fewer than k columns: every missing row has fewer than k cells
    few = [half_of(eds, k, 0, i, 0) for i in pick(k - 1)] + [half_of(eds, k, 1, i, 1) for i in pick(k - 1)]
    a_eds, a_present, a_statuses = rows.assemble_host(few, rr, cr, CODEC)
    orc, o_eds, o_present, _, _ = O.repair(a_eds, a_present, rr, cr)
    assert orc == N.E_UNREPAIRABLE
    with pytest.raises(N.CdaError) as e:
        rows.rebuild(ctx, few, rr, cr, want_eds=True)
    assert e.value.code == N.E_UNREPAIRABLE and e.value.statuses.tolist() == a_statuses.tolist()
    assert np.array_equal(e.value.present, o_present) and np.array_equal(e.value.eds, o_eds)
    h = ctypes.c_void_p(1)
    descs, shares = rows.pack(few, k)
    out = np.zeros(32, np.uint8)
    rc = ctx._L.cda_square_rebuild_axes(ctx._h, k, len(few), N._p(descs), N._p(shares), N._p(rr), N._p(cr),
                                        ctypes.byref(h), N._p(a_statuses.copy()), None, None, N._p(out), None)
    assert rc == N.E_UNREPAIRABLE and h.value is None


def test_rebuild_k128_from_the_ods_rows(ctx):
    k = 128
    ods, eds, rr, cr, dah = big_block(ctx, k)
    halves = [half_of(eds, k, 0, i, 0) for i in range(k)]
    statuses = check_rebuilt(ctx, k, halves, ods, eds, rr, cr, dah)
    assert statuses.tolist() == [PLACED] * k


def test_argument_checks_with_a_context(ctx):
    k = 4
    _, eds, rr, cr, _ = block(k)
    halves = every_half(eds, k)[:3]
    descs, shares = rows.pack(halves, k)
    roots = rows.pack_roots(rr, cr)
    L, V = ctx._L, ctypes.c_void_p
    st = np.zeros(3, np.uint8)
    args = [N._p(descs), N._p(shares), N._p(roots), 4 * k, N._p(st), None]
    for missing in (0, 1, 2, 4):
        a = list(args)
        a[missing] = None
        assert L.cda_axis_halves_verify(ctx._h, k, 3, *a) == N.E_ARG, missing
    assert L.cda_axis_halves_verify(ctx._h, 3, 3, *args) == N.E_NOT_POW2
    assert L.cda_axis_halves_verify(ctx._h, 1024, 3, *args) == N.E_UNSUPPORTED
    d = {"descs": up(descs), "shares": up(np.concatenate([shares.reshape(-1), np.zeros(16, np.uint8)])),
         "roots": up(roots)}
    d["statuses"], d["axes"] = up(np.zeros(16, np.uint8)), up(np.zeros(3 * 2 * k * 512 + 16, np.uint8))
    d["eds"], d["present"] = up(np.zeros(4 * k * k * 512 + 16, np.uint8)), up(np.zeros(4 * k * k, np.uint8))
    ptr = {name: t.data_ptr() for name, t in d.items()}

    def verify(**moved):
        p = dict(ptr, **moved)
        return L.cda_axis_halves_verify_device(ctx._h, k, 3, V(p["descs"]), V(p["shares"]), V(p["roots"]), 4 * k,
                                               V(p["statuses"]), V(p["axes"]), None)

    def assemble(**moved):
        p = dict(ptr, **moved)
        return L.cda_axis_halves_assemble_device(ctx._h, k, 3, V(p["descs"]), V(p["shares"]), V(p["roots"]),
                                                 V(p["eds"]), V(p["present"]), V(p["statuses"]), None)
    for name in ("descs", "shares", "roots", "statuses"):
        assert verify(**{name: 0}) == N.E_ARG and assemble(**{name: 0}) == N.E_ARG, name
    for name in ("eds", "present"):
        assert assemble(**{name: 0}) == N.E_ARG, name
    for name in ("descs", "shares", "roots", "axes"):
        assert verify(**{name: ptr[name] + (8 if name in ("shares", "axes") else 2)}) == N.E_ARG, name
    for name in ("descs", "shares", "roots", "eds", "present"):
        assert assemble(**{name: ptr[name] + (8 if name in ("shares", "eds") else 2)}) == N.E_ARG, name
    assert verify() == N.OK and assemble() == N.OK
    import torch
    torch.cuda.synchronize()
    assert d["statuses"].cpu().numpy()[:3].tolist() == [PLACED, DUPLICATE, PLACED]
