"""GPU tests of the bad-encoding fraud proofs: cda_square_open_eds retains a square as it was committed (honest or not)
and proves its cells as cda_square_open's handle does; cda_befp_validate / _device give cda.befp.validate_host's
verdicts (tests/test_befp.py holds the rule's CPU side) on mixed batches, on mainnet block 408, at
the widest GF(2^8) and the smallest GF(2^16) axis, and on what cda_repair reports as CDA_E_BYZANTINE."""
import numpy as np
import pytest

import oracle_lib as O
from cda import CdaError
from cda import _native as N
from cda import befp
from cda.befp import BAD_SHARE, FRAUD, MALFORMED, NO_FRAUD, TOO_FEW, BadEncodingProof
from test_befp import CODECS, HostSquare, corrupted, honest_eds
from test_inclusion import mainnet_ods

pytestmark = pytest.mark.gpu
LEO = CODECS["leopard"]


def all_cells(k):
    w = 2 * k
    return np.array([(a, i, p, p + 1) for a in (0, 1) for i in range(w) for p in range(w)], N.RANGE_QUERY_DTYPE)


def same_proofs(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("k", [1, 2, 4, 16])
def test_open_eds_honest(ctx, k):
    """An honest EDS retained as given commits to what extending its ODS commits to, and the handle serves the three
    kinds of proof exactly as cda_square_open's does."""
    ods = O.gen_ods(k, 0xED50 + k)
    rc, eds, rr, cr, dah = O.extend_commit(ods)
    assert rc == 0
    with ctx.open_square_eds(eds) as sq:
        assert sq.k == k and sq.dah == dah
        assert np.array_equal(sq.row_roots, rr) and np.array_equal(sq.col_roots, cr)
        with ctx.open_square(ods) as ref:
            if k in (2, 4):
                assert same_proofs(sq.prove(all_cells(k)), ref.prove(all_cells(k)))
            ranges = [(0, 1), (0, k * k), (k * k - 1, k * k)]
            got, want = sq.share_proofs_raw(ranges), ref.share_proofs_raw(ranges)
            assert all(np.array_equal(got[f], want[f]) for f in got)
            nq = [(a, i, bytes(ods[0, :N.NAMESPACE_SIZE])) for a in (0, 1) for i in (0, 2 * k - 1)]
            assert same_proofs(sq.prove_namespace(nq), ref.prove_namespace(nq))


def test_open_eds_commits_to_a_bad_square(ctx):
    """The encoding is not checked: the roots are those over the square as given, and every cell is proved against
    them, which is what a fraud proof has to carry."""
    k, w = 4, 8
    bad = corrupted(honest_eds(k, 0xED60), k, k + 1, k + 2, 9)
    rc, rr, cr, _, _ = O.roots(bad)
    assert rc == 0
    host = HostSquare(bad, k)
    with ctx.open_square_eds(bad) as sq:
        assert np.array_equal(sq.row_roots, rr) and np.array_equal(sq.col_roots, cr)
        assert sq.dah == O.dah_hash(rr, cr)
        q = all_cells(k)
        counts, nodes, cells = sq.prove(q)
        for i, (a, idx, p, _) in enumerate(q.tolist()):
            want = host.prove(a, idx, p)
            assert [nodes[i, j].tobytes() for j in range(counts[i])] == want.nodes
            assert cells[i].tobytes() == host.cell(a, idx, p)


def two_squares(k, seed):
    """Two blocks of a batch: an honest square, and one with a bad Q1 cell (0, k) and a bad Q3 cell (2k-1, 2k-1), as
    host squares (the mirror's trees) with their roots.  The Q1 cell is bad in byte 0: the code works byte by byte, so
    a cell of row 0 rebuilt through it is wrong in byte 0, the first of its namespace."""
    eds = honest_eds(k, seed)
    w = 2 * k
    bad = corrupted(corrupted(eds, k, 0, k, 0), k, w - 1, w - 1, 41)
    return HostSquare(eds, k), HostSquare(bad, k)


def mixed_batch(k):
    """Proofs of every verdict kind, rejected ones between valid ones, over two blocks."""
    w = 2 * k
    good, bad = two_squares(k, 0xED70 + k)
    rng = np.random.default_rng(k)

    def some(n, avoid=None):
        pool = [p for p in range(w) if p != avoid]
        return sorted(int(x) for x in rng.choice(pool, n, replace=False))

    def on(block, p):
        p.block = block
        return p
    sh = good.create(0, 0).shares
    flipped = (sh[-1][0], sh[-1][1][:100] + bytes([sh[-1][1][100] ^ 4]) + sh[-1][1][101:], sh[-1][2])
    proofs = [
        on(0, good.create(0, 0)),                                          # NO_FRAUD, all 2k
        on(0, BadEncodingProof(2, 0, list(sh))),                           # MALFORMED: axis
        on(1, bad.create(0, w - 1)),                                       # FRAUD: all 2k present, a bad parity cell
        on(0, BadEncodingProof(0, 0, list(sh[:k - 1]))),                   # TOO_FEW
        on(1, bad.create(1, w - 1, some(k, avoid=w - 1))),                 # FRAUD: the bad cell left out
        on(0, BadEncodingProof(0, 0, list(sh[:-1]) + [flipped])),          # BAD_SHARE
        on(0, good.create(1, 1 % w, some(min(k + 1, w)))),                 # NO_FRAUD, k + 1 shares
        on(1, bad.create(0, 1 % w if k > 1 else 0, some(k))),              # a neighbouring row (k = 1: row 0 again)
        on(0, BadEncodingProof(1, w, list(good.create(1, 0).shares))),     # MALFORMED: index
        on(1, bad.create(1, k, range(k, w))),                              # FRAUD: column k through the bad Q1 cell
        on(2, good.create(0, 0)),                                          # MALFORMED: roots outside the total
        on(1, bad.create(0, w - 1, range(k))),                             # FRAUD from the Q0-side half alone
        on(0, BadEncodingProof(0, 0, list(sh[:1]) + list(sh[:1]) + list(sh[2:]))),  # MALFORMED: a position twice
        on(0, good.create(1, w - 1, some(k))),                             # NO_FRAUD, k shares
    ]
    if k > 1:
        # row 0 through the bad Q1 cell from cells 1 .. k: cell 0 is rebuilt from inconsistent shares, the first byte
        # of its namespace is no longer 0 and breaks the push order (under the Lagrange decoder too)
        proofs.insert(3, on(1, bad.create(0, 0, range(1, k + 1))))
    return good, bad, proofs


def host_verdict(p, squares, codec=LEO, reason=None):
    if p.block >= len(squares):
        return MALFORMED
    return befp.validate_host(p, *squares[p.block].roots, codec=codec, reason=reason)


@pytest.mark.parametrize("k", [1, 2, 4, 16])
def test_mixed_batch(ctx, k):
    """One call over proofs of every verdict kind and two blocks, with raw descriptors that point outside the totals:
    the verdicts are validate_host's, and the device form on torch tensors on a stream of its own gives the same
    bytes."""
    import torch
    good, bad, proofs = mixed_batch(k)
    squares = [good, bad]
    want = [host_verdict(p, squares) for p in proofs]
    assert {FRAUD, NO_FRAUD, MALFORMED, TOO_FEW, BAD_SHARE} == set(want)
    if k > 1:
        why = []
        assert host_verdict(proofs[3], squares, CODECS["lagrange"], why) == FRAUD and why == ["order"]
    roots = befp.pack_roots([s.roots for s in squares])
    assert befp.validate(ctx, proofs, [s.roots for s in squares]) == want
    # the same arrays with descriptors outside the totals appended: entries, entry count, roots
    descs, entries, shares, nodes = befp.pack(proofs, k)
    ne, M = len(entries), 0xFFFFFFFF
    extra = np.array([(0, 0, ne, 1, 0), (0, 0, ne - k + 1, k, 0), (0, 0, M, 2, 0), (0, 0, 0, M, 0),
                      (0, 0, 0, 2 * k, len(roots) - 4 * k + 1), (1, 0, 0, 2 * k, M)], N.BEFP_DESC_DTYPE)
    descs = np.concatenate([descs, extra, descs[:1]])
    want = want + [MALFORMED] * len(extra) + want[:1]
    assert ctx.befp_validate(k, descs, entries, shares, nodes, roots).tolist() == want
    dev = torch.device("cuda", 0)
    up = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
          for a in (descs, entries, shares, nodes, roots)]
    d_ver = torch.full((len(descs),), 77, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    ctx.befp_validate_device(k, len(descs), up[0].data_ptr(), up[1].data_ptr(), ne, up[2].data_ptr(),
                             up[3].data_ptr() if len(nodes) else 0, len(nodes), up[4].data_ptr(), len(roots),
                             d_ver.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert d_ver.cpu().numpy().tolist() == want


def test_argument_checks(ctx):
    k = 4
    good = HostSquare(honest_eds(k, 0xED80), k)
    descs, entries, shares, nodes = befp.pack([good.create(0, 0)], k)
    roots = befp.pack_roots([good.roots])
    assert len(ctx.befp_validate(k, descs[:0], entries, shares, nodes, roots)) == 0
    for bad_k, code in ((0, N.E_ARG), (3, N.E_ARG), (1024, N.E_UNSUPPORTED)):
        with pytest.raises(CdaError) as e:
            ctx.befp_validate(bad_k, descs, entries, shares, nodes, roots)
        assert e.value.code == code
    with pytest.raises(CdaError) as e:  # shares not 16-byte aligned
        ctx.befp_validate_device(k, 1, 256, 256, 8, 264, 256, 10, 256, 16, 256)
    assert e.value.code == N.E_ARG
    with pytest.raises(CdaError) as e:
        ctx.open_square_eds(np.zeros((4 * 9, 512), np.uint8))
    assert e.value.code == N.E_NOT_POW2


def test_mainnet_block_408(ctx):
    """k = 32: an axis is two 32-lane passes of the gather.  The block as committed is never fraud; with one Q3 cell
    corrupted both axes through it are, from k shares and from all 2k."""
    ods = mainnet_ods()
    k, w = 32, 64
    eds = O.extend(ods)
    r, c = 40, 57
    with ctx.open_square_eds(eds) as sq, ctx.open_square_eds(corrupted(eds, k, r, c, 300)) as bad:
        roots = [(sq.row_roots, sq.col_roots), (bad.row_roots, bad.col_roots)]
        assert np.array_equal(sq.row_roots, ctx.extend_commit(ods, want_eds=False)[1])
        half = list(range(5, 5 + k))
        proofs, want = [], []
        for axis, index in ((0, r), (1, c), (0, 3), (1, 3)):
            for pos in (None, half):
                proofs.append(befp.create(sq, axis, index, pos))
                want.append(NO_FRAUD)
                p = befp.create(bad, axis, index, pos)
                p.block = 1
                proofs.append(p)
                want.append(FRAUD if index in (r, c) else NO_FRAUD)
        assert befp.validate(ctx, proofs, roots) == want
        assert [befp.validate_host(p, *roots[p.block], codec=LEO) for p in proofs[:4]] == want[:4]


def big_pair(ctx, k, seed):
    """A k x k block extended on the device, with the Q2 cell (r, c) corrupted: (bad EDS, r, c)."""
    eds = ctx.extend_commit(O.gen_ods(k, seed))[0]
    r, c = k + 3, 5
    return corrupted(eds, k, r, c, 17), r, c


def test_k128_widest_gf8_axis(ctx):
    k = 128
    bad, r, c = big_pair(ctx, k, 0xED90)
    with ctx.open_square_eds(bad) as sq:
        roots = [(sq.row_roots, sq.col_roots)]
        proofs = [befp.create(sq, 0, r, range(k, 2 * k)), befp.create(sq, 0, r), befp.create(sq, 1, c, range(k)),
                  befp.create(sq, 0, r + 1, range(1, 2 * k, 2)), befp.create(sq, 1, c + 1)]
        assert [len(p.shares) for p in proofs] == [128, 256, 128, 128, 256]
        assert befp.validate(ctx, proofs, roots) == [FRAUD, FRAUD, FRAUD, NO_FRAUD, NO_FRAUD]


def test_k256_smallest_gf16_axis(ctx):
    k = 256
    bad, r, c = big_pair(ctx, k, 0xEDA0)
    with ctx.open_square_eds(bad) as sq:
        roots = [(sq.row_roots, sq.col_roots)]
        proofs = [befp.create(sq, 1, c, range(0, 2 * k, 2)), befp.create(sq, 1, c + 1, range(k, 2 * k))]
        assert [len(p.shares) for p in proofs] == [256, 256]
        want = [befp.validate_host(p, *roots[0], codec=LEO) for p in proofs]
        assert want == [FRAUD, NO_FRAUD]
        assert befp.validate(ctx, proofs, roots) == want


@pytest.mark.parametrize("k", [4, 32])
def test_repair_to_fraud_proof(ctx, k):
    """End to end: a proposer commits to a square with one bad parity cell; a node that holds 60 % of it runs Repair
    against the committed roots and is told which axis is Byzantine; the proof built for that axis from the cells the
    node saw is FRAUD on the device and on the host, and the same for the honest square is NO_FRAUD."""
    w, seed = 2 * k, 0
    eds = honest_eds(k, 0xE2E0 + k)
    r, c = k + 1, k + 2
    bad = corrupted(eds, k, r, c, 77)
    present = (np.random.default_rng(seed).random(w * w) >= 0.4).astype(np.uint8)
    with ctx.open_square_eds(bad) as sq, ctx.open_square_eds(eds) as honest:
        rc, _, _, ax, ix = O.repair(bad, present, sq.row_roots, sq.col_roots, fft=True)
        assert rc == O.E_BYZANTINE  # the seed's choice, made on the CPU
        with pytest.raises(CdaError) as e:
            ctx.repair(bad, present, sq.row_roots, sq.col_roots)
        assert e.value.code == N.E_BYZANTINE and (e.value.axis, e.value.index) == (ax, ix)
        assert (ax, ix) in ((0, r), (1, c))
        view = present.reshape(w, w)
        positions = np.flatnonzero(view[:, ix] if ax else view[ix]).tolist()
        assert len(positions) >= k
        roots = [(sq.row_roots, sq.col_roots), (honest.row_roots, honest.col_roots)]
        proof = befp.create(sq, ax, ix, positions)
        fine = befp.create(honest, ax, ix, positions)
        fine.block = 1
        assert befp.validate(ctx, [proof, fine], roots) == [FRAUD, NO_FRAUD]
        assert [befp.validate_host(p, *roots[p.block], codec=LEO) for p in (proof, fine)] == [FRAUD, NO_FRAUD]
