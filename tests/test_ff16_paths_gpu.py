"""GF(2^16) squares (k > 128) through cda_repair and the batched codec calls: the launches behind the block path
that only these shapes reach.  Everything is bit-exact against the CPU oracle (tests/oracle_lib.py).

A. cda_repair at k = 256 (w = 512; csrc/repair.cpp repair_impl).  The decoder is rs_decode_kernel<16> with n = 512
   (launch_rs_decode: U = 2 in a crossword batch, U = 1 for the one codeword of a sequential replay).
    1 q0_only         packed upload (scatter_cell_runs_kernel<false>, presence rows of 8 words); batch 1 = rows and
                      columns 0..k-1 interleaved, batch 2 completes the bottom half; launch_axes_verify on 512-leaf
                      trees with the atomicMin flag.
    2 q3_only         every data shard of every codeword erased: decode from parity alone.
    3 checkerboard    exactly k survivors per axis, alternating (runs one cell apart join across the gaps, so the
                      square goes up whole).
    4 sanity_passes   32 complete axes in both halves: launch_axes_verify per_tree on 512-leaf trees, both passes of
                      the sanity re-encode (launch_rs_encode16 from repair.cpp with cw_per_blk = 2k: the row-strided,
                      then the column-strided source, packed destination) and parity_compare_kernel at k = 256 -- no
                      flag may be raised.
    5 sanity_root     a flipped Q0 bit in complete row 100: the per_tree root flag of that tree, reported first.
    6 sanity_parity_row   the committed roots are those of a square with a bad Q1 cell, so row 5's root matches and
                      only parity_compare_kernel (row pass) can report it.
    7 sanity_parity_col   the same square with column k+9 complete instead: the column-strided re-encode and the
                      column half of the parity flags.
    8 byzantine_first_batch  a corrupted present cell in row 40: batch 1 (all 1024 axes) fails its root check and is
                      replayed one operation at a time (launch_rs_decode with one codeword, roots_of through
                      launch_axes_roots on 512 leaves) up to row 40.
    9 byzantine_later_batch  a committed bad Q3 cell, Q0 present: batch 1 passes, batch 2 is replayed up to row k+3.
   10 unrepairable    20 % presence after a call that left a whole other square on the device: packed upload, the
                      oracle's presence and cells, zeros or the caller's filler elsewhere.
   11 registered      case 1 in place in page-locked memory: scatter_cell_runs_kernel<true> reads the runs itself.
   12 repair_device   cases 8 and 10 on a torch allocation with a caller stream (cda_repair_device).
   Honest cases (1-4, 11) expect the oracle's own extension.  Every other input is first run through both oracle
   decoders (Lagrange and Leopard FFT), which must agree on rc, axis, index, presence and every present cell: a
   decode from an inconsistent codeword is algorithm-dependent and no reference for anything.

B. cda_repair at k = 512: the sanity check on ~1000 complete rows through rs_encode16_reg_kernel with total = 1024,
   1024-leaf verify trees (96 KiB of LDS), rs_decode_kernel<16> with n = 1024 (U = 1) inside a batch.

C. cda_rs_encode_device at GF(2^16), codewords contiguous and as columns of a k x ncw grid (how Repair's sanity
   check strides it): rs_encode16_kernel batched (launch_rs_encode16), and rs_encode16_reg_kernel
   (launch_rs_encode16_reg, k = 512) with fewer codewords than workgroups, with one workgroup that has a next
   codeword to prefetch while the others have none (body2's `more`), with a mixed launch, and with two 512-byte
   slices per codeword.

D. cda_rs_decode at GF(2^16) on structured loss (parity only, a contiguous window of k, even positions, the two
   ends), k in {129, 256, 300, 512}: for k below m = ceilPow2(k) the positions [k, m) are always erased."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

K = 256
W = 2 * K
FILL = 0xEE  # the caller's bytes in missing cells
ROW, COL = 0, 1


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def _grid(pres):
    return np.ascontiguousarray(pres, np.uint8).reshape(-1)


def _damaged(square, pres):
    """The caller's square: `square` where present, FILL elsewhere."""
    out = square.copy()
    out[np.flatnonzero(pres == 0)] = FILL
    return out


@pytest.fixture(scope="module")
def sq256():
    rc, eds, rr, cr, _ = O.extend_commit(O.gen_ods(K, 7))
    assert rc == 0
    return _frozen(eds, rr, cr)


def _commit_bad(eds, r, c, byte):
    """A square with one flipped byte in cell (r, c) and the roots that commit to it."""
    bad = eds.copy()
    bad[r * W + c, byte] ^= 0xFF
    rc, rr, cr, _, _ = O.roots(bad)
    assert rc == 0
    return _frozen(bad, rr, cr)


@pytest.fixture(scope="module")
def bad_q1(sq256):
    return _commit_bad(sq256[0], 5, K + 9, 77)


def _oracle_agreed(damaged, pres, rr, cr):
    """The sequential oracle's outcome, required to be the same with either of its decoders (no GPU involved)."""
    a = O.repair(damaged, pres, rr, cr, fft=False)
    b = O.repair(damaged, pres, rr, cr, fft=True)
    assert (a[0], a[3], a[4]) == (b[0], b[3], b[4]), "oracle decoders disagree: not a reference"
    assert np.array_equal(a[2], b[2])
    m = a[2].astype(bool)
    assert np.array_equal(a[1][m], b[1][m])
    return a


def _assert_exact(rc_g, eds_g, p_g, err, want):
    """As test_gpu_parity._check_repair_exact, against an oracle result computed beforehand."""
    rc_o, eds_o, p_o, ax_o, ix_o = want
    assert rc_g == rc_o, (rc_g, rc_o)
    if rc_o == O.E_BYZANTINE:
        assert (err.axis, err.index) == (ax_o, ix_o)
    assert np.array_equal(p_g, p_o)
    m = p_o.astype(bool)
    assert np.array_equal(eds_g[m], eds_o[m])
    return m


def _repair_exact(ctx, damaged, pres, rr, cr, outcome):
    want = _oracle_agreed(damaged, pres, rr, cr)
    assert (want[0], want[3], want[4]) == outcome  # the input reaches what it was built for
    rc_g, eds_g, p_g, err = ctx.repair_status(damaged, pres, rr, cr)
    _assert_exact(rc_g, eds_g, p_g, err, want)
    return want


# ---- A. honest squares: the oracle's extension is the reference --------------------------------------------------
def _pres_q0():
    pres = np.zeros((W, W), np.uint8)
    pres[:K, :K] = 1
    return _grid(pres)


def _pres_q3():
    pres = np.zeros((W, W), np.uint8)
    pres[K:, K:] = 1
    return _grid(pres)


def _pres_checkerboard():
    r, c = np.indices((W, W))
    return _grid((r + c) % 2 == 0)


def _pres_complete_axes():
    rng = np.random.default_rng(41)
    pres = (rng.random((W, W)) < 0.7).astype(np.uint8)
    for half in (0, K):  # 8 complete rows and 8 complete columns in each half
        pres[half + rng.choice(K, 8, replace=False), :] = 1
        pres[:, half + rng.choice(K, 8, replace=False)] = 1
    return _grid(pres)


@pytest.mark.parametrize("pattern", [_pres_q0, _pres_q3, _pres_checkerboard, _pres_complete_axes],
                         ids=["q0_only", "q3_only", "checkerboard", "sanity_passes"])
def test_repair_k256_honest(ctx, sq256, pattern):
    eds, rr, cr = sq256
    pres = pattern()
    if pattern is _pres_checkerboard:
        g = pres.reshape(W, W)
        assert (g.sum(0) == K).all() and (g.sum(1) == K).all()
    if pattern is _pres_complete_axes:
        g = pres.reshape(W, W)
        assert ((g.sum(1) == W).sum(), (g.sum(0) == W).sum()) == (16, 16)
    rc, got, p, _ = ctx.repair_status(_damaged(eds, pres), pres, rr, cr)
    assert rc == 0
    assert p.all()
    assert np.array_equal(got, eds)


# ---- A. prerepairSanityCheck outcomes ---------------------------------------------------------------------------
def test_repair_k256_sanity_root_mismatch(ctx, sq256):
    eds, rr, cr = sq256
    pres = (np.random.default_rng(42).random((W, W)) < 0.8).astype(np.uint8)
    pres[100, :] = 1
    bad = eds.copy()
    bad[100 * W + 31, 300] ^= 0x04  # one bit of a Q0 cell of complete row 100
    assert not (pres.sum(0) == W).any() and (pres.sum(1) == W).sum() == 1
    pres = _grid(pres)
    _repair_exact(ctx, _damaged(bad, pres), pres, rr, cr, (O.E_BYZANTINE, ROW, 100))


@pytest.mark.parametrize("missing,outcome", [((400, K + 9), (O.E_BYZANTINE, ROW, 5)),
                                             ((5, 17), (O.E_BYZANTINE, COL, K + 9))], ids=["row", "col"])
def test_repair_k256_sanity_parity_mismatch_with_matching_root(ctx, bad_q1, missing, outcome):
    """The committed square itself has a bad parity cell (5, k+9), so the roots of row 5 and column k+9 match and
    only the re-encode can tell.  One missing cell decides which of the two is complete."""
    bad, rr, cr = bad_q1
    pres = np.ones((W, W), np.uint8)
    pres[missing] = 0
    pres = _grid(pres)
    _repair_exact(ctx, _damaged(bad, pres), pres, rr, cr, outcome)


# ---- A. solveCrossword outcomes ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def first_batch_case(sq256):
    """60 % presence (every axis decodable at once: one batch of 2w operations) and a corrupted present cell of
    row 40 right of the diagonal, so row 40 meets it before any column does."""
    eds, rr, cr = sq256
    pres = (np.random.default_rng(43).random((W, W)) < 0.6).astype(np.uint8)
    assert (pres.sum(0) >= K).all() and (pres.sum(1) >= K).all() and not (pres.sum(0) == W).any()
    c = 41 + int(np.flatnonzero(pres[40, 41:])[3])
    bad = eds.copy()
    bad[40 * W + c, 9] ^= 0x81
    pres = _grid(pres)
    damaged = _damaged(bad, pres)
    want = _oracle_agreed(damaged, pres, rr, cr)
    assert (want[0], want[3], want[4]) == (O.E_BYZANTINE, ROW, 40)
    return _frozen(damaged, pres) + (want,)


@pytest.fixture(scope="module")
def unrepairable_case(sq256):
    eds, rr, cr = sq256
    pres = _grid(np.random.default_rng(44).random((W, W)) < 0.2)
    damaged = _damaged(eds, pres)
    want = _oracle_agreed(damaged, pres, rr, cr)
    assert want[0] == O.E_UNREPAIRABLE
    return _frozen(damaged, pres) + (want,)


def test_repair_k256_byzantine_first_batch(ctx, sq256, first_batch_case):
    damaged, pres, want = first_batch_case
    _assert_exact(*ctx.repair_status(damaged, pres, sq256[1], sq256[2]), want)


def test_repair_k256_byzantine_later_batch(ctx, sq256):
    """Batch 1 touches no root that the bad Q3 cell (k+3, k+7) affects; batch 2 fails and is replayed: row k,
    column k, ... row k+3.  Q0-Q2 and three rows and columns of Q3 are present afterwards."""
    bad, rr, cr = _commit_bad(sq256[0], K + 3, K + 7, 200)
    pres = _pres_q0()
    want = _repair_exact(ctx, _damaged(bad, pres), pres, rr, cr, (O.E_BYZANTINE, ROW, K + 3))
    assert int(want[2].sum()) == 3 * K * K + 3 * K + 3 * (K - 3) == 198135


def test_repair_k256_unrepairable_after_a_whole_square(ctx, sq256, unrepairable_case):
    eds, rr, cr = sq256
    damaged, pres, want = unrepairable_case
    rc, got, p, _ = ctx.repair_status(eds, np.ones(W * W, np.uint8), rr, cr)  # leaves a whole square on the device
    assert rc == 0 and p.all() and np.array_equal(got, eds)  # (a sanity check of all 2w axes, all passing)
    rc_g, eds_g, p_g, err = ctx.repair_status(damaged, pres, rr, cr)
    m = _assert_exact(rc_g, eds_g, p_g, err, want)
    left = eds_g[~m]
    assert np.all((left == 0) | (left == FILL))


# ---- A. the other two ways a square reaches the device --------------------------------------------------------------
def test_repair_k256_q0_in_registered_memory(ctx, sq256):
    eds, rr, cr = sq256
    pres = _pres_q0()
    square = _damaged(eds, pres)
    ctx.host_register(square)
    try:
        rc, _, _, _ = ctx.repair_status(square, pres, rr, cr, inplace=True)
        assert rc == 0
        assert pres.all()
        assert np.array_equal(square, eds)
    finally:
        ctx.host_unregister(square)


@pytest.mark.parametrize("case", ["first_batch_case", "unrepairable_case"])
def test_repair_device_k256(ctx, sq256, case, request):
    import torch
    damaged, pres, want = request.getfixturevalue(case)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    d = torch.from_numpy(damaged.copy()).to(dev)
    torch.cuda.synchronize()
    rc_g, p_g, err = ctx.repair_device(K, d.data_ptr(), pres, sq256[1], sq256[2], s.cuda_stream)
    s.synchronize()
    _assert_exact(rc_g, d.cpu().numpy(), p_g, err, want)


# ---- B. k = 512 -----------------------------------------------------------------------------------------------------
def test_repair_k512(ctx):
    k, w = 512, 1024
    rc, eds, rr, cr, _ = O.extend_commit(O.gen_ods(k, 11))
    assert rc == 0
    rng = np.random.default_rng(45)
    pres = np.ones((w, w), np.uint8)
    for r in rng.choice(w, 24, replace=False):
        pres[r, rng.choice(w, 500, replace=False)] = 0
    assert (pres.sum(1) == w).sum() == w - 24
    pres = _grid(pres)
    square = _damaged(eds, pres)
    rc, _, _, _ = ctx.repair_status(square, pres, rr, cr, inplace=True)
    assert rc == 0
    assert pres.all()
    assert np.array_equal(square, eds)


# ---- C. cda_rs_encode_device, batched and strided -----------------------------------------------------------------
def _encode_device_both_layouts(ctx, k, ncw, L, seed):
    import torch
    dev = torch.device("cuda", 0)
    data = np.random.default_rng(seed).integers(0, 256, (ncw, k, L), dtype=np.uint8)
    ref = np.stack([O.leo_encode(data[c]) for c in range(ncw)])

    def first_bad(got):
        bad = np.flatnonzero((got != ref).any(axis=(1, 2)))
        return None if bad.size == 0 else int(bad[0])

    # codeword c = data[c], shards contiguous; one codeword of room behind the last must stay untouched
    d_src = torch.from_numpy(data).to(dev)
    d_dst = torch.full((ncw + 1, k, L), 0xA5, dtype=torch.uint8, device=dev)
    ctx.rs_encode_device(k, L, ncw, d_src.data_ptr(), k * L, L, d_dst.data_ptr(), k * L, L)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert first_bad(got[:ncw]) is None, "contiguous codewords"
    assert (got[ncw] == 0xA5).all()
    # the same codewords as the columns of a k x ncw grid (src_cw = one shard, src_sh = the grid's pitch)
    d_src = torch.from_numpy(np.ascontiguousarray(data.transpose(1, 0, 2))).to(dev)
    d_dst = torch.full((k, ncw, L), 0xA5, dtype=torch.uint8, device=dev)
    ctx.rs_encode_device(k, L, ncw, d_src.data_ptr(), L, ncw * L, d_dst.data_ptr(), L, ncw * L)
    torch.cuda.synchronize()
    assert first_bad(d_dst.cpu().numpy().transpose(1, 0, 2)) is None, "column codewords"


@pytest.mark.parametrize("k,ncw,L", [(129, 3, 512), (256, 5, 512), (300, 3, 512), (256, 2, 64), (1024, 2, 512)])
def test_rs_encode_device_ff16_lds_encoder(ctx, k, ncw, L):
    _encode_device_both_layouts(ctx, k, ncw, L, 1000 * k + ncw)


@pytest.mark.parametrize("shape", ["three", "ncu_plus_1", "ncu_plus_half", "two_slices"])
def test_rs_encode_device_ff16_register_encoder(ctx, shape):
    """The persistent encoder runs min(codeword slices, CUs) workgroups; workgroup g walks g, g + grid, ..."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    ncw, L = {"three": (3, 512), "ncu_plus_1": (ncu + 1, 512), "ncu_plus_half": (ncu + ncu // 2, 512),
              "two_slices": (2, 1024)}[shape]
    _encode_device_both_layouts(ctx, 512, ncw, L, ncw)


# ---- D. cda_rs_decode, structured loss ------------------------------------------------------------------------------
def _survivors(k, pattern):
    pres = np.zeros(2 * k, np.uint8)
    if pattern == "parity_only":
        pres[k:] = 1
    elif pattern == "window":
        pres[k // 2:k // 2 + k] = 1
    elif pattern == "even":
        pres[0::2] = 1
    else:  # "ends": the first ceil(k/2) data shards and the last floor(k/2) parity shards
        pres[:(k + 1) // 2] = 1
        pres[2 * k - k // 2:] = 1
    assert pres.sum() == k
    return pres


@pytest.mark.parametrize("pattern", ["parity_only", "window", "even", "ends"])
@pytest.mark.parametrize("k", [129, 256, 300, 512])
def test_rs_decode_ff16_structured_loss(ctx, k, pattern):
    L = 128
    d = np.random.default_rng(2000 + k).integers(0, 256, (k, L), dtype=np.uint8)
    full = np.concatenate([d, O.leo_encode(d)])
    pres = _survivors(k, pattern)
    damaged = np.where(pres[:, None] == 1, full, 0x5C).astype(np.uint8)
    if k == 300:  # the oracle's own decoder agrees that `full` is the answer
        rc, dec = O.leo_decode(damaged, pres)
        assert rc == 0 and np.array_equal(dec, full)
    assert np.array_equal(ctx.rs_decode(damaged, pres), full)
