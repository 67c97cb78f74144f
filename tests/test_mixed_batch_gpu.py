"""GPU tests of the mixed-size batch: cda_extend_commit_mixed / cda_extend_commit_mixed_device and, behind them,
small_square_kernel (a whole k <= 8 square from ODS to DAH in one workgroup).  Every comparison is bit-exact against
the CPU oracle: block b of a call must be what cda_extend_commit returns for that block alone."""
import functools

import numpy as np
import pytest

import kat
import oracle_lib as O

pytestmark = pytest.mark.gpu

KS = [1, 8, 2, 2, 16, 4, 1, 8, 32, 4, 16, 1]  # 16 twice and apart: a group is gathered and scattered
CLEAN = -1  # an all-ones status word read as int64


@pytest.fixture(scope="module")
def mctx():
    """A context of this module's own: the tests move its CDA_OPT_MIXED_SMALL_MAX."""
    import cda
    c = cda.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def block(k, seed):
    """(ods, eds, row roots, column roots, dah) of one oracle block; computed once, never written to."""
    ods = O.gen_ods(k, seed)
    rc, eds, rr, cr, dah = O.extend_commit(ods)
    assert rc == 0
    for a in (ods, eds, rr, cr):
        a.setflags(write=False)
    return ods, eds, rr, cr, dah


def batch(ks, seed0=0x5EED):
    return [block(k, seed0 + 31 * b + k) for b, k in enumerate(ks)]


def check_block(got, want, b, with_eds=True):
    eds, rr, cr, dah = got
    _, eds_o, rr_o, cr_o, dah_o = want
    if with_eds:
        assert np.array_equal(eds, eds_o), f"block {b}: EDS"
    else:
        assert eds is None
    assert np.array_equal(rr, rr_o), f"block {b}: row roots"
    assert np.array_equal(cr, cr_o), f"block {b}: column roots"
    assert dah == dah_o, f"block {b}: DAH"


def run_host(ctx, blocks, want_eds=True):
    eds, rr, cr, dah = ctx.extend_commit_mixed([blk[0] for blk in blocks], want_eds=want_eds)
    return list(zip(eds, rr, cr, dah))


# ---- 1. each small size alone ----
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_each_small_size_alone(mctx, k):
    want = block(k, 0xA11 + k)
    (got,) = run_host(mctx, [want])
    check_block(got, want, 0)


def test_small_known_answers(mctx):
    from cda import da
    one = np.frombuffer(da.min_shares()[0], np.uint8).reshape(1, 512)
    two = np.stack([np.frombuffer(bytes(s), np.uint8) for s in kat.generate_shares(4)])
    _, _, _, dah = mctx.extend_commit_mixed([one, two])
    assert dah[0] == kat.MIN_DAH
    assert dah[1] == kat.TYPICAL_K2


# ---- 2. mixed batch ----
@pytest.mark.parametrize("want_eds", [True, False])
def test_mixed_batch(mctx, want_eds):
    blocks = batch(KS)
    got = run_host(mctx, blocks, want_eds)
    assert len(got) == len(KS)
    for b, (g, w) in enumerate(zip(got, blocks)):
        check_block(g, w, b, want_eds)


# ---- 3. the same outputs on every route ----
def test_same_outputs_on_every_route(mctx):
    import cda
    from cda import _native as N
    blocks = batch(KS)
    try:
        for small_max in (0, 1, 2, 4, 8):
            mctx.set_option(N.OPT_MIXED_SMALL_MAX, small_max)
            for b, (g, w) in enumerate(zip(run_host(mctx, blocks), blocks)):
                check_block(g, w, (small_max, b))
        for bad in (3, 16, -1, 5):
            with pytest.raises(cda.CdaError) as ei:
                mctx.set_option(N.OPT_MIXED_SMALL_MAX, bad)
            assert ei.value.code == N.E_ARG
    finally:
        mctx.set_option(N.OPT_MIXED_SMALL_MAX, 8)


# ---- 4. more workgroups than the chip holds at once ----
def test_many_small_blocks(mctx):
    rng = np.random.default_rng(520)
    ks = [int(k) for k in rng.choice([1, 2, 4, 8], 520)]
    assert set(ks) == {1, 2, 4, 8}
    blocks = batch(ks, 0xB10C)
    got = run_host(mctx, blocks, want_eds=False)
    for b, (g, w) in enumerate(zip(got, blocks)):
        check_block(g, w, b, with_eds=False)


# ---- 5. large and wide fields in the mix ----
@pytest.mark.parametrize("ks", [[128, 1, 8], [2, 256, 4]])
def test_large_blocks_in_the_mix(mctx, ks):
    blocks = batch(ks, 0xF16)
    for b, (g, w) in enumerate(zip(run_host(mctx, blocks), blocks)):
        check_block(g, w, b)


# ---- 6. order errors ----
def swapped(k, seed):
    """A k x k ODS with leaves 2 and 3 of row 1 swapped."""
    ods = O.gen_ods(k, seed).copy()
    ods[[k + 2, k + 3]] = ods[[k + 3, k + 2]]
    assert ods[k + 2, :29].tobytes() > ods[k + 3, :29].tobytes()
    return ods


def order_case():
    ks = [4, 8, 2, 8]
    good = batch(ks, 0x0DD)
    ods = [good[0][0], swapped(8, 0x0DD + 1), good[2][0], swapped(8, 0x0DD + 3)]
    return ks, good, ods


def test_order_error_names_the_lowest_block(mctx):
    import cda
    ks, _, ods = order_case()
    with pytest.raises(cda.CdaError) as ei:
        mctx.extend_commit_mixed(ods)
    e = ei.value
    assert (e.code, e.block, e.axis, e.index, e.leaf) == (-5, 1, 0, 1, 3)


def test_column_only_violation_in_a_batch(mctx, ctx):
    import cda
    k = 4
    ods = O.gen_ods(k, 98).reshape(k, k, 512).copy()
    # column 2 decreases between rows 1 and 2 while every row stays sorted (tests/test_gpu_parity.py)
    ods[2, :, 19:29] = 0
    ods[2, :, 29:] = 0
    ods[3, :, 19:29] = 0
    ods = np.sort(ods.reshape(k * k, 512).view("S512").reshape(k, k), axis=1).view(np.uint8).reshape(k * k, 512)
    with pytest.raises(cda.CdaError) as alone:
        ctx.extend_commit(ods)
    a = alone.value
    assert a.code == -5 and a.axis == 1
    good = batch([2, 8], 0xC01)
    with pytest.raises(cda.CdaError) as ei:
        mctx.extend_commit_mixed([good[0][0], good[1][0], ods])
    e = ei.value
    assert (e.code, e.block, e.axis, e.index, e.leaf) == (-5, 2, a.axis, a.index, a.leaf)


# ---- 7. device form ----
def run_device(ctx, ks, ods_list, stream, torch):
    """Enqueue one device-form call on `stream`; returns the tensors (read them after a synchronise)."""
    from cda import _native as N
    off = N.mixed_offsets(ks)
    dev = torch.device("cuda", 0)
    d_ods = torch.from_numpy(np.concatenate(ods_list)).to(dev)
    d_eds = torch.zeros((int(off["eds"][-1]),), dtype=torch.uint8, device=dev)
    d_roots = torch.zeros((int(off["recs"][-1]), 96), dtype=torch.uint8, device=dev)
    d_dah = torch.zeros((len(ks), 32), dtype=torch.uint8, device=dev)
    d_status = torch.zeros((len(ks),), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()  # the buffers are ready before another stream uses them
    ctx.extend_commit_mixed_device(ks, d_ods.data_ptr(), d_eds.data_ptr(), d_roots.data_ptr(), d_dah.data_ptr(),
                                   d_status.data_ptr(), stream.cuda_stream)
    return off, d_ods, d_eds, d_roots, d_dah, d_status


def check_device(ks, blocks, out, skip=()):
    off, _, d_eds, d_roots, d_dah, d_status = out
    eds, roots, dah, status = (t.cpu().numpy() for t in (d_eds, d_roots, d_dah, d_status))
    for b, (k, want) in enumerate(zip(ks, blocks)):
        if b in skip:
            continue
        w = 2 * k
        assert status[b] == CLEAN, (b, hex(int(status[b])))
        recs = roots[off["recs"][b]:off["recs"][b + 1]]
        assert not recs[:, 90:].any(), b  # 90-B node + 6 zero bytes per record
        got = (eds[off["eds"][b]:off["eds"][b + 1]].reshape(-1, 512), recs[:w, :90], recs[w:, :90], dah[b].tobytes())
        check_block(got, want, b)
    return status


def test_device_form_matches(mctx):
    import torch
    blocks = batch(KS)
    s = torch.cuda.Stream(torch.device("cuda", 0))
    out = run_device(mctx, KS, [blk[0] for blk in blocks], s, torch)
    s.synchronize()
    check_device(KS, blocks, out)


def test_device_form_back_to_back(mctx):
    """Two calls on one context with different ks and no synchronise between them: the second call's descriptor table
    must not replace the first's before the device has read it."""
    import torch
    ks1, ks2 = KS, [8, 4, 2, 1, 16, 8, 8, 1, 2]
    b1, b2 = batch(ks1), batch(ks2, 0x2D)
    s = torch.cuda.Stream(torch.device("cuda", 0))
    dev = torch.device("cuda", 0)
    from cda import _native as N
    outs = []
    for ks, blocks in ((ks1, b1), (ks2, b2)):
        off = N.mixed_offsets(ks)
        outs.append((off, torch.from_numpy(np.concatenate([blk[0] for blk in blocks])).to(dev),
                     torch.zeros((int(off["eds"][-1]),), dtype=torch.uint8, device=dev),
                     torch.zeros((int(off["recs"][-1]), 96), dtype=torch.uint8, device=dev),
                     torch.zeros((len(ks), 32), dtype=torch.uint8, device=dev),
                     torch.zeros((len(ks),), dtype=torch.int64, device=dev)))
    torch.cuda.synchronize()
    for ks, (off, d_ods, d_eds, d_roots, d_dah, d_status) in zip((ks1, ks2), outs):
        mctx.extend_commit_mixed_device(ks, d_ods.data_ptr(), d_eds.data_ptr(), d_roots.data_ptr(), d_dah.data_ptr(),
                                        d_status.data_ptr(), s.cuda_stream)
    s.synchronize()
    check_device(ks1, b1, outs[0])
    check_device(ks2, b2, outs[1])


def test_device_form_order_errors(mctx):
    import torch
    ks, good, ods = order_case()
    s = torch.cuda.Stream(torch.device("cuda", 0))
    out = run_device(mctx, ks, ods, s, torch)
    s.synchronize()
    status = check_device(ks, good, out, skip=(1, 3))  # blocks 0 and 2: clean status, right EDS, roots and DAH
    key = (0 << 40) | (1 << 20) | 3
    assert int(status[1]) == key and int(status[3]) == key, [hex(int(x)) for x in status]


# ---- 8. the batched header call ----
def test_headers_from_shares(mctx):
    from cda import da
    lists = [da.min_shares(), [bytes(s) for s in kat.generate_shares(4)], [bytes(s) for s in kat.generate_shares(64)]]
    got = da.new_data_availability_headers_from_shares(lists, ctx=mctx)
    assert len(got) == 3
    for shares, dah in zip(lists, got):
        one = da.new_data_availability_header_from_shares(shares, ctx=mctx)
        assert dah.row_roots == one.row_roots and dah.column_roots == one.column_roots
        assert dah.hash() == one.hash()
        dah.validate_basic()
    assert got[0].hash() == kat.MIN_DAH and got[1].hash() == kat.TYPICAL_K2
