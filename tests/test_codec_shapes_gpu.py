"""GPU tests of every launch shape of the erasure decoder (rs_decode_kernel) and of the GF(2^8) LDS encoder
(rs_encode8_kernel): the cases of tests/codec_cases.py, which tests/test_codec_shapes.py proves to reach every cell
the launch rules (csrc/codec_shape.h) can produce.  Everything is bit-exact against the CPU oracle.

A. cda_rs_decode, one codeword per call: the shard length alone selects U, the units per workgroup that every index
   of the kernel depends on.  Random bytes, missing shards filled with 0x5C; the result must be
   data ‖ leo_encode(data) byte for byte, and the oracle's independent Lagrange decoder must return the same from
   the same damaged input.
B. cda_axis_halves_verify with 512 second-side halves at k = 16: 512 codewords of 512-byte shards in one launch
   (U = 16, one workgroup per codeword), offsets and strides from the prep kernel; statuses against
   cda.rows.verify_host.
C. rs_encode8_kernel through cda_rs_encode (one codeword) and cda_rs_encode_device (contiguous codewords and codewords
   as columns of a k x ncw grid, a guard codeword behind the last) against leo_encode, per codeword."""
import functools

import numpy as np
import pytest

import codec_cases as CC
import oracle_lib as O
from cda import rows
from cda.rows import BAD_ROOT, PLACED
from test_axis_halves import CODEC, block, every_half, flipped_half
from test_ff16_paths_gpu import _encode_device_both_layouts

pytestmark = pytest.mark.gpu

FILL = 0x5C  # the caller's bytes in missing shards: ignored and overwritten


@functools.lru_cache(maxsize=4)
def _codeword(k, L):
    """(k, L) random data and its parity, once per shape (read-only)."""
    d = np.random.default_rng(7000 + 31 * k + L).integers(0, 256, (k, L), dtype=np.uint8)
    full = np.concatenate([d, O.leo_encode(d)])
    full.flags.writeable = False
    return full


def _first_bad(got, want, cell):
    """None, or where the first wrong byte is: the shard, the offset in it, and that offset in units of the
    workgroup's U * unit bytes (a remainder of 0 at every bad run points at a unit, anything else at a position)."""
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size == 0:
        return None
    shard = int(bad[0])
    off = int(np.flatnonzero(got[shard] != want[shard])[0])
    span = cell[2] * cell[0] * 4
    return (f"first bad shard {shard} of {len(bad)} bad, first bad byte at offset {off} = workgroup slice {off // span}"
            f" + {off % span} (U * unit = {span}, unit {off % span // (cell[0] * 4)} of the slice)")


def _decode_case(ctx, k, L, cell, pattern, seed):
    full = _codeword(k, L)
    pres = CC.survivors(k, pattern, seed)
    damaged = np.where(pres[:, None] == 1, full, FILL).astype(np.uint8)
    rc, ref = O.leo_decode(damaged, pres)
    assert rc == 0 and np.array_equal(ref, full), "the oracle's Lagrange decoder disagrees: not a reference"
    got = ctx.rs_decode(damaged, pres)
    bad = _first_bad(got, full, cell)
    assert bad is None, f"k={k} L={L} cell={cell} mask={pattern} present={np.flatnonzero(pres).tolist()[:40]}: {bad}"


GROUPS = sorted({c[2][:2] for c in CC.DECODE_CASES})


@pytest.mark.parametrize("field,log2n", GROUPS, ids=[f"gf{f}-n{1 << n}" for f, n in GROUPS])
def test_rs_decode_every_cell(ctx, field, log2n):
    ran = 0
    for index, (k, L, cell, patterns) in enumerate(CC.DECODE_CASES):
        if cell[:2] != (field, log2n):
            continue
        for t, pattern in enumerate(patterns):
            _decode_case(ctx, k, L, cell, pattern, 100 * index + t)
            ran += 1
    assert ran >= 2


@pytest.mark.parametrize("k,L", [(5, 65536), (129, 65536)], ids=["gf8", "gf16"])
def test_rs_decode_runs_on_the_device(ctx, k, L):
    """No silent fallback: one decode call is one more launch of the axis queue's decoder."""
    full = _codeword(k, L)
    pres = CC.survivors(k, "random_k", k)
    damaged = np.where(pres[:, None] == 1, full, FILL).astype(np.uint8)
    ctx.profile_enable(True)
    try:
        before = ctx.profile_read().get("axis_rs_decode", (0.0, 0))[1]
        got = ctx.rs_decode(damaged, pres)
        after = ctx.profile_read().get("axis_rs_decode", (0.0, 0))[1]
    finally:
        ctx.profile_enable(False)
    assert after == before + 1
    assert np.array_equal(got, full)


def test_halves_verify_512_codewords_at_u16(ctx):
    """B: every second-side half of one honest k = 16 square, eight times over, a few of them with one flipped byte
    in one cell; each half is verified on its own, so the statuses are those of the host rule for the same batch."""
    k, L, ncw, _ = CC.HALVES_CASE
    assert L == 512
    _, eds, rr, cr, _ = block(k)
    second = [h for h in every_half(eds, k) if h.side == 1]
    assert len(second) == 4 * k
    halves = (second * (ncw // len(second) + 1))[:ncw]
    flips = {0: (0, 100), 1: (k - 1, 511), 255: (7, 29), 256: (3, 0), 300: (k // 2, 257), ncw - 1: (k - 1, 30)}
    for at, (cell, byte) in flips.items():
        halves[at] = flipped_half(halves[at], cell, byte)
    want, want_axes = rows.verify_host(halves, rr, cr, CODEC)
    assert [i for i, s in enumerate(want) if s != PLACED] == sorted(flips) and set(want[sorted(flips)]) == {BAD_ROOT}
    ctx.profile_enable(True)
    try:
        before = ctx.profile_read().get("axis_half_rs_decode", (0.0, 0))[1]
        got, axes = rows.verify(ctx, halves, rr, cr, want_axes=True)
        after = ctx.profile_read().get("axis_half_rs_decode", (0.0, 0))[1]
    finally:
        ctx.profile_enable(False)
    assert after == before + 1  # all 512 codewords in one decoder launch
    assert got.tolist() == want.tolist()
    good = want == PLACED
    wrong = np.flatnonzero((axes[good] != want_axes[good]).any(axis=(1, 2)))
    assert wrong.size == 0, f"completed axes differ, first at verified half {int(wrong[0])}"


@pytest.mark.parametrize("k,L,ncw,form,cell", CC.ENCODE8_CASES,
                         ids=[f"k{c[0]}-L{c[1]}-n{c[2]}" for c in CC.ENCODE8_CASES])
def test_rs_encode8_lds_every_cell(ctx, k, L, ncw, form, cell):
    seed = 9000 + 1000 * k + L + ncw
    if form == "host":
        d = np.random.default_rng(seed).integers(0, 256, (k, L), dtype=np.uint8)
        got, want = ctx.rs_encode(d), O.leo_encode(d)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (f"cell={cell}: first bad parity shard {int(bad[0])}, first bad byte "
                               f"{int(np.flatnonzero(got[bad[0]] != want[bad[0]])[0])}")
    else:
        _encode_device_both_layouts(ctx, k, ncw, L, seed)
