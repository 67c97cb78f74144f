"""The batched block path's RS schedule for whole batches on the register encoder: Q1 and Q2 straight from the ODS in
one launch, Q3 from Q2 by rows, the Q0 copy on the context's second stream beside the hashing, and a leaf kernel that
reads Q0 cells (and the push-order neighbours) from the ODS.  Shapes (k, B), the smallest that can take it for each
encoder body, and two that must keep the two passes (the release library takes it from 256 MiB of ODS on, so these run
on the test-hooks library opened with CDA_RS_MIN_ODS_MIB=0, again on the release library whatever it chooses there,
and (128, 32), the release library's own threshold, closes the gap):

  (16, 4)    L = 4, no LDS exchange, the grid exactly at the latency threshold (32 workgroups per job)
  (16, 5)    L = 4, one block past it
  (32, 3)    L = 5
  (64, 2)    L = 6
  (128, 2)   L = 7
  (8, 4)     the LDS encoder: the two passes
  (16, 1)    the latency form: the two passes

Every block is one of four kinds: a namespace-sorted random square; three long runs of equal namespaces; a square with
two shares of a row swapped (out of push order in that row); a square with two whole rows swapped (every row in
order, the columns not).  A batch too small for the four runs as many batches as it takes.  Every EDS byte, row and
column root, record padding, DAH and status word is compared with the CPU oracle (tests/oracle_lib.py); the status
word of a block out of order is the smallest violation key (axis << 40 | index << 20 | leaf) worked out from the ODS
here, and the oracle rejects exactly those blocks.

Ordering, with no host synchronisation between the calls: two calls into one EDS buffer (a stream-ordered snapshot
between them sees the first call's whole EDS), and one ODS buffer overwritten by a stream-ordered copy between two
calls.  (16, 5) and (128, 2) are also compared byte for byte with the test-hooks library opened with CDA_RS_SCHED=0
(the two passes).  cda_extend_commit_batch with the EDS copied out at (64, 3): the host-buffer batch runs on the
context's own stream and keeps the two passes (engine.cpp rs_from_ods); its bytes are checked all the same."""
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

CASES = [(16, 4), (16, 5), (32, 3), (64, 2), (128, 2), (8, 4), (16, 1)]
AB_CASES = [(16, 5), (128, 2)]
KINDS = ["random", "equal", "bad_row", "bad_col"]
CLEAN = -1  # the status word of a block whose namespaces are in push order

_REF = {}  # (k, kind) -> (ods, eds, rr, cr, dah, status): computed once, never written to


def _ods(k, kind):
    if kind == "random":
        return O.gen_ods(k, 0x0FF0 + 131 * k)
    if kind == "equal":  # row-major non-decreasing runs: every row and column is sorted
        ods = O.gen_ods(k, 0xE0 + k).copy()
        ods[:, 19:29] = 0
        ods[:, 28] = 0x10 + (np.arange(k * k) * 3) // (k * k)
        return ods
    ods = O.gen_ods(k, 0xBAD0 + k + len(kind)).copy().reshape(k, k, 512)
    if kind == "bad_row":  # row 1: leaves 2 and 3 swapped
        ods[1, [2, 3]] = ods[1, [3, 2]]
    else:  # rows k - 3 and k - 2 swapped: each row stays sorted, every column with distinct namespaces there is not
        ods[[k - 3, k - 2]] = ods[[k - 2, k - 3]]
    return ods.reshape(k * k, 512)


def _status(ods, k):
    """The smallest violation key of the block, as leaf_hash_kernel's atomicMin leaves it (-1: none)."""
    ns = [ods[i, :29].tobytes() for i in range(k * k)]
    best = None
    for r in range(k):
        for c in range(k):
            keys = []
            if c + 1 < k and ns[r * k + c + 1] < ns[r * k + c]:
                keys.append((0 << 40) | (r << 20) | (c + 1))
            if r + 1 < k and ns[(r + 1) * k + c] < ns[r * k + c]:
                keys.append((1 << 40) | (c << 20) | (r + 1))
            for key in keys:
                best = key if best is None else min(best, key)
    return CLEAN if best is None else best


def _ref(k, kind):
    if (k, kind) not in _REF:
        ods = _ods(k, kind)
        rc, _, rr, cr, dah = O.extend_commit(ods, want_eds=False)
        status = _status(ods, k)
        assert (rc == 0) == (status == CLEAN), (k, kind, rc, hex(status))
        assert (status == CLEAN) == (kind in ("random", "equal")), (k, kind, hex(status))
        for a in (ods, rr, cr):
            a.setflags(write=False)
        _REF[(k, kind)] = (ods, O.extend(ods), rr, cr, dah, status)
    return _REF[(k, kind)]


def _batches(k, B):
    """Lists of B kinds that between them hold the four (one batch when B >= 4)."""
    kinds = ["random"] * max(B - 4, 0) + KINDS
    kinds += ["random"] * (-len(kinds) % B)
    return [kinds[i:i + B] for i in range(0, len(kinds), B)]


def _stack(k, kinds):
    return np.stack([_ref(k, kind)[0] for kind in kinds])


class _Out:
    def __init__(self, k, B, dev):
        import torch
        w = 2 * k
        self.eds = torch.empty((B, w * w, 512), dtype=torch.uint8, device=dev)
        self.roots = torch.empty((B, 2 * w, 96), dtype=torch.uint8, device=dev)
        self.dah = torch.empty((B, 32), dtype=torch.uint8, device=dev)
        self.status = torch.empty((B,), dtype=torch.int64, device=dev)

    def host(self):
        return tuple(t.cpu().numpy() for t in (self.eds, self.roots, self.dah, self.status))


def _enqueue(ctx, k, B, d_ods, out, s):
    ctx.extend_commit_device(k, B, d_ods.data_ptr(), out.eds.data_ptr(), out.roots.data_ptr(), out.dah.data_ptr(),
                             out.status.data_ptr(), s.cuda_stream)


def _run(ctx, ods):
    import torch
    B, kk, _ = ods.shape
    k = int(round(kk ** 0.5))
    dev = torch.device("cuda", 0)
    d_ods = torch.from_numpy(ods).to(dev)
    out = _Out(k, B, dev)
    s = torch.cuda.Stream(dev)
    _enqueue(ctx, k, B, d_ods, out, s)
    s.synchronize()
    return out.host()


def _check(k, kinds, eds, roots, dah, status, what=""):
    w = 2 * k
    for b, kind in enumerate(kinds):
        _, eds_o, rr, cr, dah_o, st_o = _ref(k, kind)
        tag = (k, b, kind, what)
        assert np.array_equal(eds[b], eds_o), tag + ("eds",)
        assert int(status[b]) == st_o, tag + (hex(int(status[b])), hex(st_o))
        if st_o != CLEAN:
            continue  # the oracle rejects the block: no roots to compare
        assert np.array_equal(roots[b, :w, :90], rr), tag + ("row roots",)
        assert np.array_equal(roots[b, w:, :90], cr), tag + ("column roots",)
        assert not roots[b, :, 90:].any(), tag + ("record padding",)
        assert dah[b].tobytes() == dah_o, tag + ("dah",)


def _hooks_ctx(env):
    """A context of the test-hooks library opened with these switches in the environment (read at cda_init; the
    release library has none of them)."""
    import cda
    from cda import _native as N
    old = {name: os.environ.get(name) for name in env}
    os.environ.update(env)
    try:
        return cda.Context(0, lib_path=N.HOOKS_LIB_PATH)
    finally:
        for name, v in old.items():
            if v is None:
                del os.environ[name]
            else:
                os.environ[name] = v


@pytest.fixture(scope="module")
def from_ods_ctx():
    """The new schedule at every batch size that can take it (CDA_RS_MIN_ODS_MIB=0): the release library keeps the
    two passes below 256 MiB of ODS, where the fork and join cost more than the schedule saves."""
    c = _hooks_ctx({"CDA_RS_MIN_ODS_MIB": "0"})
    yield c
    c.close()


@pytest.fixture(scope="module")
def two_pass_ctx():
    """The two RS passes at every batch size (CDA_RS_SCHED=0)."""
    c = _hooks_ctx({"CDA_RS_SCHED": "0"})
    yield c
    c.close()


@pytest.mark.parametrize("k,B", CASES)
def test_matches_oracle(from_ods_ctx, k, B):
    for kinds in _batches(k, B):
        _check(k, kinds, *_run(from_ods_ctx, _stack(k, kinds)))


@pytest.mark.parametrize("k,B", CASES)
def test_release_library_matches_oracle(ctx, k, B):
    for kinds in _batches(k, B):
        _check(k, kinds, *_run(ctx, _stack(k, kinds)))


def test_release_library_at_its_threshold(ctx):
    """(128, 32): 256 MiB of ODS, the smallest k = 128 batch for which the release library takes the new schedule."""
    k, B = 128, 32
    kinds = (KINDS * B)[:B]
    _check(k, kinds, *_run(ctx, _stack(k, kinds)))


@pytest.mark.parametrize("k,B", AB_CASES)
def test_same_bytes_as_the_two_passes(from_ods_ctx, two_pass_ctx, k, B):
    for kinds in _batches(k, B):
        ods = _stack(k, kinds)
        new, old = _run(from_ods_ctx, ods), _run(two_pass_ctx, ods)
        for x, y, what in zip(new, old, ("eds", "roots", "dah", "status")):
            assert x.tobytes() == y.tobytes(), (k, kinds, what)


def test_two_calls_into_one_eds_buffer(from_ods_ctx):
    """Two ODS buffers, one EDS buffer, one stream, no host wait in between: a stream-ordered snapshot taken between
    the calls holds the first call's whole EDS (Q0 included), the buffer itself the second call's."""
    import torch
    ctx = from_ods_ctx
    k, B = 128, 2
    first, second = _batches(k, B)
    dev = torch.device("cuda", 0)
    d_a, d_b = torch.from_numpy(_stack(k, first)).to(dev), torch.from_numpy(_stack(k, second)).to(dev)
    out_a, out_b = _Out(k, B, dev), _Out(k, B, dev)
    out_b.eds = out_a.eds
    snap = torch.empty_like(out_a.eds)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        _enqueue(ctx, k, B, d_a, out_a, s)
        snap.copy_(out_a.eds, non_blocking=True)
        _enqueue(ctx, k, B, d_b, out_b, s)
    s.synchronize()
    _, roots_a, dah_a, status_a = out_a.host()
    _check(k, first, snap.cpu().numpy(), roots_a, dah_a, status_a, "first call")
    _check(k, second, *out_b.host(), "second call")


def test_ods_buffer_overwritten_between_two_calls(from_ods_ctx):
    """One ODS buffer that a stream-ordered device copy overwrites right after the first call, a second call behind
    it: the first call's Q0 copy and leaf kernel have read the ODS before the copy lands."""
    import torch
    ctx = from_ods_ctx
    k, B = 128, 2
    first, second = _batches(k, B)
    dev = torch.device("cuda", 0)
    d_ods = torch.from_numpy(_stack(k, first)).to(dev)
    d_next = torch.from_numpy(_stack(k, second)).to(dev)
    out_a, out_b = _Out(k, B, dev), _Out(k, B, dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        _enqueue(ctx, k, B, d_ods, out_a, s)
        d_ods.copy_(d_next, non_blocking=True)
        _enqueue(ctx, k, B, d_ods, out_b, s)
    s.synchronize()
    _check(k, first, *out_a.host(), "first call")
    _check(k, second, *out_b.host(), "second call")


def test_host_batch_copies_the_whole_eds_out(ctx):
    """cda_extend_commit_batch with the EDS copied out: every byte of Q0 is there when a slot's D2H reads it."""
    k, kinds = 64, ["random", "equal", "random"]
    eds, rr, cr, dah = ctx.extend_commit_batch(_stack(k, kinds), want_eds=True)
    for b, kind in enumerate(kinds):
        _, eds_o, rr_o, cr_o, dah_o, _ = _ref(k, kind)
        assert np.array_equal(eds[b], eds_o), (b, "eds")
        assert np.array_equal(rr[b], rr_o) and np.array_equal(cr[b], cr_o), (b, "roots")
        assert bytes(dah[b]) == dah_o, (b, "dah")
