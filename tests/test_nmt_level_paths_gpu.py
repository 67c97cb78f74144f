"""The batched tree path (nmt_levels_kernel launches, then dah_kernel) at the smallest batches that reach it.

cda_extend_commit_device takes batches with nblocks * 4k <= 512 through trees_lds_kernel; the batches below are one
block past that bound for each k, so they run the level kernels: the row-tree lane permutation (a wave holds left
halves only or right halves only), the digest-only parity node (hash_node_parity) wherever a whole wave is parity,
and the general node everywhere else.  The tree depths are L = 4..9, so the launch sequence takes every split of
two-level launches and a final launch it has.  Every row root, column root, DAH and status word is compared with the
CPU oracle (tests/oracle_lib.py)."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

CASES = [(8, 17), (16, 9), (32, 5), (64, 3), (128, 2), (256, 1)]
CLEAN = np.int64(-1)  # the status word of a block whose namespaces are in push order


def _equal_ns_block(k, seed):
    """A namespace-sorted ODS of three long runs of equal namespaces (inner nodes with min == max, nodes whose two
    children carry different ranges, and the Q0 / parity boundary at every level)."""
    ods = O.gen_ods(k, seed).copy()
    run = (np.arange(k * k) * 3) // (k * k)  # row-major non-decreasing: every row and column is sorted
    ods[:, 19:29] = 0
    ods[:, 28] = 0x10 + run
    return ods


def _batch(k, B):
    ods = np.stack([O.gen_ods(k, 0x51AB + 131 * k + b) for b in range(B)])
    ods[B - 1] = _equal_ns_block(k, 0xE0 + k)
    return ods


def _run(ctx, ods):
    import torch
    B, kk, _ = ods.shape
    k = int(round(kk ** 0.5))
    w = 2 * k
    dev = torch.device("cuda", 0)
    d_ods = torch.from_numpy(ods).to(dev)
    d_eds = torch.empty((B, w * w, 512), dtype=torch.uint8, device=dev)
    d_roots = torch.empty((B, 2 * w, 96), dtype=torch.uint8, device=dev)
    d_dah = torch.empty((B, 32), dtype=torch.uint8, device=dev)
    d_status = torch.empty((B,), dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(dev)
    ctx.extend_commit_device(k, B, d_ods.data_ptr(), d_eds.data_ptr(), d_roots.data_ptr(), d_dah.data_ptr(),
                             d_status.data_ptr(), s.cuda_stream)
    s.synchronize()
    return d_roots.cpu().numpy(), d_dah.cpu().numpy(), d_status.cpu().numpy()


@pytest.mark.parametrize("k,B", CASES)
def test_level_kernel_path_matches_oracle(ctx, k, B):
    assert B * 4 * k > 512  # past trees_lds_kernel's bound: the level kernels run
    w = 2 * k
    ods = _batch(k, B)
    roots, dah, status = _run(ctx, ods)
    for b in range(B):
        rc, _, rr, cr, dah_o = O.extend_commit(ods[b], want_eds=False)
        assert rc == 0
        assert np.array_equal(roots[b, :w, :90], rr), (k, b, "row roots")
        assert np.array_equal(roots[b, w:, :90], cr), (k, b, "column roots")
        assert not roots[b, :, 90:].any(), (k, b, "record padding")
        assert dah[b].tobytes() == dah_o, (k, b, "dah")
        assert status[b] == CLEAN, (k, b, hex(int(status[b])))


def test_out_of_order_namespace_status_matches_oracle(ctx):
    """One block of the batch has a namespace out of push order: its status word names the first violation (axis 0,
    row 1, leaf 3), as the oracle rejects exactly that block; the roots of the other blocks are unaffected."""
    k, B = 16, 9
    w = 2 * k
    ods = _batch(k, B)
    bad = 4
    ods[bad, [k + 2, k + 3]] = ods[bad, [k + 3, k + 2]]  # row 1: leaves 2 and 3 swapped
    assert ods[bad, k + 2, :29].tobytes() > ods[bad, k + 3, :29].tobytes()
    roots, dah, status = _run(ctx, ods)
    for b in range(B):
        rc, _, rr, cr, dah_o = O.extend_commit(ods[b], want_eds=False)
        assert (rc == 0) == (status[b] == CLEAN), (b, rc, hex(int(status[b])))
        if b == bad:
            assert rc != 0
            # row 1's leaf 3 (key 0 << 40 | 1 << 20 | 3) precedes the column violations the swap also causes
            assert int(status[b]) == (1 << 20) | 3, hex(int(status[b]))
        else:
            assert np.array_equal(roots[b, :w, :90], rr) and np.array_equal(roots[b, w:, :90], cr), b
            assert dah[b].tobytes() == dah_o, b
