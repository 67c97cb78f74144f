"""Level 1 of the batched tree path by 2x2 cell quads (nmt_level1_quads_kernel, then level 2 from one
nmt_levels_kernel launch), at the smallest batches that leave trees_lds_kernel (nblocks * 4k > 512) for each wave shape:

  (1, 129)           L = 1: no quads, the one nmt_levels_kernel launch as before
  (2, 65)            L = 2: quads, then level 2 is the root level
  (4, 33), (16, 9)   a wave spans several quad-rows and both halves: the general form on parity quads
  (64, 3)            one quad-row per wave, half Q0 and half parity: a mixed wave
  (128, 2)           wave-uniform: the parity form and the general form each on whole waves
  (256, 1)           L = 9: the launch split 1, 1, 2, 2, 3

Every block is one of three kinds: a namespace-sorted random square; three long runs of equal namespaces (min == max
nodes, range-merging nodes at the Q0 / parity boundary); one namespace over the whole of Q0.  A batch of fewer than
three blocks cannot hold the three, so those cases run as many batches as it takes.  Every row root, column root,
record padding, DAH and status word is compared with the CPU oracle (tests/oracle_lib.py): a wrong or misplaced
level-1 record changes a root.  The (16, 9) and (128, 2) batches also go through the test-hooks library opened with
CDA_L1_QUADS=0 (levels 1-2 in one nmt_levels_kernel launch), whose outputs must be the same bytes."""
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

CASES = [(1, 129), (2, 65), (4, 33), (16, 9), (64, 3), (128, 2), (256, 1)]
AB_CASES = [(16, 9), (128, 2)]
CLEAN = np.int64(-1)  # the status word of a block whose namespaces are in push order


def _equal_ns_block(k, seed):
    """A namespace-sorted ODS of three long runs of equal namespaces (inner nodes with min == max, nodes whose two
    children carry different ranges, and the Q0 / parity boundary at every level)."""
    ods = O.gen_ods(k, seed).copy()
    run = (np.arange(k * k) * 3) // (k * k)  # row-major non-decreasing: every row and column is sorted
    ods[:, 19:29] = 0
    ods[:, 28] = 0x10 + run
    return ods


def _single_ns_block(k, seed):
    """An ODS whose whole Q0 carries one namespace: every Q0 node has min == max, also across the quad boundary."""
    ods = O.gen_ods(k, seed).copy()
    ods[:, :29] = ods[0, :29]
    return ods


def _batches(k, B):
    """Batches of B blocks that between them hold the three kinds (one batch when B >= 3)."""
    kinds = ["random"] * max(B - 2, 1) + ["equal", "single"]
    kinds += ["random"] * (-len(kinds) % B)
    blocks = []
    for n, kind in enumerate(kinds):
        if kind == "equal":
            blocks.append(_equal_ns_block(k, 0xE0 + k))
        elif kind == "single":
            blocks.append(_single_ns_block(k, 0x51 + k))
        else:
            blocks.append(O.gen_ods(k, 0x7A11 + 131 * k + n))
    return [np.stack(blocks[i:i + B]) for i in range(0, len(blocks), B)]


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


@pytest.fixture(scope="module")
def old_levels_ctx():
    """A context of the test-hooks library with levels 1-2 in one nmt_levels_kernel launch (CDA_L1_QUADS=0 at
    cda_init; the release library has no such switch)."""
    import cda
    from cda import _native as N
    if not os.path.exists(N.HOOKS_LIB_PATH):
        pytest.skip("the test-hooks library is not built")
    old = os.environ.get("CDA_L1_QUADS")
    os.environ["CDA_L1_QUADS"] = "0"
    try:
        c = cda.Context(0, lib_path=N.HOOKS_LIB_PATH)
    finally:
        if old is None:
            del os.environ["CDA_L1_QUADS"]
        else:
            os.environ["CDA_L1_QUADS"] = old
    yield c
    c.close()


@pytest.mark.parametrize("k,B", CASES)
def test_quads_path_matches_oracle(ctx, k, B):
    assert B * 4 * k > 512  # past trees_lds_kernel's bound: the level kernels run
    assert (B - 1) * 4 * k <= 512  # and the smallest such batch
    w = 2 * k
    for n, ods in enumerate(_batches(k, B)):
        roots, dah, status = _run(ctx, ods)
        for b in range(B):
            rc, _, rr, cr, dah_o = O.extend_commit(ods[b], want_eds=False)
            assert rc == 0
            assert np.array_equal(roots[b, :w, :90], rr), (k, n, b, "row roots")
            assert np.array_equal(roots[b, w:, :90], cr), (k, n, b, "column roots")
            assert not roots[b, :, 90:].any(), (k, n, b, "record padding")
            assert dah[b].tobytes() == dah_o, (k, n, b, "dah")
            assert status[b] == CLEAN, (k, n, b, hex(int(status[b])))


@pytest.mark.parametrize("k,B", AB_CASES)
def test_quads_and_one_launch_levels_agree(ctx, old_levels_ctx, k, B):
    for n, ods in enumerate(_batches(k, B)):
        new, old = _run(ctx, ods), _run(old_levels_ctx, ods)
        for x, y, what in zip(new, old, ("roots", "dah", "status")):
            assert x.tobytes() == y.tobytes(), (k, n, what)
