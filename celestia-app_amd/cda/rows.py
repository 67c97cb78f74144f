"""Halves of rows and columns: serve them from a retained square, verify batches, rebuild a square from them.

celestia-node's shwap.Row is half of an axis -- k consecutive cells, either cells [0, k) or cells [k, 2k) -- sent with
no proof at all.  The receiver checks it (Row.Verify) by completing the axis with the codec, building the wrapper tree
over the 2k cells and comparing its root with the one in the header.  Rows are also what a reconstructing full node
pulls when it wants whole axes and not single cells: 512 k bytes and no proof node, against k samples of log2(2k)
nodes each.  Row.Verify lives in celestia-node, outside the pinned tree, so the rule below (H0-H2) is this
project's statement of it; the codec, the wrapper tree's quadrant rule and the roots it rests on are pinned.  rsmt2d
has no assemble step, so the placement rule is this library's, as cda.sampling.assemble_host's is.

    halves_of(square, queries)                  the producer: Square.axis_halves as AxisHalf records
    verify_host(halves, rows, cols, codec)      H0-H2 on the host, the mirror the device form is tested against
    verify(ctx, halves, rows, cols)             cda_axis_halves_verify: the whole batch in one call
    assemble_host(halves, rows, cols, codec)    verification and the placement rule on the host
    rebuild(ctx, halves, rows, cols)            cda_square_rebuild_axes: verified, placed, repaired, retained

The rule.  A half covers cells [side k, side k + k) of row `index` (axis 0) or column `index` (axis 1); the roots of
its block are roots[root_off, root_off + 4k), the 2k row roots then the 2k column roots.  The first check that applies
decides:
    H0 MALFORMED  axis > 1, index >= 2k, side > 1 or root_off + 4k > nroots
    H1            side 0: cells [k, 2k) := Encode(cells [0, k)); side 1: cells [0, k) := Decode with exactly the
                  cells [k, 2k) present
    H2 BAD_ROOT   the wrapper tree (squareSize k, axisIndex index) over the 2k cells cannot be built (push order), or
                  its root is not roots[root_off + axis 2k + index]; otherwise VERIFIED (= PLACED)
Placement, all halves belonging to one square (root_off 0): among verified halves the lowest-indexed half of an axis
is that axis's half and a later one -- the other side included -- is DUPLICATE; the owner of a cell is the
lowest-indexed such half whose axis contains it, and an owner's whole completed axis is placed; a half whose bytes
differ from the owner's at a cell it does not own is CONFLICT (and still places the cells it owns), else PLACED.
"""
from dataclasses import dataclass

import numpy as np

from . import _native as N
from .wrapper import ErasuredNamespacedMerkleTree, PushError

PLACED, DUPLICATE, CONFLICT, BAD_ROOT, MALFORMED = (N.HALF_PLACED, N.HALF_DUPLICATE, N.HALF_CONFLICT, N.HALF_BAD_ROOT,
                                                    N.HALF_MALFORMED)
VERIFIED = PLACED
ROW, COL = N.AXIS_ROW, N.AXIS_COL
FIRST, SECOND = N.SIDE_FIRST, N.SIDE_SECOND


@dataclass
class AxisHalf:
    """Cells [side k, side k + k) of row (axis 0) or column (axis 1) `index`: `shares`, k cells of 512 bytes in cell
    order.  root_off: where its block's 4k roots start in the roots of a verify call."""
    axis: int
    index: int
    side: int
    shares: object
    root_off: int = 0

    def cells(self):
        return [bytes(x) for x in self.shares]


def halves_of(square, queries):
    """The halves `queries` ((axis, index, side) tuples) of an open Square, one launch.  -> list of AxisHalf."""
    queries = [(int(a), int(i), int(s)) for a, i, s in queries]
    if not queries:
        return []
    shares = square.axis_halves(queries)
    return [AxisHalf(a, i, s, shares[n]) for n, (a, i, s) in enumerate(queries)]


def pack(halves, k, root_off=0):
    """The arrays cda_axis_halves_verify takes for `halves` of 2k x 2k squares: (descs, shares (n, k, 512)); root_off
    is added to every half's own."""
    descs = np.zeros(len(halves), N.AXIS_HALF_DESC_DTYPE)
    shares = np.zeros((len(halves), k, N.SHARE_SIZE), np.uint8)
    for p, h in enumerate(halves):
        cells = h.cells()
        if len(cells) != k or any(len(c) != N.SHARE_SIZE for c in cells):
            raise ValueError("a half is k cells of 512 bytes")
        descs[p] = tuple(v & 0xFFFFFFFF for v in (h.axis, h.index, h.side, h.root_off + root_off))
        shares[p] = np.frombuffer(b"".join(cells), np.uint8).reshape(k, N.SHARE_SIZE)
    return descs, shares


def pack_roots(row_roots, col_roots):
    """(4k, 90) uint8: the row roots then the column roots."""
    return np.concatenate([np.ascontiguousarray(row_roots, np.uint8).reshape(-1, N.NODE_SIZE),
                           np.ascontiguousarray(col_roots, np.uint8).reshape(-1, N.NODE_SIZE)])


def _axis_root(codec, k, index, cells):
    """The wrapper tree's 90-byte root over the 2k cells, or None when the tree cannot be built."""
    if hasattr(codec, "axis_root"):
        return codec.axis_root(k, index, cells)
    tree = ErasuredNamespacedMerkleTree(k, index)
    try:
        for cell in cells:
            tree.push(cell)
    except PushError:
        return None
    return tree._root_node()


def complete_host(half, k, codec):
    """H1: the 2k cells of the half's axis."""
    cells = half.cells()
    if half.side == FIRST:
        return cells + [bytes(x) for x in codec.encode(cells)]
    return [bytes(x) for x in codec.decode([None] * k + cells)][:k] + cells


def verify_host(halves, row_roots, col_roots, codec):
    """H0-H2 of every half against one block's 2k row roots and 2k column roots (root_off + 4k <= 4k: a root_off
    other than 0 is MALFORMED), on the host.  codec: encode(k shards) -> k parity shards, decode(2k shards or None) ->
    2k shards, and optionally axis_root(k, index, 2k cells) -> 90-byte root or None (default: cda.wrapper's tree).
    -> (statuses (n,) uint8: PLACED for verified, BAD_ROOT or MALFORMED; axes (n, 2k, 512) uint8, the completed axes,
    zero for a malformed half)."""
    w = len(row_roots)
    k = w // 2
    statuses = np.zeros(len(halves), np.uint8)
    axes = np.zeros((len(halves), w, N.SHARE_SIZE), np.uint8)
    for p, h in enumerate(halves):
        if h.axis not in (ROW, COL) or not 0 <= h.index < w or h.side not in (FIRST, SECOND) or h.root_off != 0 or \
                len(col_roots) != w:
            statuses[p] = MALFORMED
            continue
        cells = complete_host(h, k, codec)
        axes[p] = np.frombuffer(b"".join(cells), np.uint8).reshape(w, N.SHARE_SIZE)
        committed = bytes(row_roots[h.index]) if h.axis == ROW else bytes(col_roots[h.index])
        statuses[p] = VERIFIED if _axis_root(codec, k, h.index, cells) == committed else BAD_ROOT
    return statuses, axes


def verify(ctx, halves, row_roots, col_roots, want_axes=False):
    """cda_axis_halves_verify of `halves` against one block's roots, one call.  -> statuses (n,) uint8[, axes
    (n, 2k, 512)]."""
    k = len(row_roots) // 2
    descs, shares = pack(halves, k)
    return ctx.axis_halves_verify(k, descs, shares, pack_roots(row_roots, col_roots), want_axes)


def assemble_host(halves, row_roots, col_roots, codec):
    """Verification and the placement rule (csrc/axis_half_rule.h) on the host, the mirror
    cda_axis_halves_assemble_device is tested against.  -> (eds ((2k)^2, 512) uint8, zero where nothing is placed;
    present ((2k)^2,) uint8; statuses (n,) uint8)."""
    w = len(row_roots)
    statuses, axes = verify_host(halves, row_roots, col_roots, codec)
    eds = np.zeros((w * w, N.SHARE_SIZE), np.uint8)
    present = np.zeros(w * w, np.uint8)
    axis_half = {}  # (axis, index) -> its lowest-indexed verified half
    for p, h in enumerate(halves):
        if statuses[p] == VERIFIED:
            axis_half.setdefault((h.axis, h.index), p)
    for p, h in enumerate(halves):
        if statuses[p] != VERIFIED:
            continue
        if axis_half[(h.axis, h.index)] != p:
            statuses[p] = DUPLICATE
            continue
        for pos in range(w):
            cell = h.index * w + pos if h.axis == ROW else pos * w + h.index
            other = axis_half.get((1 - h.axis, pos))
            if other is None or p < other:
                eds[cell] = axes[p, pos]
                present[cell] = 1
            elif not np.array_equal(axes[p, pos], axes[other, h.index]):
                statuses[p] = CONFLICT
    return eds, present, statuses


def rebuild(ctx, halves, row_roots, col_roots, want_eds=False):
    """cda_square_rebuild_axes over `halves`: verified, placed, repaired against the roots (rsmt2d Repair) and
    retained, without the square leaving the device.  -> (Square, statuses, present[, eds]).  When Repair fails
    CdaError carries the code (E_UNREPAIRABLE, E_BYZANTINE with axis and index) and, as attributes, statuses, present
    and eds."""
    k = len(row_roots) // 2
    descs, shares = pack(halves, k)
    rc, sq, statuses, present, eds, err = ctx.square_rebuild_axes(descs, shares, row_roots, col_roots, want_eds)
    if rc != N.OK:
        e = N.CdaError(rc, axis=err.axis, index=err.index)
        e.statuses, e.present, e.eds = statuses, present, eds
        raise e
    return (sq, statuses, present, eds) if want_eds else (sq, statuses, present)
