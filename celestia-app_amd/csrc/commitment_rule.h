// commitment_rule.h — the rule of a blob commitment proof: which inner nodes of the row trees are a blob's
// subtree roots, and how a row's subtree roots and the nodes of its range proof fold to the row root.  Shared by the
// prover and verifier kernels (sampling_kernels.hip), the host calls (commitment.cpp) and the stand-alone programs of
// tests/san, which build it with a plain C++ compiler.
//
// Tiles.  A row's range [s, e), 0 <= s < e <= k, under subtree width W (a power of two) is tiled greedily from the
// left: at cursor c the tile is the largest power of two z <= W with c % z == 0 and c + z <= e.  The tile of size 2^h
// at c is node (h, c >> h) of the row tree.  A blob of `len` shares has W = SubTreeWidth(len, threshold) (go-square
// inclusion.SubTreeWidth) and starts at a multiple of W (NextShareIndex), so s % W == 0 in every row: the tiles are
// (e - s) / W tiles of size W and then one tile per set bit of (e - s) % W, widest first.
//
// Fold of one row (SubtreeWalk): nmt_verify_rule.h's walk started above the leaves.  The proof's nodes are
// ProveRange(s, e) of the 2k-leaf row tree: popcount(s) left hull nodes, widest first, then popcount(2k - e) nodes
// behind the range, in order.  Going up from level 0, the root of a tile of size 2^h joins the span at level h:
//   - below log2 W only the tail's tiles exist.  The first of them starts the span as one node; a later one comes in
//     front of the running node (its position lo is odd exactly when bit h of (e - s) % W is set), so after it has
//     joined lo is even and no left hull node is taken down here;
//   - at log2 W the W-sized roots enter in front of the running node;
//   - wherever the span is not empty VerifyWalk::step and up apply as they stand.
// After log2(2k) levels the span is node 0 and every proof node is used.  A row is accepted by its counts alone only
// if it has exactly the tiles' number of roots and popcount(s) + popcount(2k - e) nodes: then no step finds a node
// missing and none is left over.
#pragma once
#include <stdint.h>

#include "nmt_verify_rule.h"

namespace cda {

constexpr uint32_t kCommitMaxK = 32768;         // the widest ODS the codec accepts (nmt_verify_rule.h kVerifyMaxEnd / 2)
constexpr uint32_t kCommitMaxRoots = 1u << 18;  // subtree roots of one proof the commitment kernel folds (512 x 512)

// go-square inclusion.SubTreeWidth(len, threshold) for len, threshold > 0:
// min(RoundUpPowerOfTwo(ceil(len / threshold)), BlobMinSquareSize(len)); a power of two m has m >= ceil(sqrt(len))
// exactly when m * m >= len
CDA_HD uint32_t sub_tree_width(uint64_t len, uint32_t threshold) {
  const uint64_t s = (len + threshold - 1) / threshold;
  uint64_t a = 1, b = 1;
  while (a < s) a <<= 1;
  while (b * b < len) b <<= 1;
  return (uint32_t)(a < b ? a : b);
}

// the tile at cursor c of a range that ends at e
CDA_HD uint32_t subtree_tile(uint32_t c, uint32_t e, uint32_t W) {
  uint32_t z = W;
  while (z > 1 && ((c & (z - 1)) || c + z > e)) z >>= 1;
  return z;
}
// the number of tiles of [s, e) with s % W == 0
CDA_HD uint32_t subtree_tile_count(uint32_t s, uint32_t e, uint32_t W) {
  return (e - s) / W + VerifyWalk::popcount((e - s) & (W - 1));
}
// the proof nodes of ProveRange(s, e) of a perfect tree of `leaves` leaves
CDA_HD uint32_t range_proof_nodes(uint32_t s, uint32_t e, uint32_t leaves) {
  return VerifyWalk::popcount(s) + VerifyWalk::popcount(leaves - e);
}

struct SubtreeWalk {
  VerifyWalk w;   // the span, the unused left hull nodes and the next node behind, as in VerifyInclusion's walk
  uint32_t s, e;  // the row's leaf range
  uint32_t rem;   // (e - s) % W: the tail's tiles
  uint32_t nfull; // (e - s) / W
  uint32_t nroots;
  int hw, top;    // log2 W, log2(2k)
  bool live;      // the span is not empty

  // s % W == 0, 0 <= s < e <= k, W <= k, W and k powers of two.  false: rejected by the counts alone.
  CDA_HD bool init(uint32_t start, uint32_t end, uint32_t W, uint32_t k, uint32_t nr, uint32_t nn) {
    s = start;
    e = end;
    rem = (end - start) & (W - 1);
    nfull = (end - start) / W;
    nroots = nr;
    hw = top = 0;
    while ((1u << hw) < W) hw++;
    while ((1u << top) < 2 * k) top++;
    live = false;
    w.lo = w.hi = 0;
    w.nnodes = nn;
    w.lp = w.rp = VerifyWalk::popcount(start);
    w.levels = top;
    return nr == subtree_tile_count(start, end, W) && nn == range_proof_nodes(start, end, 2 * k);
  }
  // Level h, before VerifyWalk::step: roots [first, first + count) join the span, the first of them as node `at` of
  // level h (count = 0: none).  Call for h = 0 .. top - 1, each followed by w.step and w.up() if `live`.
  CDA_HD void enter(int h, uint32_t& first, uint32_t& count, uint32_t& at) {
    first = count = at = 0;
    if (h < hw) {
      if (!((rem >> h) & 1)) return;
      first = nroots - 1 - VerifyWalk::popcount(rem & ((1u << h) - 1));  // the tail descends: its smallest tile is last
      count = 1;
      at = live ? w.lo - 1 : (e >> h) - 1;
      if (!live) w.hi = at + 1;
      w.lo = at;
      live = true;
    } else if (h == hw && nfull) {
      count = nfull;
      at = s >> hw;
      if (!live) w.hi = at + nfull;
      w.lo = at;
      live = true;
    }
  }
};

}  // namespace cda
