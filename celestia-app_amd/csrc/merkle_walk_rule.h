// merkle_walk_rule.h — go-square merkle Proof.Verify's path (computeHashFromAunts) without recursion, shared by the
// row-proof kernel (sampling_kernels.hip) and the host planner plan::merkle_walk (plan.cpp, which builds with a plain
// C++ compiler).
//
// computeHashFromAunts(index, total, leafHash, aunts) splits a tree of `total` leaves at the largest power of two
// below total, descends into the half that holds `index` with all aunts but the last, and hashes the result with the
// last aunt on the other side.  The same, walked twice:
//   - top-down from (index, total) to the leaf: one left / right decision per level, kept as one bit each (a tree of
//     up to 2^63 leaves is at most 63 levels deep: going right at least halves the leaves, going left leaves a power
//     of two that halves from then on);
//   - bottom-up over the aunts: aunt j (0 = the leaf's sibling) pairs with the running hash on the side the decision
//     of level depth - 1 - j says.
// The proof is rejected by its numbers alone when index < 0, total <= 0, index >= total, there are more than
// kMerkleMaxAunts aunts, or the aunt count is not the depth of the leaf (the recursion runs out of aunts, or has
// some left at the leaf).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CDA_MW_HD __host__ __device__ __forceinline__
#else
#define CDA_MW_HD inline
#endif

namespace cda {

constexpr uint32_t kMerkleMaxAunts = 100;  // go-square merkle proof.go MaxAunts

struct MerkleWalk {
  uint64_t dirs;  // bit j: the running hash is the RIGHT child when aunt j is applied (the aunt goes on the left)
  int depth;      // levels between the leaf and the root = aunts a valid proof carries

  // false: Proof.Verify fails whatever the hashes are
  CDA_MW_HD bool init(int64_t total, int64_t index, uint64_t naunts) {
    dirs = 0;
    depth = 0;
    if (index < 0 || total <= 0 || index >= total || naunts > kMerkleMaxAunts) return false;
    uint64_t n = (uint64_t)total, i = (uint64_t)index;
    uint64_t k = 1;  // the split point of n: the largest power of two below it (0 for n = 1)
    while ((k << 1) < n) k <<= 1;
    if (n == 1) k = 0;
    while (n > 1) {
      uint64_t right = 0;
      if (i < k) {
        n = k;
      } else {
        i -= k;
        n -= k;
        right = 1;
      }
      dirs = (dirs << 1) | right;
      depth++;
      while (k >= n && k) k >>= 1;
    }
    return naunts == (uint64_t)depth;
  }
  CDA_MW_HD bool aunt_on_left(int j) const { return (dirs >> j) & 1; }
};

}  // namespace cda
