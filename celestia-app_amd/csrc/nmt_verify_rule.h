// nmt_verify_rule.h — nmt Proof.VerifyInclusion's node schedule by index arithmetic, shared by the verify kernels
// (sampling_kernels.hip) and the host planner plan::verify_walk (plan.cpp, which builds with a plain C++ compiler).
//
// VerifyInclusion recomputes the root of the subtree of top = 2 * splitpoint(end) leaves recursively, popping the
// proof's nodes left to right, then applies the nodes left over as right siblings.  The same pairs, without a stack:
//   - the first popcount(start) nodes are the left hull of [start, end), widest first: going up from the leaves, the
//     span [lo, hi) of a level takes the last unused one in front whenever lo is odd;
//   - the nodes after them come in order: the span takes the next one behind whenever hi is odd, and where none is
//     left its odd last node goes up unchanged (a tree whose leaf count is no power of two);
//   - after log2(top) levels the span is one node; every node still unused is applied above it.
// A proof with fewer than popcount(start) nodes is rejected.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CDA_HD __host__ __device__ __forceinline__
#else
#define CDA_HD inline
#endif

namespace cda {

// the widest axis the codec accepts (cda_rs_max_chunks = 32768^2: 2k = 65536): no proof ends beyond it
constexpr uint32_t kVerifyMaxEnd = 65536;

struct VerifyWalk {
  uint32_t lo, hi;  // the span of the current level, in nodes of that level
  uint32_t lp, rp;  // left hull nodes still unused: [0, lp); next node behind the span: rp
  uint32_t nnodes;
  int levels;       // log2(2 * splitpoint(end)): levels below the subtree root

  static CDA_HD uint32_t popcount(uint32_t v) {
    uint32_t n = 0;
    for (; v; v &= v - 1) n++;
    return n;
  }
  // false: the proof is rejected by its node count alone
  CDA_HD bool init(uint32_t start, uint32_t end, uint32_t nn) {
    lo = start;
    hi = end;
    nnodes = nn;
    lp = rp = popcount(start);
    levels = 0;
    while ((1u << levels) < end) levels++;  // 2 * splitpoint(end) = the next power of two >= end (1 for end = 1)
    return nn >= lp;
  }
  // One level: left / right = the node put in front of / behind the span (-1: none); afterwards [lo, hi) is the span
  // these extend it to, whose nodes pair up from lo (an odd last one goes up unchanged).  Then call up().
  CDA_HD void step(int& left, int& right) {
    left = right = -1;
    if (lo & 1) {
      left = (int)--lp;
      lo--;
    }
    if ((hi & 1) && rp < nnodes) {
      right = (int)rp++;
      hi++;
    }
  }
  CDA_HD void up() {
    lo >>= 1;
    hi = (hi + 1) >> 1;
  }
};

}  // namespace cda
