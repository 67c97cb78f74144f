// commitment_walk_dump.cpp — prints SubtreeWalk's schedule (celestia-app_amd/csrc/commitment_rule.h) for every
// (k <= argv[1], W <= k, s, e) with s % W == 0 and 0 <= s < e <= k, one line each:
//   "k W s e | R<j>@<level>:<node> ... | N<i>@<level>:<node> ... | end <lo>:<hi>:<lp>:<rp>"
// R: subtree root j of the row enters as that node of that level; N: node i of ProveRange(s, e) of the 2k-leaf tree
// does.  The tiles themselves come first on the line as "T<size>@<cursor>".  tests/test_commitment_proofs.py compares
// the lines with the recursion of cda/commitment.py.  Host only: the header and this file, any C++17 compiler.
#include <cstdio>
#include <cstdlib>

#include "../../celestia-app_amd/csrc/commitment_rule.h"

int main(int argc, char** argv) {
  const unsigned max_k = argc > 1 ? (unsigned)atoi(argv[1]) : 64;
  for (unsigned k = 1; k <= max_k; k <<= 1)
    for (unsigned W = 1; W <= k; W <<= 1)
      for (unsigned s = 0; s < k; s += W)
        for (unsigned e = s + 1; e <= k; e++) {
          printf("%u %u %u %u |", k, W, s, e);
          unsigned nroots = 0;
          for (unsigned c = s; c < e; nroots++) {
            const unsigned z = cda::subtree_tile(c, e, W);
            printf(" T%u@%u", z, c);
            c += z;
          }
          const unsigned nn = cda::range_proof_nodes(s, e, 2 * k);
          cda::SubtreeWalk sw;
          if (!sw.init(s, e, W, k, nroots, nn)) {
            printf(" | reject\n");
            continue;
          }
          printf(" |");
          char nodes[4096];
          size_t at_n = 0;
          nodes[0] = 0;
          for (int h = 0; h < sw.top; h++) {
            uint32_t first, count, at;
            sw.enter(h, first, count, at);
            for (uint32_t j = 0; j < count; j++) printf(" R%u@%d:%u", first + j, h, at + j);
            if (!sw.live) continue;
            int left, right;
            sw.w.step(left, right);
            if (left >= 0) at_n += (size_t)snprintf(nodes + at_n, sizeof nodes - at_n, " N%d@%d:%u", left, h, sw.w.lo);
            if (right >= 0)
              at_n += (size_t)snprintf(nodes + at_n, sizeof nodes - at_n, " N%d@%d:%u", right, h, sw.w.hi - 1);
            if (at_n >= sizeof nodes) return 2;
            sw.w.up();
          }
          printf(" |%s | end %u:%u:%u:%u\n", nodes, sw.w.lo, sw.w.hi, sw.w.lp, sw.w.rp);
        }
  return 0;
}
