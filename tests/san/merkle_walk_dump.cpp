// merkle_walk_dump.cpp — prints plan::merkle_walk's verdict and fold order, one line per case:
// "total index naunts reject" or "total index naunts L|R ..." (aunt 0 first; L: the aunt is hashed on the left).
// Cases: every (total, index) with total <= argv[1] (index runs one past the tree, and -1) and every aunt count from
// 0 to the path length + 1; then argv[2] pseudo-random larger totals (up to 2^62) with the path length - 1, the path
// length and the path length + 1 aunts; then the rejections by number alone (total <= 0, more than 100 aunts).
// tests/test_share_proofs.py compares the lines with cda.proof.Proof.verify on hashlib trees.  Host only: plan.cpp +
// this file, any C++17 compiler.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../celestia-app_amd/csrc/plan.h"

static void line(int64_t total, int64_t index, uint64_t naunts) {
  std::vector<uint8_t> left;
  printf("%lld %lld %llu", (long long)total, (long long)index, (unsigned long long)naunts);
  if (!cda::plan::merkle_walk(total, index, naunts, left)) {
    printf(" reject\n");
    return;
  }
  for (uint8_t l : left) printf(" %c", l ? 'L' : 'R');
  printf("\n");
}

// the path length of (total, index), by the recursion itself (not the header's loop)
static int depth_of(uint64_t total, uint64_t index) {
  if (total <= 1) return 0;
  uint64_t k = 1;
  while ((k << 1) < total) k <<= 1;
  return 1 + (index < k ? depth_of(k, index) : depth_of(total - k, index - k));
}

int main(int argc, char** argv) {
  const int64_t max_total = argc > 1 ? atoll(argv[1]) : 64;
  const int nrandom = argc > 2 ? atoi(argv[2]) : 300;
  for (int64_t total = 1; total <= max_total; total++)
    for (int64_t index = -1; index <= total; index++) {
      const int d = index >= 0 && index < total ? depth_of((uint64_t)total, (uint64_t)index) : 2;
      for (int na = 0; na <= d + 1; na++) line(total, index, (uint64_t)na);
    }
  uint64_t x = 0x9E3779B97F4A7C15ull;  // xorshift64
  auto next = [&]() {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x;
  };
  for (int i = 0; i < nrandom; i++) {
    const uint64_t total = (next() >> (2 + next() % 56)) + 65, index = next() % total;
    const int d = depth_of(total, index);
    for (int na = d - 1; na <= d + 1; na++) line((int64_t)total, (int64_t)index, (uint64_t)na);
  }
  line(0, 0, 0);
  line(-4, 0, 2);
  line(INT64_MIN, 0, 0);
  line(INT64_MAX, INT64_MAX - 1, 62);
  line(INT64_MAX, INT64_MAX - 1, 63);
  line(8, 3, 101);
  line(8, 3, 1000000);
  return 0;
}
