// mixed_route_dump.cpp — prints what csrc/mixed_route.h (plain C++, no HIP) decides for one mixed-size call; a
// stand-alone host program that tests/test_mixed_batch.py builds with the plain C++ compiler and runs.
//
//   mixed_route_dump <small_max> <k0> <k1> ...
//     check <code> <bad>        mixed_check_ks against the device limit 512 (0 ok, 1 not a power of two, 2 too large)
//     ods / eds / roots <n + 1 offsets>
//     small <blocks>            the fused kernel's blocks, in input order
//     desc <log2k> <block> <ods_off> <eds_off> <rec_off>     one line per small block
//     lds <kmax> <bytes>        the fused launch's dynamic LDS
//     group <k> : <blocks>      host form, one line per group
//     run <k> <first> <count>   device form, one line per run
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../celestia-app_amd/csrc/mixed_route.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const uint32_t small_max = (uint32_t)strtoul(argv[1], nullptr, 10);
  std::vector<uint32_t> ks;
  for (int i = 2; i < argc; i++) ks.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
  const uint32_t n = (uint32_t)ks.size();
  uint32_t bad = 0;
  const int chk = cda::mixed_check_ks(ks.data(), n, 512, &bad);
  printf("check %d %u\n", chk, chk ? bad : 0u);
  if (chk) return 0;
  const cda::MixedOffsets off = cda::mixed_offsets(ks.data(), n);
  auto line = [](const char* name, const std::vector<uint64_t>& v) {
    printf("%s", name);
    for (uint64_t x : v) printf(" %llu", (unsigned long long)x);
    printf("\n");
  };
  line("ods", off.ods);
  line("eds", off.eds);
  line("roots", off.roots);
  const std::vector<uint32_t> small = cda::mixed_small_blocks(ks.data(), n, small_max);
  printf("small");
  for (uint32_t b : small) printf(" %u", b);
  printf("\n");
  uint32_t kmax = 0;
  for (const cda::SmallSquareDesc& d : cda::small_square_descs(ks.data(), small, off, &kmax))
    printf("desc %u %u %llu %llu %llu\n", d.log2k, d.block, (unsigned long long)d.ods_off,
           (unsigned long long)d.eds_off, (unsigned long long)d.rec_off);
  if (kmax) printf("lds %u %zu\n", kmax, cda::small_square_lds_bytes(kmax));
  for (const cda::MixedGroup& g : cda::mixed_groups(ks.data(), n, small_max)) {
    printf("group %u :", g.k);
    for (uint32_t b : g.blocks) printf(" %u", b);
    printf("\n");
  }
  for (const cda::MixedRun& r : cda::mixed_runs(ks.data(), n, small_max)) printf("run %u %u %u\n", r.k, r.first, r.count);
  return 0;
}
