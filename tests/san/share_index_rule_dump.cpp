// share_index_rule_dump.cpp — runs the host form of celestia-app_amd/csrc/share_index_rule.h over EVERY k = 2 square
// whose four shares are drawn from an alphabet of share headers, under the threshold argv[1].  The alphabet comes from
// stdin, one header per line: 68 hex digits, bytes [0, 34) of a share.  For A headers that is A^4 squares, in the order
// of the base-A digits i0 i1 i2 i3 (share 0 first); one line each:
//   "i0 i1 i2 i3 | nseq npadding norphans first_orphan | start:nshares:seq_len:kind:version:status:ns ..."
// tests/test_blob_index.py compares the lines with cda.blob.index_host.  Host only: the header and this file, any
// C++17 compiler; built with AddressSanitizer and UBSan by the test.  Only bytes [0, 34) of a share may be read: the
// rest of every share is poisoned, and the buffer ends 34 bytes into the last share.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(p, n) ((void)(p), (void)(n))
#endif

#include "../../celestia-app_amd/csrc/share_index_rule.h"

namespace {
int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }
}  // namespace

int main(int argc, char** argv) {
  const uint32_t threshold = argc > 1 ? (uint32_t)atoi(argv[1]) : 64, k = 2, n = k * k;
  std::vector<std::vector<uint8_t>> alphabet;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    if (line.size() != 68) return 2;
    std::vector<uint8_t> h(34);
    for (size_t i = 0; i < 34; i++) {
      const int a = nibble(line[2 * i]), b = nibble(line[2 * i + 1]);
      if (a < 0 || b < 0) return 2;
      h[i] = (uint8_t)(a * 16 + b);
    }
    alphabet.push_back(h);
  }
  const size_t A = alphabet.size();
  if (A == 0) return 2;
  std::vector<uint8_t> sq((n - 1) * 512 + 34, 0xEE);
  for (uint32_t g = 0; g + 1 < n; g++) ASAN_POISON_MEMORY_REGION(sq.data() + g * 512 + 40, 512 - 40);
  std::vector<cda_sequence> recs(n);
  for (size_t c = 0; c < A * A * A * A; c++) {
    const size_t idx[4] = {c / (A * A * A), c / (A * A) % A, c / A % A, c % A};
    for (uint32_t g = 0; g < n; g++) memcpy(sq.data() + g * 512, alphabet[idx[g]].data(), 34);
    cda_square_summary sum;
    cda::share_index_host(sq.data(), (size_t)k * 512, k, threshold, n, recs.data(), &sum);
    printf("%zu %zu %zu %zu | %u %u %u %u |", idx[0], idx[1], idx[2], idx[3], sum.nseq, sum.npadding, sum.norphans,
           sum.first_orphan);
    for (uint32_t i = 0; i < sum.nseq; i++) {
      const cda_sequence& r = recs[i];
      printf(" %u:%u:%u:%u:%u:%u:", r.start, r.nshares, r.seq_len, r.kind, r.share_version, r.status);
      for (int j = 0; j < 29; j++) printf("%02x", r.ns[j]);
    }
    printf("\n");
  }
  return 0;
}
