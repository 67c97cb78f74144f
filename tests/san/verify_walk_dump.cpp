// verify_walk_dump.cpp — prints plan::verify_walk's schedule for every range [start, end) with end <= argv[1] and
// every node count 0..13, one line each: "start end nnodes level:lo:hi:left:right ... tail T" or "... reject".
// tests/test_sampling.py compares the lines with the rule restated in Python (itself fuzzed against
// NMTProof.verify_inclusion).  Host only: plan.cpp + this file, any C++17 compiler.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../celestia-app_amd/csrc/plan.h"

int main(int argc, char** argv) {
  const unsigned max_end = argc > 1 ? (unsigned)atoi(argv[1]) : 64;
  std::vector<cda::plan::VerifyStep> steps;
  for (unsigned end = 1; end <= max_end; end++)
    for (unsigned start = 0; start < end; start++)
      for (unsigned nn = 0; nn < 14; nn++) {
        uint32_t tail = 0;
        printf("%u %u %u", start, end, nn);
        if (!cda::plan::verify_walk(start, end, nn, steps, &tail)) {
          printf(" reject\n");
          continue;
        }
        printf(" ");
        for (size_t i = 0; i < steps.size(); i++)
          printf("%s%d:%u:%u:%d:%d", i ? " " : "", steps[i].level, steps[i].lo, steps[i].hi, steps[i].left,
                 steps[i].right);
        printf(" tail %u\n", tail);
      }
  return 0;
}
