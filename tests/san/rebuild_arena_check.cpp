// rebuild_arena_check.cpp — CPU check of assemble_workspace (celestia-app_amd/csrc/rebuild.h), the layout of
// cda_samples_assemble_device's workspace, and of the index arithmetic of sample_place_rule.h, built and run under
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_rebuild.py.  No device is touched.  Like arena_check.cpp:
// the layout is measured, bound to a heap buffer of exactly the measured size, and every slot is written through the
// bound pointers the way the kernels index them -- the owner slot by sample_cell of every well-formed sample -- so a
// slot the measuring walk did not count, or a cell outside the square, is a heap overflow the sanitizer reports.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../celestia-app_amd/csrc/sample_place_rule.h"
#include "../../celestia-app_amd/csrc/rebuild.h"

using namespace cda;

static int g_fail = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      if (g_fail++ < 20) {                                   \
        fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);                        \
        fprintf(stderr, "\n");                               \
      }                                                      \
    }                                                        \
  } while (0)

static void check_layout(uint32_t k, uint32_t n) {
  AssembleArgs a{};
  a.k = k;
  a.nsamples = n;
  const size_t cells = 4 * (size_t)k * k;
  const size_t measured = workspace_bytes(a, assemble_workspace);
  const size_t want = align256((size_t)n * sizeof(cda_nmt_proof_desc)) + align256((size_t)n * CDA_NAMESPACE_SIZE) +
                      align256(n) + align256(cells * sizeof(uint32_t));
  CHECK(measured == want, "assemble_workspace(%u, %u): measured %zu, the slots need %zu", k, n, measured, want);
  if (measured == 0) return;
  uint8_t* buf = (uint8_t*)aligned_alloc(256, measured);
  if (!buf) {
    CHECK(false, "no memory for %zu bytes", measured);
    return;
  }
  Arena ar(buf);
  assemble_workspace(a, ar);
  CHECK(ar.used() == measured, "assemble_workspace(%u, %u): bound %zu, measured %zu", k, n, ar.used(), measured);
  CHECK((uint8_t*)a.nmt_descs == buf, "the first slot is not the base");
  CHECK((uint8_t*)a.nmt_ns == buf + align256((size_t)n * sizeof(cda_nmt_proof_desc)), "nmt_ns is out of place");
  CHECK((uint8_t*)(a.owner + cells) <= buf + measured, "owner ends beyond the workspace");
  memset(a.owner, 0xFF, cells * sizeof(uint32_t));
  // what prep and claim write, for samples that walk the border of the square and step over it
  const uint32_t w = 2 * k;
  const uint32_t at[] = {0, 1, k - 1, k, w - 1, w, w + 1, 0x7FFFFFFFu, 0xFFFFFFFFu};
  uint8_t share[CDA_SHARE];
  memset(share, 0x5A, sizeof share);
  uint32_t p = 0;
  for (uint32_t axis = 0; axis < 3 && p < n; axis++)
    for (uint32_t index : at)
      for (uint32_t pos : at) {
        if (p >= n) break;
        const cda_sample_desc d{axis, index, pos, 0xFFFFFFF0u, 32};
        const bool ok = sample_well_formed(d, k);
        CHECK(ok == (axis <= 1 && index < w && pos < w), "sample_well_formed(%u, %u, %u) at k = %u", axis, index, pos, k);
        if (!ok) {
          a.nmt_descs[p] = befp_empty_desc();
        } else {
          a.nmt_descs[p] = sample_nmt_desc(d, p, k);
          CHECK(a.nmt_descs[p].root < 4 * k && a.nmt_descs[p].end == pos + 1, "sample_nmt_desc");
          sample_namespace(d, k, share, a.nmt_ns + (size_t)p * CDA_NAMESPACE_SIZE);
          CHECK(a.nmt_ns[(size_t)p * CDA_NAMESPACE_SIZE] == ((index < k && pos < k) ? 0x5A : 0xFF), "sample_namespace");
          const size_t cell = sample_cell(d, k);
          CHECK(cell == (axis ? (size_t)pos * w + index : (size_t)index * w + pos), "sample_cell");
          if (a.owner[cell] > p) a.owner[cell] = p;
        }
        a.ok[p] = ok;
        p++;
      }
  CHECK(sample_settle(3, 3, false) == CDA_SAMPLE_PLACED && sample_settle(4, 3, true) == CDA_SAMPLE_DUPLICATE &&
            sample_settle(4, 3, false) == CDA_SAMPLE_CONFLICT,
        "sample_settle");
  free(buf);
}

int main() {
  const uint32_t ks[] = {1, 2, 4, 16, 128, 512};
  const uint32_t ns[] = {0, 1, 255, 256, 257, (1u << 20) - 3};
  for (uint32_t k : ks)
    for (uint32_t n : ns) check_layout(k, n);
  if (g_fail) {
    fprintf(stderr, "rebuild_arena_check: %d failure(s)\n", g_fail);
    return 1;
  }
  printf("rebuild_arena_check: all passed\n");
  return 0;
}
