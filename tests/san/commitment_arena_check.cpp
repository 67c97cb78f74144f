// commitment_arena_check.cpp — CPU check of commit_verify_workspace (celestia-app_amd/csrc/commitment.h), the layout
// of cda_commitment_proofs_verify's workspace, built and run under AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_commitment_proofs.py.  No device is touched.  Like arena_check.cpp: the layout is measured, bound to a
// heap buffer of exactly the measured size, and every slot is written through the bound pointers over its whole
// extent, the way the kernels index it (per proof, per row record) -- so a slot the measuring walk did not count is a
// heap overflow the sanitizer reports.  The memset the launch clears the workspace with (from `pre`, the measured
// size) is made here too.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../celestia-app_amd/csrc/commitment_rule.h"
#include "../../celestia-app_amd/csrc/commitment.h"

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

static void check_layout(uint32_t nproofs, uint32_t nrows) {
  CommitVerifyArgs a{};
  a.nproofs = nproofs;
  a.nrows = nrows;
  const size_t p = nproofs, n = nrows;
  const size_t measured = workspace_bytes(a, commit_verify_workspace);
  const size_t want = align256(p * 4) + align256(p * sizeof(CommitSet)) + align256(p * 32) + align256(p * 4) +
                      align256(p * sizeof(cda_share_proof_desc)) + 4 * align256(n * 4) +
                      align256(n * sizeof(cda_share_row)) + 3 * align256(n);
  CHECK(measured == want, "commit_verify_workspace(%u, %u): measured %zu, the slots need %zu", nproofs, nrows, measured,
        want);
  if (measured == 0) return;
  uint8_t* buf = (uint8_t*)aligned_alloc(256, measured);
  if (!buf) {
    CHECK(false, "no memory for %zu bytes", measured);
    return;
  }
  Arena ar(buf);
  commit_verify_workspace(a, ar);
  CHECK(ar.used() == measured, "commit_verify_workspace(%u, %u): bound %zu, measured %zu", nproofs, nrows, ar.used(),
        measured);
  CHECK((uint8_t*)a.pre == buf, "pre is not the first slot: the launch's memset starts there");
  memset(a.pre, 0, measured);
  if (n) memset(a.owner, 0xFF, n * 4);
  for (size_t i = 0; i < p; i++) {
    a.pre[i] = CDA_CP_COMMITMENT;
    a.sets[i] = CommitSet{(uint32_t)i, 1u, kCommitMaxRoots, 1u};
    for (int t = 0; t < 8; t++) a.got[i * 8 + t] = 0xA5A5A5A5u;
    a.got_ok[i] = 1;
    a.sp_descs[i].data_root = (uint32_t)i;
    a.sp_descs[i].pad_[2] = 1;
  }
  for (size_t r = 0; r < n; r++) {
    CHECK(a.owner[r] == ~0u, "owner[%zu] was not cleared to none", r);
    a.owner[r] = (uint32_t)r;
    a.claims[r]++;
    a.root_base[r] = (uint32_t)r;
    a.row_w[r] = kCommitMaxK;
    a.sp_rows[r].total = 4 * (int64_t)kCommitMaxK;
    a.sp_rows[r].pad_ = 1;
    a.ns_ok[r] = a.row_ok[r] = a.fold_ok[r] = 1;
  }
  CHECK(n == 0 || (uint8_t*)(a.fold_ok + n) <= buf + measured, "fold_ok ends beyond the workspace");
  free(buf);
}

int main() {
  const uint32_t ps[] = {0, 1, 31, 33, 257, 4096};
  const uint32_t ns[] = {0, 1, 255, 256, 257, (1u << 18) + 5};
  for (uint32_t p : ps)
    for (uint32_t n : ns) check_layout(p, n);
  // the rule's arithmetic at its edges: the widest square, every width
  for (uint32_t W = 1; W <= kCommitMaxK; W <<= 1) {
    CHECK(subtree_tile_count(0, kCommitMaxK, W) == kCommitMaxK / W, "tile count of a full row at W = %u", W);
    CHECK(subtree_tile(kCommitMaxK - W, kCommitMaxK, W) == W, "last tile at W = %u", W);
    SubtreeWalk sw;
    CHECK(sw.init(kCommitMaxK - W, kCommitMaxK, W, kCommitMaxK, 1, range_proof_nodes(kCommitMaxK - W, kCommitMaxK, 2 * kCommitMaxK)),
          "init of the last tile at W = %u", W);
  }
  CHECK(sub_tree_width((uint64_t)kCommitMaxK * kCommitMaxK, 1) == kCommitMaxK, "SubTreeWidth of the widest square");
  CHECK(sub_tree_width(1, 0xFFFFFFFFu) == 1, "SubTreeWidth at the largest threshold");
  if (g_fail) {
    fprintf(stderr, "commitment_arena_check: %d failure(s)\n", g_fail);
    return 1;
  }
  printf("commitment_arena_check: all passed\n");
  return 0;
}
