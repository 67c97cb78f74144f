// arena_check.cpp — CPU check of the carve helper (celestia-app_amd/csrc/arena.h) and of the three workspace layouts
// that walk it (share_proof.h: validate_workspace, namespace_proof.h: ns_verify_workspace, befp.h: befp_workspace),
// built and run under AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_sanitize.py.  No device is touched:
// each layout is measured, then bound to a heap buffer of exactly the measured size, and every byte of every slot is
// written through the bound pointers, so a slot the measuring walk did not count is a heap overflow the sanitizer
// reports.
//
// Per layout and shape: the first slot is the base (launch_share_proofs_validate clears the layout from its first
// slot), every slot is 256-byte aligned, the slots follow each other in the documented order without gap or overlap,
// and the last one ends exactly at the measured size.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../celestia-app_amd/csrc/befp.h"
#include "../../celestia-app_amd/csrc/namespace_proof.h"
#include "../../celestia-app_amd/csrc/share_proof.h"

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

// the shapes: around one 256-thread block and one 256-byte slot, and one large
static const size_t kGrid[] = {0, 1, 255, 256, 257, (1u << 20) - 3};

struct Slot {
  void* p;
  size_t bytes;
};
template <class T>
static Slot slot(T* p, size_t count) {
  return Slot{(void*)p, count * sizeof(T)};
}

// Binds a layout to a heap buffer of exactly `measured` bytes and checks what the header comment says.  `bind` walks
// the arena it is given and returns the slots in the documented order.
template <class Bind>
static void check_layout(const char* what, size_t x, size_t y, size_t measured, Bind bind) {
  CHECK(measured % 256 == 0, "%s(%zu, %zu): measured %zu is no multiple of 256", what, x, y, measured);
  size_t want = 0;
  {
    Arena measure;
    for (const Slot& s : bind(measure)) {
      CHECK(s.p == nullptr, "%s(%zu, %zu): a measuring walk returned a pointer", what, x, y);
      want += align256(s.bytes);
    }
    CHECK(measure.used() == measured, "%s(%zu, %zu): two measuring walks disagree", what, x, y);
  }
  CHECK(want == measured, "%s(%zu, %zu): measured %zu, the slots need %zu", what, x, y, measured, want);
  if (measured == 0) return;  // nothing to bind: every slot is empty
  uint8_t* buf = (uint8_t*)aligned_alloc(256, measured);
  if (!buf) {
    CHECK(false, "%s(%zu, %zu): no memory for %zu bytes", what, x, y, measured);
    return;
  }
  Arena ar(buf);
  const std::vector<Slot> slots = bind(ar);
  CHECK(ar.used() == measured, "%s(%zu, %zu): bound %zu, measured %zu", what, x, y, ar.used(), measured);
  CHECK(slots[0].p == buf, "%s(%zu, %zu): the first slot is not the base", what, x, y);
  uint8_t* at = buf;
  for (size_t i = 0; i < slots.size(); i++) {
    uint8_t* p = (uint8_t*)slots[i].p;
    CHECK(((uintptr_t)p & 255) == 0, "%s(%zu, %zu): slot %zu is not 256-byte aligned", what, x, y, i);
    CHECK(p == at, "%s(%zu, %zu): slot %zu at %td, expected %td", what, x, y, i, p - buf, at - buf);
    memset(p, 0xA5, slots[i].bytes);
    at = p + align256(slots[i].bytes);
  }
  CHECK(at == buf + measured, "%s(%zu, %zu): the last slot ends at %td of %zu", what, x, y, at - buf, measured);
  free(buf);
}

static void check_validate(uint32_t nproofs, uint32_t nrows) {
  ValidateArgs a{};
  a.nproofs = nproofs;
  a.nrows = nrows;
  const size_t n = nrows;
  check_layout("validate_workspace", nproofs, nrows, workspace_bytes(a, validate_workspace), [&](Arena& ar) {
    validate_workspace(a, ar);
    return std::vector<Slot>{slot(a.pre, nproofs),  slot(a.owner, n),
                             slot(a.claims, n),     slot(a.nmt_descs, n),
                             slot(a.nmt_ns, n * CDA_NAMESPACE_SIZE), slot(a.nmt_ok, n),
                             slot(a.row_ok, n)};
  });
}

static void check_ns_verify(uint32_t nproofs) {
  NsVerifyArgs a{};
  a.nproofs = nproofs;
  const size_t n = nproofs;
  check_layout("ns_verify_workspace", nproofs, 0, workspace_bytes(a, ns_verify_workspace), [&](Arena& ar) {
    ns_verify_workspace(a, ar);
    return std::vector<Slot>{slot(a.nmt_descs, n), slot(a.pre, n), slot(a.nmt_ok, n), slot(a.abs_ok, n)};
  });
}

// Shapes of more than 2^22 slots are measured and compared with the slots' sizes but not bound: nproofs * 2k near
// 2^41 is no buffer a host can allocate, and the library refuses such calls (check_axis_shape: 2k is bounded by
// the axis-root kernel and nproofs * 2k by 2^31).  Every value of the grid is bound on both axes below that.
static void check_befp(uint32_t k, uint32_t nproofs) {
  BefpArgs a{};
  a.k = k;
  a.nproofs = nproofs;
  const size_t n = nproofs, slots = n * 2 * k;
  auto bind = [&](Arena& ar) {
    befp_workspace(a, ar);
    return std::vector<Slot>{slot(a.pre, n),       slot(a.cw_off, n),
                             slot(a.cw_stride, n), slot(a.axis_idx, n),
                             slot(a.status, n),    slot(a.recs, n * CDA_REC_BYTES),
                             slot(a.nmt_descs, slots), slot(a.nmt_ns, slots * CDA_NAMESPACE_SIZE),
                             slot(a.nmt_ok, slots), slot(a.mask, slots)};
  };
  const size_t measured = workspace_bytes(a, befp_workspace);
  if (slots <= ((size_t)1 << 22)) {
    check_layout("befp_workspace", k, nproofs, measured, bind);
    return;
  }
  Arena measure;
  size_t want = 0;
  for (const Slot& s : bind(measure)) want += align256(s.bytes);
  CHECK(want == measured, "befp_workspace(%u, %u): measured %zu, the slots need %zu", k, nproofs, measured, want);
  CHECK(a.axes == nullptr, "befp_workspace(%u, %u): the layout set the axis buffers", k, nproofs);
}

static void check_arena() {
  alignas(256) static uint8_t buf[1024];
  Arena ar(buf);
  CHECK(ar.used() == 0, "a fresh arena has used %zu", ar.used());
  CHECK(ar.take<uint32_t>(0) == (uint32_t*)buf && ar.used() == 0, "an empty take at the start moved the arena");
  CHECK(ar.take<uint8_t>(1) == buf && ar.used() == 256, "take(1) did not hand out the first slot");
  CHECK(ar.take<uint64_t>(0) == (uint64_t*)(buf + 256) && ar.used() == 256,
        "an empty take does not return the current position, or moves it");
  CHECK(ar.take<uint8_t>(257) == buf + 256 && ar.used() == 768, "take(257) did not take two slots");
  CHECK(ar.take<uint32_t>(64) == (uint32_t*)(buf + 768) && ar.used() == 1024, "take of exactly one slot");
  Arena measure;
  CHECK(measure.take<uint8_t>(0) == nullptr && measure.used() == 0, "measuring: an empty take");
  CHECK(measure.take<uint32_t>(65) == nullptr && measure.used() == 512, "measuring: 260 bytes are two slots");
  CHECK(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512, "align256");
}

int main() {
  check_arena();
  for (size_t x : kGrid) {
    check_ns_verify((uint32_t)x);
    for (size_t y : kGrid) {
      check_validate((uint32_t)x, (uint32_t)y);
      check_befp((uint32_t)x, (uint32_t)y);
    }
  }
  if (g_fail) {
    fprintf(stderr, "arena_check: %d failure(s)\n", g_fail);
    return 1;
  }
  printf("arena_check: all passed\n");
  return 0;
}
