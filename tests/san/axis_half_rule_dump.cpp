// axis_half_rule_dump.cpp — the host form of celestia-app_amd/csrc/axis_half_rule.h and the layout of the
// workspace its kernels index (axis_half_workspace, csrc/axis_half.h), built and run under AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_axis_halves.py, which compares the output line for line with its Python
// restatement of the rule.  No device is touched (hipcc as the host compiler: the headers need HIP's).
//   H lines  H0 and what prep and scatter derive, for every descriptor with axis 0..2, index 0..2k, side 0..2 and
//            root_off in {0, 1, 4k} at k in {1, 2}, verifying (nroots = 4k + 1) and assembling (nroots = 4k):
//            "H k asm axis index side root_off : ok tree_index root masks sources"
//   S lines  the placement of every ordered set of up to three halves at k = 1, with every combination of verified
//            flags and of equal-bytes flags of the pairs: "S ids v e : statuses axis_owners cell_owners"
//   A lines  the workspace measured, bound to a heap buffer of exactly the measured size and written the way the
//            kernels index it, with the axis buffers, the square and its presence map beside it, so a slot the
//            measuring walk did not count, or a cell outside the square, is a heap overflow the sanitizer reports:
//            "A k n asm bytes"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../celestia-app_amd/csrc/axis_half_rule.h"
#include "../../celestia-app_amd/csrc/axis_half.h"

using namespace cda;

static void dump_h0(uint32_t k, uint32_t assembling) {
  const uint32_t w = 2 * k;
  const AxisHalfShape t{k, assembling ? 4 * k : 4 * k + 1, assembling};
  const uint32_t offs[] = {0, 1, 4 * k};
  for (uint32_t axis = 0; axis <= 2; axis++)
    for (uint32_t index = 0; index <= w; index++)
      for (uint32_t side = 0; side <= 2; side++)
        for (uint32_t root_off : offs) {
          const cda_axis_half_desc d{axis, index, side, root_off};
          const bool ok = axis_half_well_formed(d, t);
          printf("H %u %u %u %u %u %u : %d %llu %lld ", k, assembling, axis, index, side, root_off, (int)ok,
                 (unsigned long long)axis_half_tree_index(d, ok), ok ? (long long)axis_half_root(d, k) : -1ll);
          for (uint32_t j = 0; j < w; j++) printf("%u", axis_half_present(d, ok, k, j));
          for (uint32_t j = 0; j < w; j++) printf(" %lld", (long long)axis_half_source(d, ok, k, j));
          printf("\n");
        }
}

static void dump_settle() {
  const uint32_t k = 1, w = 2;
  cda_axis_half_desc all[8];
  for (uint32_t i = 0; i < 8; i++) all[i] = cda_axis_half_desc{i >> 2, (i >> 1) & 1, i & 1, 0};
  for (uint32_t n = 1; n <= 3; n++) {
    uint32_t sets = 1;
    for (uint32_t i = 0; i < n; i++) sets *= 8;
    const uint32_t npairs = n * (n - 1) / 2;
    for (uint32_t set = 0; set < sets; set++)
      for (uint32_t v = 0; v < (1u << n); v++)
        for (uint32_t e = 0; e < (1u << npairs); e++) {
          cda_axis_half_desc descs[3];
          uint32_t ids[3];
          uint8_t status[3];
          for (uint32_t p = 0, rest = set; p < n; p++, rest /= 8) {
            ids[p] = rest % 8;
            descs[p] = all[ids[p]];
            status[p] = (v >> p & 1) ? CDA_HALF_PLACED : CDA_HALF_BAD_ROOT;
          }
          // pair (p, q), p < q, is bit q (q - 1) / 2 + p of e
          auto equal = [&](uint32_t p, uint32_t q) {
            const uint32_t lo = p < q ? p : q, hi = p < q ? q : p;
            return (e >> (hi * (hi - 1) / 2 + lo) & 1) != 0;
          };
          std::vector<uint32_t> axis_owner(2 * w), cell_owner((size_t)w * w);
          axis_half_place_all(k, n, descs, status, axis_owner.data(), cell_owner.data(), equal);
          printf("S");
          for (uint32_t p = 0; p < n; p++) printf(" %u", ids[p]);
          printf(" %u %u :", v, e);
          for (uint32_t p = 0; p < n; p++) printf(" %u", status[p]);
          for (uint32_t o : axis_owner) printf(" %d", (int)o);
          for (uint32_t o : cell_owner) printf(" %d", (int)o);
          printf("\n");
        }
  }
}

static int dump_layout(uint32_t k, uint32_t n, uint32_t assembling) {
  const uint32_t w = 2 * k;
  AxisHalfArgs a{};
  a.k = k;
  a.nhalves = n;
  a.assembling = assembling;
  a.nroots = 4 * k;
  const size_t measured = workspace_bytes(a, axis_half_workspace);
  printf("A %u %u %u %zu\n", k, n, assembling, measured);
  if (measured == 0) return 0;
  uint8_t* buf = (uint8_t*)aligned_alloc(256, measured);
  if (!buf) return 1;
  Arena ar(buf);
  axis_half_workspace(a, ar);
  if (ar.used() != measured || (uint8_t*)a.cw_off != buf) {
    fprintf(stderr, "axis_half_workspace(%u, %u): bound %zu, measured %zu\n", k, n, ar.used(), measured);
    return 1;
  }
  const size_t cells = (size_t)w * w;
  std::vector<uint8_t> shares((size_t)n * k * CDA_SHARE, 0x5A), axes((size_t)n * w * CDA_SHARE), eds(cells * CDA_SHARE),
      present(cells);
  std::vector<cda_axis_half_desc> descs(n);
  const AxisHalfShape t{k, a.nroots, assembling};
  const uint32_t at[] = {0, 1, k - 1, k, w - 1, w, 0xFFFFFFFFu};
  for (uint32_t p = 0; p < n; p++)
    descs[p] = cda_axis_half_desc{p % 3, at[p % 7], (p / 7) % 3, (p % 11 == 10) ? 1u : 0u};
  if (assembling) memset(a.axis_owner, 0xFF, 4 * (size_t)k * sizeof(uint32_t));
  for (uint32_t p = 0; p < n; p++) {  // prep, scatter, what the tree and combine write, claim, place
    const cda_axis_half_desc& d = descs[p];
    const bool ok = axis_half_well_formed(d, t);
    a.cw_off[p] = (long long)((size_t)p * w * CDA_SHARE);
    a.cw_stride[p] = CDA_SHARE;
    a.axis_idx[p] = axis_half_tree_index(d, ok);
    a.status[p] = ~0ull;
    memset(a.recs + (size_t)p * CDA_REC_BYTES, 0, CDA_REC_BYTES);
    for (uint32_t j = 0; j < w; j++) {
      a.mask[(size_t)p * w + j] = axis_half_present(d, ok, k, j);
      const int64_t from = axis_half_source(d, ok, k, j);
      uint8_t* slot = axes.data() + ((size_t)p * w + j) * CDA_SHARE;
      if (from >= 0)
        memcpy(slot, shares.data() + ((size_t)p * k + (size_t)from) * CDA_SHARE, CDA_SHARE);
      else
        memset(slot, 0, CDA_SHARE);
    }
    if (!ok || !assembling) continue;
    uint32_t& o = a.axis_owner[axis_half_key(d, k)];
    if (p < o) o = p;
  }
  if (assembling)
    for (uint32_t p = 0; p < n; p++) {
      const cda_axis_half_desc& d = descs[p];
      if (!axis_half_well_formed(d, t) || a.axis_owner[axis_half_key(d, k)] != p) continue;
      for (uint32_t pos = 0; pos < w; pos++) {
        const uint32_t cross = a.axis_owner[axis_half_cross_key(d, k, pos)];
        if (!axis_half_owns(p, cross)) continue;
        const size_t cell = axis_half_cell(d, k, pos);
        memcpy(eds.data() + cell * CDA_SHARE, axes.data() + ((size_t)p * w + pos) * CDA_SHARE, CDA_SHARE);
        present[cell] = 1;
      }
    }
  free(buf);
  return 0;
}

int main() {
  for (uint32_t k : {1u, 2u})
    for (uint32_t assembling : {0u, 1u}) dump_h0(k, assembling);
  dump_settle();
  const uint32_t ks[] = {1, 2, 4, 16, 128, 512};
  const uint32_t ns[] = {0, 1, 7, 255, 256, 257};
  for (uint32_t k : ks)
    for (uint32_t n : ns)
      for (uint32_t assembling : {0u, 1u})
        if (dump_layout(k, n, assembling)) return 1;
  printf("axis_half_rule_dump: done\n");
  return 0;
}
