// mixed_route.h — the pure part of the mixed-size batch (cda_extend_commit_mixed, mixed.cpp): where each block of a
// call sits in the packed buffers, which blocks take the one-workgroup kernel (small_square_kernels.hip), and how the
// others are batched -- groups of equal k for the host form, runs of consecutive equal k for the device form.  Plain
// C++ with no HIP include, shared by the launcher and by host code that builds with a plain C++ compiler
// (tests/san/mixed_route_dump.cpp, which tests/test_mixed_batch.py runs).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace cda {

constexpr uint32_t kSmallSquareMaxK = 8;         // 4k^2 = 256 cells: one per thread of the workgroup
constexpr int kSmallSquareThreads = 256;
constexpr int kSmallSquareMaxLds = 80 * 1024;    // half of a CU's 160 KiB: two blocks share a CU
constexpr int kMixedSmallMaxDefault = 8;         // CDA_OPT_MIXED_SMALL_MAX of a new context

// The largest k of a call's blocks that takes the fused kernel: 0 (none), 1, 2, 4 or 8
inline bool mixed_small_max_valid(int64_t v) { return v == 0 || v == 1 || v == 2 || v == 4 || v == 8; }

// small_square_kernel's dynamic LDS for a launch whose largest block has this k: the 2 KiB of layer matrices, then one
// region used in turn by the two bit-sliced codec states (512 k^2 bytes each), by the leaf records and the tree levels
// (two buffers of 4k^2 records of 112 B: 896 k^2) and by the DAH fold (48 digests of 32 B and 64 schedule rows of 68
// words: 18,944 B).
constexpr size_t kSmallSquareCbBytes = 256 * 8;
constexpr size_t kSmallSquareDahBytes = (size_t)(48 * 8 + 64 * 68) * 4;
inline size_t small_square_lds_bytes(uint32_t kmax) {
  return kSmallSquareCbBytes + std::max<size_t>((size_t)1024 * kmax * kmax, kSmallSquareDahBytes);
}

// ---- packed offsets ----
// Block b is a ks[b] x ks[b] square of 512-byte shares; every buffer is packed in block order with no padding.
// ods / eds: byte offsets; roots: the block's first row root (or column root) in the host form's row_roots /
// col_roots arrays of 90-B nodes, 2k per block -- the device form's records (4k per block: row roots, then column
// roots) start at twice that.  Each vector has n + 1 entries, the last being the total.
struct MixedOffsets {
  std::vector<uint64_t> ods, eds, roots;
};
inline MixedOffsets mixed_offsets(const uint32_t* ks, uint32_t n) {
  MixedOffsets o;
  o.ods.assign(n + 1, 0);
  o.eds.assign(n + 1, 0);
  o.roots.assign(n + 1, 0);
  for (uint32_t b = 0; b < n; b++) {
    const uint64_t k = ks[b];
    o.ods[b + 1] = o.ods[b] + k * k * 512;
    o.eds[b + 1] = o.eds[b] + 4 * k * k * 512;
    o.roots[b + 1] = o.roots[b] + 2 * k;
  }
  return o;
}

// ---- argument check ----
// 0, or 1 (some ks[b] is not a power of two; *bad = the lowest such b), or 2 (all are, some ks[b] > max_k; *bad = the
// lowest such b)
inline int mixed_check_ks(const uint32_t* ks, uint32_t n, uint32_t max_k, uint32_t* bad) {
  for (uint32_t b = 0; b < n; b++)
    if (ks[b] == 0 || (ks[b] & (ks[b] - 1))) return *bad = b, 1;
  for (uint32_t b = 0; b < n; b++)
    if (ks[b] > max_k) return *bad = b, 2;
  return 0;
}

// ---- the small / large split ----
inline bool mixed_is_small(uint32_t k, uint32_t small_max) { return k <= small_max; }  // small_max 0: none
// the small blocks of a call, in input order
inline std::vector<uint32_t> mixed_small_blocks(const uint32_t* ks, uint32_t n, uint32_t small_max) {
  std::vector<uint32_t> s;
  for (uint32_t b = 0; b < n; b++)
    if (mixed_is_small(ks[b], small_max)) s.push_back(b);
  return s;
}
// Host form: every other block grouped by k (groups by ascending k, blocks stable in input order)
struct MixedGroup {
  uint32_t k;
  std::vector<uint32_t> blocks;
};
inline std::vector<MixedGroup> mixed_groups(const uint32_t* ks, uint32_t n, uint32_t small_max) {
  std::vector<MixedGroup> g;
  for (uint32_t b = 0; b < n; b++) {
    if (mixed_is_small(ks[b], small_max)) continue;
    auto it = std::find_if(g.begin(), g.end(), [&](const MixedGroup& x) { return x.k == ks[b]; });
    if (it == g.end()) it = g.insert(g.end(), MixedGroup{ks[b], {}});
    it->blocks.push_back(b);
  }
  std::stable_sort(g.begin(), g.end(), [](const MixedGroup& a, const MixedGroup& b) { return a.k < b.k; });
  return g;
}
// Device form: each maximal run of consecutive large blocks of equal k (a small block between two ends a run: the
// run is one contiguous sub-range of every packed buffer)
struct MixedRun {
  uint32_t k, first, count;
};
inline std::vector<MixedRun> mixed_runs(const uint32_t* ks, uint32_t n, uint32_t small_max) {
  std::vector<MixedRun> r;
  for (uint32_t b = 0; b < n; b++) {
    if (mixed_is_small(ks[b], small_max)) continue;
    if (!r.empty() && r.back().k == ks[b] && r.back().first + r.back().count == b)
      r.back().count++;
    else
      r.push_back(MixedRun{ks[b], b, 1});
  }
  return r;
}

// ---- the fused kernel's descriptors ----
// One per workgroup: the block's log2 k, its index in the status and DAH arrays, the byte offsets of its ODS and EDS
// and its first 96-B root record.
struct SmallSquareDesc {
  uint32_t log2k, block;
  uint64_t ods_off, eds_off, rec_off;
};
inline uint32_t mixed_ilog2(uint32_t v) {
  uint32_t l = 0;
  while ((1u << l) < v) l++;
  return l;
}
// descriptors of `blocks` (indices into ks) whose buffers are packed as `off` says; *kmax: their largest k
inline std::vector<SmallSquareDesc> small_square_descs(const uint32_t* ks, const std::vector<uint32_t>& blocks,
                                                       const MixedOffsets& off, uint32_t* kmax) {
  std::vector<SmallSquareDesc> d;
  *kmax = 0;
  for (uint32_t b : blocks) {
    d.push_back(SmallSquareDesc{mixed_ilog2(ks[b]), b, off.ods[b], off.eds[b], 2 * off.roots[b]});
    *kmax = std::max(*kmax, ks[b]);
  }
  return d;
}

}  // namespace cda
