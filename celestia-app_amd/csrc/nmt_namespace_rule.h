// nmt_namespace_rule.h — nmt ProveNamespace's bounds and Proof.VerifyNamespace's checks before any hashing, as plain
// byte compares shared by the kernels (sampling_kernels.hip) and the host planner (plan::namespace_bounds,
// plan::namespace_precheck in plan.cpp, which builds with a plain C++ compiler).  NamespaceIDSize = 29,
// IgnoreMaxNamespace = true: a node is min (29 B) ‖ max (29 B) ‖ digest (32 B), and its max already carries the
// IgnoreMax rule.  DESIGN §18 states the rules (P1-P3, V1-V6) in full.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "nmt_verify_rule.h"

namespace cda {

constexpr uint32_t kNsSize = 29, kNsNodeSize = 90;
constexpr uint32_t kNoLeafHash = 0xFFFFFFFFu;  // CDA_NO_LEAF_HASH

// what is left to do for a proof that passed V1-V5
enum NsPrecheck : int {
  kNsReject = 0,     // false by the numbers and namespaces alone
  kNsAcceptEmpty,    // V2: an empty proof of a namespace outside the root's range (or of the empty tree)
  kNsInclusion,      // the root is recomputed from the leaves (VerifyInclusion's leg)
  kNsAbsence,        // the root is recomputed from the supplied leaf node
};

// namespaces as 29-byte big-endian strings: <0, 0, >0
CDA_HD int ns_compare(const uint8_t* a, const uint8_t* b) {
  for (uint32_t i = 0; i < kNsSize; i++)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return 0;
}
CDA_HD const uint8_t* node_min(const uint8_t* node) { return node; }
CDA_HD const uint8_t* node_max(const uint8_t* node) { return node + kNsSize; }
// V1
CDA_HD bool node_well_formed(const uint8_t* node) { return ns_compare(node_min(node), node_max(node)) <= 0; }
// P1 (and half of V2): the namespace lies outside [root.min, root.max]
CDA_HD bool ns_outside_root(const uint8_t* nid, const uint8_t* root) {
  return ns_compare(nid, node_min(root)) < 0 || ns_compare(nid, node_max(root)) > 0;
}
// the root of a tree without leaves: 0 x 58 ‖ SHA256("")
CDA_HD bool is_empty_root(const uint8_t* root) {
  const uint8_t d[32] = {0xe3, 0xb0, 0xc4, 0x42, 0x98, 0xfc, 0x1c, 0x14, 0x9a, 0xfb, 0xf4, 0xc8, 0x99, 0x6f, 0xb9, 0x24,
                         0x27, 0xae, 0x41, 0xe4, 0x64, 0x9b, 0x93, 0x4c, 0xa4, 0x95, 0x99, 0x1b, 0x78, 0x52, 0xb8, 0x55};
  uint32_t diff = 0;
  for (uint32_t i = 0; i < 2 * kNsSize; i++) diff |= root[i];
  for (uint32_t i = 0; i < 32; i++) diff |= (uint32_t)(root[2 * kNsSize + i] ^ d[i]);
  return diff == 0;
}

// V1-V5 of VerifyNamespace(nid, start, end, nodes[0, nnodes), leaf_hash or null, nleaves leaves, root).  Fewer nodes
// than the left hull needs (V6's count check) is rejected here too, so that the split of V5 is well defined.
CDA_HD NsPrecheck ns_precheck(const uint8_t* nid, uint32_t start, uint32_t end, const uint8_t* nodes, uint32_t nnodes,
                              const uint8_t* leaf_hash, uint32_t nleaves, const uint8_t* root) {
  if (!node_well_formed(root) || (leaf_hash && !node_well_formed(leaf_hash))) return kNsReject;  // V1
  for (uint32_t i = 0; i < nnodes; i++)
    if (!node_well_formed(nodes + (size_t)i * kNsNodeSize)) return kNsReject;
  if (start > end) return kNsReject;
  if (start == end)  // V2
    return nnodes == 0 && !leaf_hash && nleaves == 0 && (ns_outside_root(nid, root) || is_empty_root(root))
               ? kNsAcceptEmpty
               : kNsReject;
  if (leaf_hash) {  // V3
    if (end != start + 1 || ns_compare(nid, node_min(leaf_hash)) >= 0) return kNsReject;
  } else if (nleaves != end - start) {  // V4
    return kNsReject;
  }
  const uint32_t nleft = VerifyWalk::popcount(start);  // V5: the subtrees left of the range, then those right of it
  if (nnodes < nleft) return kNsReject;
  for (uint32_t i = 0; i < nnodes; i++) {
    const uint8_t* x = nodes + (size_t)i * kNsNodeSize;
    if (i < nleft ? ns_compare(node_max(x), nid) >= 0 : ns_compare(node_min(x), nid) <= 0) return kNsReject;
  }
  return leaf_hash ? kNsAbsence : kNsInclusion;
}

}  // namespace cda
