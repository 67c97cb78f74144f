// befp_rule.h — the checks of a bad-encoding fraud proof that need no hash and what the
// prep step derives from a proof that passes them, as plain integer and byte code shared by the kernels
// (befp_kernels.hip) and the host planner (plan::befp_precheck in plan.cpp, which builds with a plain C++ compiler).
// No index taken from the input is used before it is bounded: befp_head_ok bounds the descriptor, and only then
// befp_entry_ok reads the proof's entries, and only an entry that passed is read through.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/cda.h"
#include "nmt_verify_rule.h"

namespace cda {

constexpr int kBefpPending = 2;  // passed B1 and B2: B3 and B4 decide (never a final verdict)
constexpr uint32_t kBefpNsSize = 29, kBefpShare = 512;

// the totals of a cda_befp_validate call
struct BefpTotals {
  uint32_t k, nentries, nnodes_total, nroots;
};

// B1, the descriptor alone: the axis, and that its entries and its block of 4k roots lie inside the totals
CDA_HD bool befp_head_ok(const cda_befp_desc& d, const BefpTotals& t) {
  const uint32_t w = 2 * t.k;
  return d.axis <= 1 && d.index < w && d.nshares <= w &&
         (unsigned long long)d.entry_off + d.nshares <= t.nentries &&
         (unsigned long long)d.root_off + 2ull * w <= t.nroots;
}
// B1, entry j of a descriptor that passed befp_head_ok: the position inside the axis and above the entry before it
// (strictly increasing: no duplicates), the nodes inside the total
CDA_HD bool befp_entry_ok(const cda_befp_desc& d, const cda_befp_entry* entries, uint32_t j, const BefpTotals& t) {
  const cda_befp_entry& e = entries[d.entry_off + j];
  if (e.pos >= 2 * t.k || (unsigned long long)e.node_off + e.nnodes > t.nnodes_total) return false;
  return j == 0 || entries[d.entry_off + j - 1].pos < e.pos;
}
// B1 then B2, given whether every entry passed
CDA_HD int befp_pre_verdict(const cda_befp_desc& d, bool head_ok, bool entries_ok, const BefpTotals& t) {
  if (!head_ok || !entries_ok) return CDA_BEFP_MALFORMED;
  return d.nshares < t.k ? CDA_BEFP_TOO_FEW : kBefpPending;
}

// B3's descriptor of entry j (the e-th of the call): leaf [index, index + 1) of the ORTHOGONAL tree, whose root is the
// column root `pos` for a row and the row root `pos` for a column
CDA_HD cda_nmt_proof_desc befp_nmt_desc(const cda_befp_desc& d, const cda_befp_entry& e, uint32_t eidx, uint32_t k) {
  cda_nmt_proof_desc n;
  n.start = d.index;
  n.end = d.index + 1;
  n.node_off = e.node_off;
  n.nnodes = e.nnodes;
  n.leaf_off = eidx;
  n.root = d.root_off + (d.axis == CDA_AXIS_ROW ? 2 * k + e.pos : e.pos);
  return n;
}
CDA_HD cda_nmt_proof_desc befp_empty_desc() {
  cda_nmt_proof_desc n;
  n.start = n.end = n.node_off = n.nnodes = n.leaf_off = n.root = 0;
  return n;
}
// the wrapper's quadrant rule (cda.sampling.sample_namespace): the share's own namespace in Q0, else parity
CDA_HD void befp_namespace(uint32_t k, uint32_t index, uint32_t pos, const uint8_t* share, uint8_t* out) {
  const bool q0 = index < k && pos < k;
  for (uint32_t i = 0; i < kBefpNsSize; i++) out[i] = q0 ? share[i] : (uint8_t)0xFF;
}

}  // namespace cda
