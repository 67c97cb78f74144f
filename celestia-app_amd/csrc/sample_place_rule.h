// sample_place_rule.h — what becomes of one proved sample when a square is assembled from samples, as
// plain integer code shared by the kernels (rebuild_kernels.hip) and host code that builds with a plain C++ compiler
// (tests/san/rebuild_arena_check.cpp).  cda.sampling.assemble_host is the same rule in Python.
//
// A sample is one cell with a one-leaf proof in its row tree (axis 0: cell (index, pos)) or its column tree (axis 1:
// cell (pos, index)).  No index taken from the input is used before it is bounded: sample_well_formed bounds the
// coordinates, and the verifier bounds the nodes (a descriptor outside the totals is its verdict 0).
//   MALFORMED   axis > 1, index >= 2k or pos >= 2k: nothing is read through it
//   REJECTED    VerifyInclusion is false
//   PLACED      verified, and the lowest-indexed verified sample of its cell: its bytes are the cell
//   DUPLICATE   verified, not the lowest, the same bytes as the placed ones
//   CONFLICT    verified, not the lowest, other bytes (one cell committed differently in its row and its column tree)
// The lowest index wins, so the result does not depend on the order the samples are looked at.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/cda.h"
#include "befp_rule.h"

namespace cda {

constexpr uint32_t kSampleNoOwner = ~0u;  // a cell no verified sample claims

CDA_HD bool sample_well_formed(const cda_sample_desc& d, uint32_t k) {
  return d.axis <= 1 && d.index < 2 * k && d.pos < 2 * k;
}
// row-major cell of a well-formed sample
CDA_HD size_t sample_cell(const cda_sample_desc& d, uint32_t k) {
  const size_t w = 2 * (size_t)k;
  return d.axis == CDA_AXIS_ROW ? d.index * w + d.pos : d.pos * w + d.index;
}
// VerifyInclusion's descriptor of well-formed sample p: leaf [pos, pos + 1) of tree `index` of its axis, the roots
// being the 2k row roots then the 2k column roots, the share being the p-th
CDA_HD cda_nmt_proof_desc sample_nmt_desc(const cda_sample_desc& d, uint32_t p, uint32_t k) {
  cda_nmt_proof_desc n;
  n.start = d.pos;
  n.end = d.pos + 1;
  n.node_off = d.node_off;
  n.nnodes = d.nnodes;
  n.leaf_off = p;
  n.root = d.axis * 2 * k + d.index;
  return n;
}
// the namespace the sample's leaf hashes under: the wrapper's quadrant rule (cda.sampling.sample_namespace)
CDA_HD void sample_namespace(const cda_sample_desc& d, uint32_t k, const uint8_t* share, uint8_t* out) {
  befp_namespace(k, d.index, d.pos, share, out);
}
// verified sample p of a cell whose lowest verified sample is `owner`; same: p's bytes equal the owner's
CDA_HD uint8_t sample_settle(uint32_t p, uint32_t owner, bool same) {
  if (p == owner) return CDA_SAMPLE_PLACED;
  return same ? CDA_SAMPLE_DUPLICATE : CDA_SAMPLE_CONFLICT;
}

}  // namespace cda
