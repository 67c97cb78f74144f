// axis_half_rule.h — what becomes of one half of a row or column (celestia-node's shwap.Row: k consecutive cells of an
// axis, sent with no proof) when it is verified and when a square is assembled from such halves, as plain
// integer and byte code shared by the kernels (axis_half_kernels.hip) and host code that builds with a plain C++
// compiler (tests/san/axis_half_rule_dump.cpp).  cda.rows.verify_host / assemble_host are the same rule in Python.
//
// Half p covers cells [side k, side k + k) of row `index` (axis 0) or column `index` (axis 1); its block's roots are
// roots[root_off, root_off + 4k), rows then columns.  No index taken from the input is used before it is bounded:
// axis_half_well_formed bounds the descriptor, and only a descriptor that passed is read through.
//   H0 MALFORMED  axis > 1, index >= 2k, side > 1 or root_off + 4k > nroots (assembling: root_off != 0)
//   H1            side 0: cells [k, 2k) := Encode(cells [0, k)); side 1: cells [0, k) := Decode of cells [k, 2k)
//   H2 BAD_ROOT   the wrapper tree over the 2k cells cannot be built, or its root is not roots[axis_half_root]
//      PLACED     otherwise (cda_axis_halves_verify's "verified")
// Assembling, among the verified halves: the lowest-indexed half of an axis is that axis's half, a later one is
// DUPLICATE; a cell belongs to the lower-indexed of its row's and its column's half; a half whose bytes differ from
// the owner's at a cell it does not own is CONFLICT.  Owners are minima and conflicts an OR, so the result does not
// depend on the order the halves are looked at.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/cda.h"
#include "befp_rule.h"

namespace cda {

constexpr uint32_t kHalfNoOwner = ~0u;  // an axis no verified half claims

// the shape of a call: assembling, every half belongs to the one square whose 4k roots are given
struct AxisHalfShape {
  uint32_t k, nroots, assembling;
};

// H0
CDA_HD bool axis_half_well_formed(const cda_axis_half_desc& d, const AxisHalfShape& t) {
  const uint32_t w = 2 * t.k;
  if (d.axis > 1 || d.index >= w || d.side > 1) return false;
  if ((unsigned long long)d.root_off + 2ull * w > t.nroots) return false;
  return !t.assembling || d.root_off == 0;
}
// The decoder's present flag of slot j < 2k of a half's axis buffer.  All ones (nothing for the decoder to write) for
// a half that failed H0 and for side 0, whose missing cells the encoder writes.
CDA_HD uint8_t axis_half_present(const cda_axis_half_desc& d, bool well_formed, uint32_t k, uint32_t j) {
  return (well_formed && d.side == CDA_SIDE_SECOND) ? (uint8_t)(j >= k) : (uint8_t)1;
}
// Where slot j < 2k of a half's axis buffer comes from: share `j - side k` of the half, or nothing (-1: zeroed)
CDA_HD int64_t axis_half_source(const cda_axis_half_desc& d, bool well_formed, uint32_t k, uint32_t j) {
  if (!well_formed) return -1;
  const uint32_t first = d.side * k;
  return (j >= first && j < first + k) ? (int64_t)(j - first) : -1;
}
// the tree's axis index (0 for a half that failed H0, as befp_prep_kernel has it for rejected proofs)
CDA_HD uint64_t axis_half_tree_index(const cda_axis_half_desc& d, bool well_formed) {
  return well_formed ? d.index : 0;
}
// the committed root of a well-formed half, as an index into the call's roots
CDA_HD size_t axis_half_root(const cda_axis_half_desc& d, uint32_t k) {
  return (size_t)d.root_off + (size_t)d.axis * 2 * k + d.index;
}
// H0 then H2
CDA_HD uint8_t axis_half_verdict(bool well_formed, bool tree_built, bool root_same) {
  if (!well_formed) return CDA_HALF_MALFORMED;
  return (tree_built && root_same) ? CDA_HALF_PLACED : CDA_HALF_BAD_ROOT;
}

// ---- placement: well-formed halves of one square ----
// the axis of a half among the square's 4k axes (rows then columns), and the axis that crosses it at position pos
CDA_HD uint32_t axis_half_key(const cda_axis_half_desc& d, uint32_t k) { return d.axis * 2 * k + d.index; }
CDA_HD uint32_t axis_half_cross_key(const cda_axis_half_desc& d, uint32_t k, uint32_t pos) {
  return (1 - d.axis) * 2 * k + pos;
}
// row-major cell at position pos of the half's axis
CDA_HD size_t axis_half_cell(const cda_axis_half_desc& d, uint32_t k, uint32_t pos) {
  const size_t w = 2 * (size_t)k;
  return d.axis == CDA_AXIS_ROW ? d.index * w + pos : pos * w + d.index;
}
// The cell at position pos of verified half p, the half of its axis, whose crossing axis belongs to half `cross`
// (kHalfNoOwner: to none): p owns it unless the crossing axis's half has the lower index.
CDA_HD bool axis_half_owns(uint32_t p, uint32_t cross) { return p < cross; }
// verified half p of an axis whose lowest verified half is `axis_owner`; differs: at some cell p does not own, p's
// bytes are not the owner's
CDA_HD uint8_t axis_half_settle(uint32_t p, uint32_t axis_owner, bool differs) {
  if (p != axis_owner) return CDA_HALF_DUPLICATE;
  return differs ? CDA_HALF_CONFLICT : CDA_HALF_PLACED;
}

// The whole placement of n halves on the host, in the steps the kernels take (claim, then place): status[p] on entry
// is the verdict of H0-H2 and on return the final status; axis_owner has 4k slots, cell_owner (2k)^2 (kHalfNoOwner: no
// half).  equal(p, q): the completed axes of halves p and q hold the same bytes in the cell they share.
template <class Equal>
inline void axis_half_place_all(uint32_t k, uint32_t n, const cda_axis_half_desc* descs, uint8_t* status,
                                uint32_t* axis_owner, uint32_t* cell_owner, Equal equal) {
  const uint32_t w = 2 * k;
  for (uint32_t a = 0; a < 2 * w; a++) axis_owner[a] = kHalfNoOwner;
  for (size_t c = 0; c < (size_t)w * w; c++) cell_owner[c] = kHalfNoOwner;
  for (uint32_t p = 0; p < n; p++)
    if (status[p] == CDA_HALF_PLACED) {
      uint32_t& o = axis_owner[axis_half_key(descs[p], k)];
      if (p < o) o = p;
    }
  for (uint32_t p = 0; p < n; p++) {
    if (status[p] != CDA_HALF_PLACED) continue;
    const cda_axis_half_desc& d = descs[p];
    const uint32_t mine = axis_owner[axis_half_key(d, k)];
    bool differs = false;
    if (mine == p)
      for (uint32_t pos = 0; pos < w; pos++) {
        const uint32_t cross = axis_owner[axis_half_cross_key(d, k, pos)];
        if (axis_half_owns(p, cross))
          cell_owner[axis_half_cell(d, k, pos)] = p;
        else if (!equal(p, cross))
          differs = true;
      }
    status[p] = axis_half_settle(p, mine, differs);
  }
}

}  // namespace cda
