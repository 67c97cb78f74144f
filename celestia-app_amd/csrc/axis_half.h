// axis_half.h — what axis_half.cpp (the C ABI of the row and column halves) and axis_half_kernels.hip share: the
// arguments and workspace, the launches; and the completion of a batch of axis buffers (decode, encode, tree roots),
// which cda_befp_validate (befp.cpp) runs as well.
#pragma once
#include "sampling.h"

namespace cda {

// cda_axis_halves_verify's and cda_axis_halves_assemble_device's arguments, all device memory (include/cda.h), and
// their workspace (axis_half.cpp, axis_half_kernels.hip)
struct AxisHalfArgs {
  const cda_axis_half_desc* descs;
  const uint8_t* shares;
  const uint8_t* roots;
  uint8_t* statuses;
  uint8_t* eds;      // assembling only, as axis_owner below
  uint8_t* present;
  uint32_t k, nhalves, nroots;
  uint32_t assembling;  // all halves belong to one square: root_off must be 0
  // workspace.  Per half: the decoder's codeword offset and stride, the tree's axis index, its root record and status
  // word; per half and slot j < 2k the decoder's present mask; the axis buffer [nhalves][2k][512].  Per axis of the
  // square (rows then columns): the lowest verified half that claims it (axis_half_rule.h kHalfNoOwner: none).
  long long* cw_off;
  long long* cw_stride;
  unsigned long long* axis_idx;
  unsigned long long* status;
  uint8_t* recs;
  uint8_t* mask;
  uint32_t* axis_owner;
  uint8_t* axes;
};
inline void axis_half_workspace(AxisHalfArgs& a, Arena& ws) {  // the layout, from a.k, a.nhalves and a.assembling
  const size_t n = a.nhalves;
  a.cw_off = ws.take<long long>(n);
  a.cw_stride = ws.take<long long>(n);
  a.axis_idx = ws.take<unsigned long long>(n);
  a.status = ws.take<unsigned long long>(n);
  a.recs = ws.take<uint8_t>(n * CDA_REC_BYTES);
  a.mask = ws.take<uint8_t>(n * 2 * a.k);
  a.axis_owner = ws.take<uint32_t>(a.assembling ? 4 * (size_t)a.k : 0);
}
int launch_axis_half_prep(const AxisHalfArgs& a, hipStream_t s);     // H0; masks, offsets, axis indices
int launch_axis_half_scatter(const AxisHalfArgs& a, hipStream_t s);  // the halves' shares -> axis buffers, zeros beside
int launch_axis_half_combine(const AxisHalfArgs& a, hipStream_t s);  // the verdicts of H0-H2
int launch_axis_half_claim(const AxisHalfArgs& a, hipStream_t s);    // axis_owner = the lowest verified half
int launch_axis_half_place(const AxisHalfArgs& a, hipStream_t s);    // owners' cells -> the square; the statuses
// nq halves out of a retained square, packed in query order (the queries were checked by the host)
int launch_axis_half_gather(const SquareView& v, const cda_axis_half_desc* d_q, uint32_t nq, uint8_t* d_shares,
                            hipStream_t s);

// k and the count of a call that completes axes: k a power of two (not_pow2 is returned otherwise) that the axis-root
// kernel takes whole (2k leaves in one workgroup's LDS)
int check_axis_shape(uint32_t k, uint32_t n, int not_pow2);

// n axis buffers of 2k x 512 B, all device memory, as the decoder and the axis-root kernel take them (host-only: no
// kernel takes this struct), and the caller's profile-scope names for the legs
struct AxisBufs {
  uint8_t* axes;
  const long long* cw_off;
  const long long* cw_stride;
  const uint8_t* mask;
  const unsigned long long* axis_idx;
  uint8_t* recs;
  unsigned long long* status;
};
struct AxisScopes {
  const char *decode, *encode8, *encode16, *roots;
};
// Completes every buffer and hashes it: the missing slots decoded (when asked: mask says which are there), slots
// [k, 2k) := Encode(slots [0, k)) in the field 2k selects, then the wrapper tree's root record and status word of
// every buffer.  One stream, no host wait.
int complete_axes(cda_ctx* c, const AxisBufs& b, uint32_t n, uint32_t k, bool decode, const AxisScopes& scopes,
                  hipStream_t s);

}  // namespace cda
