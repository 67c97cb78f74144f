// rebuild.h — what rebuild.cpp (the C ABI of cda_samples_assemble_device and cda_square_rebuild) and
// rebuild_kernels.hip share: the assembly's arguments and workspace, the launches; and the head and tail of a rebuild,
// which cda_square_rebuild and cda_square_rebuild_axes (axis_half.cpp) run around their own assembly.
#pragma once
#include <vector>

#include "sampling.h"

namespace cda {

// cda_samples_assemble_device's arguments, all device memory (include/cda.h), and its workspace (rebuild.cpp,
// rebuild_kernels.hip)
struct AssembleArgs {
  const cda_sample_desc* descs;
  const uint8_t* shares;
  const uint8_t* nodes;
  const uint8_t* roots;
  uint8_t* eds;
  uint8_t* present;
  uint8_t* statuses;
  uint32_t k, nsamples, nnodes_total;
  // workspace.  Per sample: the NMT leg's descriptor, namespace and verdict.  Per cell of the square: the lowest
  // verified sample that claims it (sample_place_rule.h kSampleNoOwner: none).
  cda_nmt_proof_desc* nmt_descs;
  uint8_t* nmt_ns;
  uint8_t* ok;
  uint32_t* owner;
};
inline void assemble_workspace(AssembleArgs& a, Arena& ws) {  // the layout, from a.k and a.nsamples
  const size_t n = a.nsamples, cells = 4 * (size_t)a.k * a.k;
  a.nmt_descs = ws.take<cda_nmt_proof_desc>(n);
  a.nmt_ns = ws.take<uint8_t>(n * CDA_NAMESPACE_SIZE);
  a.ok = ws.take<uint8_t>(n);
  a.owner = ws.take<uint32_t>(cells);
}
int launch_sample_prep(const AssembleArgs& a, hipStream_t s);   // malformed check; descriptors, namespaces
int launch_sample_claim(const AssembleArgs& a, hipStream_t s);  // owner[cell] = the lowest verified sample
int launch_sample_place(const AssembleArgs& a, hipStream_t s);  // owners' shares -> cells; the statuses

// The host side of a rebuild call: the committed roots as the caller gave them and as one array, rows then columns
// (as the rules index them), and the presence map, the caller's or one of the call's own.
struct RebuildHost {
  const uint8_t *row_roots, *col_roots;
  std::vector<uint8_t> roots, own_present;
  uint8_t* present;
  RebuildHost(uint32_t k, const uint8_t* row_roots, const uint8_t* col_roots, uint8_t* present_or_null);
};
// What a rebuild ends in once its n pieces are assembled into b.eds, the presence map at d_present and the pieces'
// statuses at d_statuses (device memory): both back in one wait, rsmt2d Repair of the square where it lies, the EDS
// back if wanted -- on CDA_E_UNREPAIRABLE and CDA_E_BYZANTINE as far as rsmt2d got, and no handle -- then the
// commitment in place, which must give h.roots.  call: the C ABI name, for the internal error's text.  Lock held.
int rebuild_finish(cda_ctx* c, uint32_t k, SquareBuild& b, const uint8_t* d_present, const uint8_t* d_statuses,
                   uint32_t n, uint8_t* statuses, RebuildHost& h, uint8_t* eds_or_null, cda_square** out, uint8_t* dah,
                   cda_err_info* err, const char* call, hipStream_t s);

}  // namespace cda
