// befp.h — what befp.cpp (the C ABI of cda_befp_validate*) and befp_kernels.hip share: the verifier's arguments and
// workspace, the launches.
#pragma once
#include "sampling.h"

namespace cda {

// cda_befp_validate's arguments, all device memory (include/cda.h), and its workspace (befp.cpp, befp_kernels.hip)
struct BefpArgs {
  const cda_befp_desc* descs;
  const cda_befp_entry* entries;
  const uint8_t* shares;
  const uint8_t* nodes;
  const uint8_t* roots;
  int32_t* verdicts;
  uint32_t k, nproofs, nentries, nnodes_total, nroots;
  // workspace.  Per proof: the verdict of B1 and B2 (befp_rule.h), the decoder's codeword offset and stride, the tree's
  // axis index, its root record and status word.  Per proof and slot j < 2k: the NMT leg's descriptor, namespace and
  // verdict of the proof's j-th entry (a slot of its own per proof, so that proofs never share a result), the
  // decoder's present mask, and the axis buffer [nproofs][2k][512].
  int32_t* pre;
  long long* cw_off;
  long long* cw_stride;
  unsigned long long* axis_idx;
  unsigned long long* status;
  uint8_t* recs;
  cda_nmt_proof_desc* nmt_descs;
  uint8_t* nmt_ns;
  uint8_t* nmt_ok;
  uint8_t* mask;
  uint8_t* axes;
};
inline void befp_workspace(BefpArgs& a, Arena& ws) {  // the layout, from a.k and a.nproofs; without the axis buffers
  const size_t n = a.nproofs, slots = n * 2 * a.k;
  a.pre = ws.take<int32_t>(n);
  a.cw_off = ws.take<long long>(n);
  a.cw_stride = ws.take<long long>(n);
  a.axis_idx = ws.take<unsigned long long>(n);
  a.status = ws.take<unsigned long long>(n);
  a.recs = ws.take<uint8_t>(n * CDA_REC_BYTES);
  a.nmt_descs = ws.take<cda_nmt_proof_desc>(slots);
  a.nmt_ns = ws.take<uint8_t>(slots * CDA_NAMESPACE_SIZE);
  a.nmt_ok = ws.take<uint8_t>(slots);
  a.mask = ws.take<uint8_t>(slots);
}
int launch_befp_prep(const BefpArgs& a, hipStream_t s);     // B1, B2; descriptors, namespaces, masks
int launch_befp_gather(const BefpArgs& a, hipStream_t s);   // entry shares -> axis buffers
int launch_befp_combine(const BefpArgs& a, hipStream_t s);  // the verdicts

}  // namespace cda
