// namespace_proof.h — what namespace_proof.cpp (the C ABI of cda_square_prove_namespace and cda_nmt_verify_namespace*)
// and namespace_kernels.hip share: the prover's launches, the verifier's arguments and workspace, its launch.
#pragma once
#include "sampling.h"

namespace cda {

// cda_square_prove_namespace's kernels, all device memory: the search, the gather and the absence leaf of every query
// (results[q].share_off is left for the next launch), then share_off = the prefix sum of nshares and *d_total = its
// end; launch_namespace_shares copies the INCLUSION results' cells once the host has sized d_shares from the total.
int launch_square_prove_namespace(const SquareView& v, const cda_namespace_query* d_q, uint32_t nq, uint32_t max_nodes,
                                  cda_namespace_result* d_results, uint8_t* d_nodes, uint8_t* d_leaf_hashes,
                                  unsigned long long* d_total, hipStream_t s);
int launch_namespace_shares(const SquareView& v, const cda_namespace_query* d_q, uint32_t nq,
                            const cda_namespace_result* d_results, uint8_t* d_shares, hipStream_t s);

// cda_nmt_verify_namespace's arguments, all device memory (include/cda.h), and its workspace
struct NsVerifyArgs {
  const cda_nmt_ns_proof_desc* descs;
  const uint8_t* namespaces;
  const uint8_t* roots;
  const uint8_t* nodes;
  const uint8_t* leaf_hashes;
  const uint8_t* leaves;
  uint8_t* ok;
  uint32_t nproofs, nroots, nnodes_total, nleaf_hashes, nleaves_total;
  // workspace, per proof: the inclusion leg's descriptor (empty unless the proof goes there), what V1-V5 left to do
  // (NsPrecheck), the inclusion leg's and the absence leg's verdicts
  cda_nmt_proof_desc* nmt_descs;
  uint8_t* pre;
  uint8_t* nmt_ok;
  uint8_t* abs_ok;
};
inline void ns_verify_workspace(NsVerifyArgs& a, Arena& ws) {  // the layout, from a.nproofs
  a.nmt_descs = ws.take<cda_nmt_proof_desc>(a.nproofs);
  a.pre = ws.take<uint8_t>(a.nproofs);
  a.nmt_ok = ws.take<uint8_t>(a.nproofs);
  a.abs_ok = ws.take<uint8_t>(a.nproofs);
}
// prep (V1-V5), launch_nmt_verify over the inclusion proofs, the absence chains, combine
int launch_nmt_verify_namespace(const NsVerifyArgs& a, hipStream_t s);

}  // namespace cda
