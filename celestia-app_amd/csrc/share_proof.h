// share_proof.h — what share_proof.cpp (the C ABI of cda_square_share_proofs and cda_share_proofs_validate*) and
// share_proof_kernels.hip share: the prover's outputs, the verifier's arguments and workspace, the launches.  The
// row-proof leg's launch is also the commitment verifier's (commitment_kernels.hip).
#pragma once
#include "sampling.h"

namespace cda {

// cda_square_share_proofs' outputs, all device memory (include/cda.h); shares null when the cells are not wanted
struct ShareProofsOut {
  cda_share_row* rows;
  uint8_t* nodes;
  uint8_t* row_roots;
  uint8_t* leaf_hashes;
  uint8_t* aunts;
  uint8_t* shares;
};
// d_row_off: nq + 1 words, d_share_off: nq words (the shares of the queries before q); nrows = d_row_off[nq]
int launch_square_share_proofs(const SquareView& v, const cda_share_range* d_q, uint32_t nq, const uint32_t* d_row_off,
                               const uint32_t* d_share_off, uint32_t nrows, uint32_t max_nodes,
                               const ShareProofsOut& out, hipStream_t s);

// cda_share_proofs_validate's arguments, all device memory (include/cda.h), and its workspace
struct ValidateArgs {
  const cda_share_proof_desc* descs;
  const cda_share_row* rows;
  const uint8_t* row_roots;
  const uint8_t* leaf_hashes;
  const uint8_t* nodes;
  const uint8_t* aunts;
  const uint8_t* leaves;
  const uint8_t* data_roots;
  int32_t* verdicts;
  uint32_t nproofs, nrows, nnodes, naunts, nleaves, nroots;
  // workspace: per proof the verdict of the counting checks; per row record the proof that owns it (~0: none), how
  // many proofs claim it, the NMT leg's descriptor, namespace and verdict, the row-proof leg's verdict
  int32_t* pre;
  uint32_t* owner;
  uint32_t* claims;
  cda_nmt_proof_desc* nmt_descs;
  uint8_t* nmt_ns;
  uint8_t* nmt_ok;
  uint8_t* row_ok;
};
// The layout, from a.nproofs and a.nrows.  launch_share_proofs_validate clears the whole of it in one memset that
// starts at its first slot, `pre`: a slot added here is cleared with the others, and none may come before `pre`.
inline void validate_workspace(ValidateArgs& a, Arena& ws) {
  const size_t n = a.nrows;
  a.pre = ws.take<int32_t>(a.nproofs);
  a.owner = ws.take<uint32_t>(n);
  a.claims = ws.take<uint32_t>(n);
  a.nmt_descs = ws.take<cda_nmt_proof_desc>(n);
  a.nmt_ns = ws.take<uint8_t>(n * CDA_NAMESPACE_SIZE);
  a.nmt_ok = ws.take<uint8_t>(n);
  a.row_ok = ws.take<uint8_t>(n);
}
// the three legs: counting checks and NMT descriptors, launch_nmt_verify over the row records, one Proof.Verify per
// lane; then the per-proof verdict
int launch_share_proofs_validate(const ValidateArgs& a, hipStream_t s);
// the row-proof leg alone, a lane per row record: it reads descs[].data_root, rows, row_roots, leaf_hashes, aunts,
// data_roots, the counts and owner, and writes row_ok
int launch_row_proof_verify(const ValidateArgs& a, hipStream_t s);

}  // namespace cda
