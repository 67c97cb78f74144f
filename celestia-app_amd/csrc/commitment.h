// commitment.h — what commitment.cpp (the C ABI of cda_square_commitment_proofs and cda_commitment_proofs_verify*) and
// commitment_kernels.hip share: the prover's outputs, the verifier's arguments and workspace, the launches.
#pragma once
#include "sampling.h"

namespace cda {

// A run of commitment row records whose subtree roots, in order, make one RFC-6962 set (a blob's commitment): the
// prover states one per query, the verifier's prep kernel one per proof that passed C0-C4 (live = 0: not folded).
struct CommitSet {
  uint32_t row0, nrows, nroots, live;
};
// cda_square_commitment_proofs' outputs, all device memory (include/cda.h).  rows, root_base (per row record: the
// subtree roots of its set before it), subtree_roots and commitments are always written; the others are null when
// only the commitments are wanted.
struct CommitProofsOut {
  cda_commitment_row* rows;
  uint32_t* root_base;
  uint8_t* subtree_roots;
  uint8_t* nodes;
  uint8_t* row_roots;
  uint8_t* leaf_hashes;
  uint8_t* aunts;
  uint8_t* commitments;
};
// d_row_off / d_root_off: nq + 1 words each (row records / subtree roots of the queries before q); d_sets: nq
int launch_square_commitment_proofs(const SquareView& v, const cda_blob_range* d_q, uint32_t nq, uint32_t threshold,
                                    const uint32_t* d_row_off, const uint32_t* d_root_off, const CommitSet* d_sets,
                                    uint32_t nrows, uint32_t nroots, uint32_t max_nodes, const CommitProofsOut& out,
                                    hipStream_t s);

// cda_commitment_proofs_verify's arguments, all device memory (include/cda.h), and its workspace
struct CommitVerifyArgs {
  const cda_commitment_proof_desc* descs;
  const cda_commitment_row* rows;
  const uint8_t* row_roots;
  const uint8_t* leaf_hashes;
  const uint8_t* nodes;
  const uint8_t* subtree_roots;
  const uint8_t* aunts;
  const uint8_t* data_roots;
  const uint8_t* commitments;
  int32_t* verdicts;
  uint32_t nproofs, nrows, nnodes, nsubroots, naunts, nroots, ncommitments;
  // workspace.  Per proof: the verdict of C0-C4, its subtree roots as one set, the set's RFC-6962 root and whether
  // every root of it was found, the row-proof leg's descriptor (its data root).  Per row record: the proof that owns
  // it (~0: none), how many claim it, the roots of its proof before it, W (0: the legs leave the record alone), the
  // row-proof leg's record, the verdicts of C5, C6 and C7.
  int32_t* pre;
  CommitSet* sets;
  uint32_t* got;
  uint32_t* got_ok;
  cda_share_proof_desc* sp_descs;
  uint32_t* owner;
  uint32_t* claims;
  uint32_t* root_base;
  uint32_t* row_w;
  cda_share_row* sp_rows;
  uint8_t* ns_ok;
  uint8_t* row_ok;
  uint8_t* fold_ok;
};
// The layout, from a.nproofs and a.nrows.  As validate_workspace (share_proof.h): one memset from `pre` clears all of
// it.
inline void commit_verify_workspace(CommitVerifyArgs& a, Arena& ws) {
  const size_t n = a.nrows;
  a.pre = ws.take<int32_t>(a.nproofs);
  a.sets = ws.take<CommitSet>(a.nproofs);
  a.got = ws.take<uint32_t>((size_t)a.nproofs * 8);
  a.got_ok = ws.take<uint32_t>(a.nproofs);
  a.sp_descs = ws.take<cda_share_proof_desc>(a.nproofs);
  a.owner = ws.take<uint32_t>(n);
  a.claims = ws.take<uint32_t>(n);
  a.root_base = ws.take<uint32_t>(n);
  a.row_w = ws.take<uint32_t>(n);
  a.sp_rows = ws.take<cda_share_row>(n);
  a.ns_ok = ws.take<uint8_t>(n);
  a.row_ok = ws.take<uint8_t>(n);
  a.fold_ok = ws.take<uint8_t>(n);
}
// prep (C0-C4), the namespaces (C5), the row proofs (C6: launch_row_proof_verify), the folds (C7: a chain kernel and a
// workgroup kernel), the commitments (C8), combine; prof: the context, for the per-leg profile scopes
int launch_commitment_proofs_verify(const CommitVerifyArgs& a, void* prof, hipStream_t s);

}  // namespace cda
