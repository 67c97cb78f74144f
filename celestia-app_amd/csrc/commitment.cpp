// commitment.cpp — C ABI of the blob commitment proofs (include/cda.h): "the blob with share commitment C
// is in the block with data root R", proved without the blob's shares (ADR-011's blob inclusion proof).
//
//   cda_commitment_proof_sizes           the row records and subtree roots a prover call writes
//   cda_square_commitment_proofs         many blobs of a retained square per call: the subtree roots out of the retained
//                                        levels, their range proofs and row proofs, and the commitments (GetCommitment,
//                                        pkg/inclusion/get_commit.go) hashed on the device in the same call
//   cda_commitment_proofs_verify[_device]  rules C0-C8 of a batch
// The host checks arguments against commitment_rule.h, sizes and copies; which nodes make a proof and every hash are
// commitment_kernels.hip's.  Staging, the two forms of the verifier and the workspace as in sampling.cpp.
#include <hip/hip_runtime.h>

#include <vector>

#include "commitment.h"
#include "commitment_rule.h"
#include "ctx.h"

using namespace cda;

namespace {

// A blob's range against the k x k ODS and the rule.  false: the prover rejects it.
struct BlobPlan {
  uint32_t nrows, nroots;
};
bool plan_blob(uint32_t k, uint32_t threshold, const cda_blob_range& q, BlobPlan& p) {
  if (q.len == 0 || threshold == 0) return false;
  const uint64_t end = (uint64_t)q.start + q.len;
  if (end > (uint64_t)k * k) return false;
  const uint32_t W = sub_tree_width(q.len, threshold);
  if (W > k || q.start % W) return false;
  const uint32_t r0 = q.start / k, r1 = (uint32_t)((end - 1) / k), s0 = q.start % k, e1 = (uint32_t)((end - 1) % k) + 1;
  p.nrows = r1 - r0 + 1;
  if (r0 == r1) {
    p.nroots = subtree_tile_count(s0, e1, W);
  } else {
    const uint64_t n = (uint64_t)subtree_tile_count(s0, k, W) + (uint64_t)(p.nrows - 2) * (k / W) +
                       subtree_tile_count(0, e1, W);
    if (n > 0xFFFFFFFFull) return false;
    p.nroots = (uint32_t)n;
  }
  return true;
}

CommitVerifyArgs commit_verify_args(const void* descs, const void* rows, const void* row_roots, const void* leaf_hashes,
                                    const void* nodes, const void* subtree_roots, const void* aunts,
                                    const void* data_roots, const void* commitments, void* verdicts, uint32_t nproofs,
                                    uint32_t nrows, uint32_t nnodes, uint32_t nsubroots, uint32_t naunts,
                                    uint32_t nroots, uint32_t ncommitments) {
  CommitVerifyArgs a{};
  a.descs = (const cda_commitment_proof_desc*)descs;
  a.rows = (const cda_commitment_row*)rows;
  a.row_roots = (const uint8_t*)row_roots;
  a.leaf_hashes = (const uint8_t*)leaf_hashes;
  a.nodes = (const uint8_t*)nodes;
  a.subtree_roots = (const uint8_t*)subtree_roots;
  a.aunts = (const uint8_t*)aunts;
  a.data_roots = (const uint8_t*)data_roots;
  a.commitments = (const uint8_t*)commitments;
  a.verdicts = (int32_t*)verdicts;
  a.nproofs = nproofs;
  a.nrows = nrows;
  a.nnodes = nnodes;
  a.nsubroots = nsubroots;
  a.naunts = naunts;
  a.nroots = nroots;
  a.ncommitments = ncommitments;
  return a;
}
bool missing(const CommitVerifyArgs& a) {
  return !a.descs || !a.verdicts || (a.nrows && (!a.rows || !a.row_roots || !a.leaf_hashes)) ||
         (a.nnodes && !a.nodes) || (a.nsubroots && !a.subtree_roots) || (a.naunts && !a.aunts) ||
         (a.nroots && !a.data_roots) || (a.ncommitments && !a.commitments);
}
int commit_verify_core(cda_ctx* c, CommitVerifyArgs& a, Arena ws, hipStream_t s) {
  commit_verify_workspace(a, ws);
  return launch_commitment_proofs_verify(a, c, s) ? CDA_E_DEVICE : CDA_OK;
}

}  // namespace

extern "C" {

int cda_commitment_proof_sizes(uint32_t k, uint32_t subtree_root_threshold, uint32_t nq, const cda_blob_range* q,
                               uint64_t* nrows, uint64_t* nroots) {
  if (nrows) *nrows = 0;
  if (nroots) *nroots = 0;
  if (!nrows || !nroots || (nq && !q)) return CDA_E_ARG;
  if (!is_pow2(k)) return CDA_E_NOT_POW2;
  if (k > kCommitMaxK) return CDA_E_ARG;
  uint64_t r = 0, t = 0;
  for (uint32_t i = 0; i < nq; i++) {
    BlobPlan p;
    if (!plan_blob(k, subtree_root_threshold, q[i], p)) return CDA_E_ARG;
    r += p.nrows;
    t += p.nroots;
  }
  *nrows = r;
  *nroots = t;
  return CDA_OK;
}

int cda_square_commitment_proofs(cda_square* sq, uint32_t nq, const cda_blob_range* q,
                                 uint32_t subtree_root_threshold, uint32_t max_nodes, uint32_t rows_cap,
                                 uint32_t roots_cap, uint32_t* row_off, cda_commitment_row* rows, uint8_t* nodes,
                                 uint8_t* subtree_roots, uint8_t* row_roots, uint8_t* leaf_hashes, uint8_t* aunts,
                                 uint8_t* commitments, uint8_t* data_root) {
  cda_ctx* c = sq ? sq->c : nullptr;
  CDA_API_TRY
  if (!c) return CDA_E_ARG;  // null, or a square whose context was freed
  if (nq == 0) return CDA_OK;
  if (!q || !commitments) return CDA_E_ARG;
  const bool proofs = row_off || rows || nodes || subtree_roots || row_roots || leaf_hashes || aunts || data_root;
  if (proofs && (!row_off || !rows || !nodes || !subtree_roots || !row_roots || !leaf_hashes || !aunts || !data_root))
    return CDA_E_ARG;
  if (nq > (1u << 24)) return CDA_E_UNSUPPORTED;
  const uint32_t k = sq->k, naunts = (uint32_t)sq->view.log2w + 1;
  if (proofs && max_nodes < 2 * (uint32_t)sq->view.log2w) return CDA_E_ARG;
  // the queries against the square and the rule, and the sizes of the outputs: where each query's row records and
  // subtree roots start, and its roots as one set of the commitment kernel
  std::vector<uint32_t> off(2 * ((size_t)nq + 1));  // row_off (nq + 1) | root_off (nq + 1)
  std::vector<CommitSet> sets(nq);
  uint64_t nrows = 0, nroots = 0;
  bool too_many = false;
  for (uint32_t i = 0; i < nq; i++) {
    BlobPlan p;
    if (!plan_blob(k, subtree_root_threshold, q[i], p)) return CDA_E_ARG;
    too_many = too_many || p.nroots > kCommitMaxRoots || nrows > 0xFFFFFFFFull || nroots > 0xFFFFFFFFull;
    off[i] = (uint32_t)nrows;
    off[nq + 1 + i] = (uint32_t)nroots;
    sets[i] = CommitSet{(uint32_t)nrows, p.nrows, p.nroots, 1u};
    nrows += p.nrows;
    nroots += p.nroots;
  }
  if (proofs && (nrows > rows_cap || nroots > roots_cap)) return CDA_E_ARG;
  if (!proofs) max_nodes = 0;
  if (too_many || nrows > 0xFFFFFFFFull || nroots > 0xFFFFFFFFull || (nrows * max_nodes) >> 32 || (nrows * naunts) >> 32)
    return CDA_E_UNSUPPORTED;
  off[nq] = (uint32_t)nrows;
  off[2 * (size_t)nq + 1] = (uint32_t)nroots;
  Lock l(c);
  hipStream_t s = c->stream;
  // staging in the context's workspace: queries | offsets | sets | row records | root bases | commitments | row roots |
  // leaf hashes | aunts, the nodes, the subtree roots
  const size_t aunts_b = proofs ? nrows * naunts * 32 : 0, nodes_b = nrows * max_nodes * CDA_NODE_SIZE;
  const size_t roots_b = nroots * CDA_NODE_SIZE;
  const cda_blob_range* d_q = nullptr;
  const uint32_t* d_off = nullptr;
  const CommitSet* d_sets = nullptr;
  CommitProofsOut o{};
  auto lay = [&](Stage& st) {
    d_q = st.stage(q, nq);
    d_off = st.stage(off.data(), off.size());
    d_sets = st.stage(sets.data(), sets.size());
    o.rows = st.ar.take<cda_commitment_row>(nrows);
    o.root_base = st.ar.take<uint32_t>(nrows);
    o.commitments = st.ar.take<uint8_t>((size_t)nq * 32);
    if (!proofs) return;
    o.row_roots = st.ar.take<uint8_t>(nrows * CDA_NODE_SIZE);
    o.leaf_hashes = st.ar.take<uint8_t>(nrows * 32);
    o.aunts = st.ar.take<uint8_t>(aunts_b);
  };
  int rc;
  if ((rc = ensure(c, c->plan, staged_bytes(lay))) || (nodes_b && (rc = ensure(c, c->nodes, nodes_b))) ||
      (rc = ensure(c, c->payload, roots_b)))
    return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  o.nodes = proofs ? (uint8_t*)c->nodes.p : nullptr;
  o.subtree_roots = (uint8_t*)c->payload.p;
  {
    ProfScope ps(c, "square_commitment_proofs", s);
    if (launch_square_commitment_proofs(sq->view, d_q, nq, subtree_root_threshold, d_off, d_off + nq + 1, d_sets,
                                        (uint32_t)nrows, (uint32_t)nroots, max_nodes, o, s))
      return CDA_E_DEVICE;
  }
  const uint8_t* d_root = sq->view.dah_nodes + (2 * (size_t)(4 * k) - 2) * 32;  // the last node of the tree
  if (!copy_any(c, commitments, o.commitments, (size_t)nq * 32, s)) return CDA_E_DEVICE;
  if (proofs && (!copy_any(c, row_off, d_off, ((size_t)nq + 1) * 4, s) ||
                 !copy_any(c, rows, o.rows, nrows * sizeof(cda_commitment_row), s) ||
                 !copy_any(c, nodes, o.nodes, nodes_b, s) || !copy_any(c, subtree_roots, o.subtree_roots, roots_b, s) ||
                 !copy_any(c, row_roots, o.row_roots, nrows * CDA_NODE_SIZE, s) ||
                 !copy_any(c, leaf_hashes, o.leaf_hashes, nrows * 32, s) || !copy_any(c, aunts, o.aunts, aunts_b, s) ||
                 !copy_any(c, data_root, d_root, 32, s)))
    return CDA_E_DEVICE;
  if (!dev_ok(c, hipStreamSynchronize(s), "sync")) return CDA_E_DEVICE;
  flush_profile(c);
  return CDA_OK;
  CDA_API_CATCH(c)
}

int cda_commitment_proofs_verify(cda_ctx* c, uint32_t nproofs, const cda_commitment_proof_desc* descs,
                                 const cda_commitment_row* rows, const uint8_t* row_roots, const uint8_t* leaf_hashes,
                                 uint32_t nrows, const uint8_t* nodes, uint32_t nnodes, const uint8_t* subtree_roots,
                                 uint32_t nsubtree_roots, const uint8_t* aunts, uint32_t naunts,
                                 const uint8_t* data_roots, uint32_t nroots, const uint8_t* commitments,
                                 uint32_t ncommitments, int32_t* verdicts) {
  CDA_API_TRY
  if (!c) return CDA_E_ARG;
  if (nproofs == 0) return CDA_OK;
  const CommitVerifyArgs h = commit_verify_args(descs, rows, row_roots, leaf_hashes, nodes, subtree_roots, aunts,
                                                data_roots, commitments, verdicts, nproofs, nrows, nnodes,
                                                nsubtree_roots, naunts, nroots, ncommitments);
  if (missing(h)) return CDA_E_ARG;
  Lock l(c);
  hipStream_t s = c->stream;
  const size_t nodes_b = (size_t)nnodes * CDA_NODE_SIZE, roots_b = (size_t)nsubtree_roots * CDA_NODE_SIZE;
  CommitVerifyArgs a = h;  // the same call on the staged copies; the kernels' workspace follows the verdicts
  auto lay = [&](Stage& st) {
    a.descs = st.stage(h.descs, nproofs);
    a.rows = st.stage(h.rows, nrows);
    a.row_roots = st.stage(h.row_roots, (size_t)nrows * CDA_NODE_SIZE);
    a.leaf_hashes = st.stage(h.leaf_hashes, (size_t)nrows * 32);
    a.aunts = st.stage(h.aunts, (size_t)naunts * 32);
    a.data_roots = st.stage(h.data_roots, (size_t)nroots * 32);
    a.commitments = st.stage(h.commitments, (size_t)ncommitments * 32);
    a.verdicts = st.ar.take<int32_t>(nproofs);
  };
  int rc;
  if ((rc = ensure(c, c->plan, staged_bytes(lay) + workspace_bytes(a, commit_verify_workspace))) ||
      (rc = ensure(c, c->nodes, nodes_b)) || (rc = ensure(c, c->payload, roots_b)))
    return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  a.nodes = (const uint8_t*)c->nodes.p;
  a.subtree_roots = (const uint8_t*)c->payload.p;
  if (nodes_b && (rc = staged_h2d(c, c->nodes.p, nodes, nodes_b, s))) return rc;
  if (roots_b && (rc = staged_h2d(c, c->payload.p, subtree_roots, roots_b, s))) return rc;
  if ((rc = commit_verify_core(c, a, st.ar, s))) return rc;
  return verdicts_back(c, verdicts, a.verdicts, (size_t)nproofs * 4, s);
  CDA_API_CATCH(c)
}

int cda_commitment_proofs_verify_device(cda_ctx* c, uint32_t nproofs, const void* d_descs, const void* d_rows,
                                        const void* d_row_roots, const void* d_leaf_hashes, uint32_t nrows,
                                        const void* d_nodes, uint32_t nnodes, const void* d_subtree_roots,
                                        uint32_t nsubtree_roots, const void* d_aunts, uint32_t naunts,
                                        const void* d_data_roots, uint32_t nroots, const void* d_commitments,
                                        uint32_t ncommitments, void* d_verdicts, void* stream) {
  CDA_API_TRY
  if (!c) return CDA_E_ARG;
  if (nproofs == 0) return CDA_OK;
  CommitVerifyArgs a = commit_verify_args(d_descs, d_rows, d_row_roots, d_leaf_hashes, d_nodes, d_subtree_roots, d_aunts,
                                          d_data_roots, d_commitments, d_verdicts, nproofs, nrows, nnodes,
                                          nsubtree_roots, naunts, nroots, ncommitments);
  if (missing(a)) return CDA_E_ARG;
  // row records hold 64-bit fields, everything else is read in 4-byte words
  if (((uintptr_t)d_rows & 7) ||
      (((uintptr_t)d_descs | (uintptr_t)d_row_roots | (uintptr_t)d_leaf_hashes | (uintptr_t)d_nodes |
        (uintptr_t)d_subtree_roots | (uintptr_t)d_aunts | (uintptr_t)d_data_roots | (uintptr_t)d_commitments |
        (uintptr_t)d_verdicts) & 3))
    return CDA_E_ARG;
  DevLock dl(c, (hipStream_t)stream);
  if (int rc = ensure(c, c->plan, workspace_bytes(a, commit_verify_workspace))) return rc;
  return commit_verify_core(c, a, Arena(c->plan.p), dl.s);
  CDA_API_CATCH(c)
}

}  // extern "C"
