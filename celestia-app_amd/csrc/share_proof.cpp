// share_proof.cpp — C ABI of the share proofs to the data root (include/cda.h).
//
//   cda_square_share_proofs    pkg/proof NewShareInclusionProof (proof.go:55-167) for many share ranges per launch:
//                              NMT range proofs, row roots and their RFC-6962 proofs in the data root
//   cda_share_proofs_validate[_device]  ShareProof.Validate (share_proof.go:16-82, row_proof.go:13-48) of a batch
// The host checks arguments and copies; which nodes make a proof and every hash are share_proof_kernels.hip's.
// Staging, the two forms of the verifier and the workspace as in sampling.cpp.
#include <hip/hip_runtime.h>

#include <vector>

#include "ctx.h"
#include "share_proof.h"

using namespace cda;

namespace {

ValidateArgs validate_args(const void* descs, const void* rows, const void* row_roots, const void* leaf_hashes,
                           const void* nodes, const void* aunts, const void* leaves, const void* data_roots,
                           void* verdicts, uint32_t nproofs, uint32_t nrows, uint32_t nnodes, uint32_t naunts,
                           uint32_t nleaves, uint32_t nroots) {
  return ValidateArgs{(const cda_share_proof_desc*)descs, (const cda_share_row*)rows, (const uint8_t*)row_roots,
                      (const uint8_t*)leaf_hashes, (const uint8_t*)nodes, (const uint8_t*)aunts,
                      (const uint8_t*)leaves, (const uint8_t*)data_roots, (int32_t*)verdicts, nproofs, nrows, nnodes,
                      naunts, nleaves, nroots};
}
bool missing(const ValidateArgs& a) {
  return !a.descs || !a.verdicts || (a.nrows && (!a.rows || !a.row_roots || !a.leaf_hashes)) ||
         (a.nnodes && !a.nodes) || (a.naunts && !a.aunts) || (a.nleaves && !a.leaves) || (a.nroots && !a.data_roots);
}
int share_validate_core(cda_ctx* c, ValidateArgs& a, Arena ws, hipStream_t s) {
  validate_workspace(a, ws);
  ProfScope ps(c, "share_proofs_validate", s);
  return launch_share_proofs_validate(a, s) ? CDA_E_DEVICE : CDA_OK;
}

}  // namespace

extern "C" {

int cda_square_share_proofs(cda_square* sq, uint32_t nq, const cda_share_range* q, uint32_t max_nodes,
                            uint32_t rows_cap, uint32_t* row_off, cda_share_row* rows, uint8_t* nodes,
                            uint8_t* row_roots, uint8_t* leaf_hashes, uint8_t* aunts, uint8_t* shares_or_null,
                            uint64_t shares_cap, uint8_t* data_root) {
  cda_ctx* c = sq ? sq->c : nullptr;
  CDA_API_TRY
  if (!c) return CDA_E_ARG;  // null, or a square whose context was freed
  if (nq == 0) return CDA_OK;
  if (!q || !row_off || !rows || !nodes || !row_roots || !leaf_hashes || !aunts || !data_root) return CDA_E_ARG;
  if (nq > (1u << 24)) return CDA_E_UNSUPPORTED;
  const uint32_t k = sq->k, naunts = (uint32_t)sq->view.log2w + 1;
  if (max_nodes < 2 * (uint32_t)sq->view.log2w) return CDA_E_ARG;
  // the queries against the square, and the sizes of the outputs: where each query's row records and shares start
  std::vector<uint32_t> off(2 * (size_t)nq + 1);  // row_off (nq + 1) | share_off (nq)
  uint64_t nrows = 0, nshares = 0;
  for (uint32_t i = 0; i < nq; i++) {
    if (q[i].start >= q[i].end || q[i].end > k * k) return CDA_E_ARG;
    if (nrows > 0xFFFFFFFFull || nshares > 0xFFFFFFFFull) return CDA_E_UNSUPPORTED;
    off[i] = (uint32_t)nrows;
    off[nq + 1 + i] = (uint32_t)nshares;
    nrows += (q[i].end - 1) / k - q[i].start / k + 1;
    nshares += q[i].end - q[i].start;
  }
  if (nrows > rows_cap || (shares_or_null && nshares * CDA_SHARE > shares_cap)) return CDA_E_ARG;
  if ((nrows * max_nodes) >> 32 || (nrows * naunts) >> 32 || nshares > 0xFFFFFFFFull) return CDA_E_UNSUPPORTED;
  off[nq] = (uint32_t)nrows;
  Lock l(c);
  hipStream_t s = c->stream;
  // staging in the context's workspace: queries | offsets | row records | row roots | leaf hashes | aunts, the nodes,
  // the shares
  const size_t aunts_b = nrows * naunts * 32;
  const size_t nodes_b = nrows * max_nodes * CDA_NODE_SIZE, shares_b = shares_or_null ? nshares * CDA_SHARE : 0;
  const cda_share_range* d_q = nullptr;
  const uint32_t* d_off = nullptr;
  ShareProofsOut o{};
  auto lay = [&](Stage& st) {
    d_q = st.stage(q, nq);
    d_off = st.stage(off.data(), off.size());
    o.rows = st.ar.take<cda_share_row>(nrows);
    o.row_roots = st.ar.take<uint8_t>(nrows * CDA_NODE_SIZE);
    o.leaf_hashes = st.ar.take<uint8_t>(nrows * 32);
    o.aunts = st.ar.take<uint8_t>(aunts_b);
  };
  int rc;
  if ((rc = ensure(c, c->plan, staged_bytes(lay))) || (rc = ensure(c, c->nodes, nodes_b)) ||
      (shares_b && (rc = ensure(c, c->payload, shares_b))))
    return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  o.nodes = (uint8_t*)c->nodes.p;
  o.shares = shares_b ? (uint8_t*)c->payload.p : nullptr;
  {
    ProfScope ps(c, "square_share_proofs", s);
    if (launch_square_share_proofs(sq->view, d_q, nq, d_off, d_off + nq + 1, (uint32_t)nrows, max_nodes, o, s))
      return CDA_E_DEVICE;
  }
  const uint8_t* d_root = sq->view.dah_nodes + (2 * (size_t)(4 * k) - 2) * 32;  // the last node of the tree
  if (!copy_any(c, row_off, d_off, ((size_t)nq + 1) * 4, s) ||
      !copy_any(c, rows, o.rows, nrows * sizeof(cda_share_row), s) || !copy_any(c, nodes, o.nodes, nodes_b, s) ||
      !copy_any(c, row_roots, o.row_roots, nrows * CDA_NODE_SIZE, s) ||
      !copy_any(c, leaf_hashes, o.leaf_hashes, nrows * 32, s) || !copy_any(c, aunts, o.aunts, aunts_b, s) ||
      !copy_any(c, shares_or_null, o.shares, shares_b, s) || !copy_any(c, data_root, d_root, 32, s) ||
      !dev_ok(c, hipStreamSynchronize(s), "sync"))
    return CDA_E_DEVICE;
  flush_profile(c);
  return CDA_OK;
  CDA_API_CATCH(c)
}

int cda_share_proofs_validate(cda_ctx* c, uint32_t nproofs, const cda_share_proof_desc* descs,
                              const cda_share_row* rows, const uint8_t* row_roots, const uint8_t* leaf_hashes,
                              uint32_t nrows, const uint8_t* nodes, uint32_t nnodes, const uint8_t* aunts,
                              uint32_t naunts, const uint8_t* leaves, uint32_t nleaves, const uint8_t* data_roots,
                              uint32_t nroots, int32_t* verdicts) {
  CDA_API_TRY
  if (!c) return CDA_E_ARG;
  if (nproofs == 0) return CDA_OK;
  const ValidateArgs h = validate_args(descs, rows, row_roots, leaf_hashes, nodes, aunts, leaves, data_roots, verdicts,
                                       nproofs, nrows, nnodes, naunts, nleaves, nroots);
  if (missing(h)) return CDA_E_ARG;
  Lock l(c);
  hipStream_t s = c->stream;
  const size_t nodes_b = (size_t)nnodes * CDA_NODE_SIZE, leaves_b = (size_t)nleaves * CDA_SHARE;
  ValidateArgs a = h;  // the same call on the staged copies; the kernels' workspace follows the verdicts
  auto lay = [&](Stage& st) {
    a.descs = st.stage(h.descs, nproofs);
    a.rows = st.stage(h.rows, nrows);
    a.row_roots = st.stage(h.row_roots, (size_t)nrows * CDA_NODE_SIZE);
    a.leaf_hashes = st.stage(h.leaf_hashes, (size_t)nrows * 32);
    a.aunts = st.stage(h.aunts, (size_t)naunts * 32);
    a.data_roots = st.stage(h.data_roots, (size_t)nroots * 32);
    a.verdicts = st.ar.take<int32_t>(nproofs);
  };
  int rc;
  if ((rc = ensure(c, c->plan, staged_bytes(lay) + workspace_bytes(a, validate_workspace))) ||
      (rc = ensure(c, c->nodes, nodes_b)) || (rc = ensure(c, c->payload, leaves_b)))
    return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  a.nodes = (const uint8_t*)c->nodes.p;
  a.leaves = (const uint8_t*)c->payload.p;
  if (nodes_b && (rc = staged_h2d(c, c->nodes.p, nodes, nodes_b, s))) return rc;
  if (leaves_b && (rc = staged_h2d(c, c->payload.p, leaves, leaves_b, s))) return rc;
  if ((rc = share_validate_core(c, a, st.ar, s))) return rc;
  return verdicts_back(c, verdicts, a.verdicts, (size_t)nproofs * 4, s);
  CDA_API_CATCH(c)
}

int cda_share_proofs_validate_device(cda_ctx* c, uint32_t nproofs, const void* d_descs, const void* d_rows,
                                     const void* d_row_roots, const void* d_leaf_hashes, uint32_t nrows,
                                     const void* d_nodes, uint32_t nnodes, const void* d_aunts, uint32_t naunts,
                                     const void* d_leaves, uint32_t nleaves, const void* d_data_roots,
                                     uint32_t nroots, void* d_verdicts, void* stream) {
  CDA_API_TRY
  if (!c) return CDA_E_ARG;
  if (nproofs == 0) return CDA_OK;
  ValidateArgs a = validate_args(d_descs, d_rows, d_row_roots, d_leaf_hashes, d_nodes, d_aunts, d_leaves, d_data_roots,
                                 d_verdicts, nproofs, nrows, nnodes, naunts, nleaves, nroots);
  if (missing(a)) return CDA_E_ARG;
  // shares are read 16 bytes at a time, row records hold 64-bit fields, everything else is read in 4-byte words
  if (((uintptr_t)d_leaves & 15) || ((uintptr_t)d_rows & 7) ||
      (((uintptr_t)d_descs | (uintptr_t)d_row_roots | (uintptr_t)d_leaf_hashes | (uintptr_t)d_nodes |
        (uintptr_t)d_aunts | (uintptr_t)d_data_roots | (uintptr_t)d_verdicts) & 3))
    return CDA_E_ARG;
  DevLock dl(c, (hipStream_t)stream);
  if (int rc = ensure(c, c->plan, workspace_bytes(a, validate_workspace))) return rc;
  return share_validate_core(c, a, Arena(c->plan.p), dl.s);
  CDA_API_CATCH(c)
}

}  // extern "C"
