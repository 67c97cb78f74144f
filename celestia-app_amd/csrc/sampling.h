// sampling.h — what sampling.cpp (the C ABI of cda_square_* and cda_nmt_verify*) and sampling_kernels.hip share, and
// what befp.cpp (cda_befp_validate*) and befp_kernels.hip share with them and with each other: the argument structs
// the kernels take, the layouts of the verifiers' workspaces and the launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cda.h"
#include "arena.h"
#include "cda_internal.h"

namespace cda {

// The device memory of a retained square (one allocation owned by its cda_square):
//   eds     (2k)^2 cells of 512 B, row-major
//   leaf    (2k)^2 leaf records of 96 B, cell-major (a cell's leaf is the same node in its row and its column tree)
//   levels  the records of tree levels 1 .. log2(2k), each level [tree][node] with trees 0..2k-1 the rows and
//           2k..4k-1 the columns (launch_nmt_level's layout); level h starts square_level_offset(log2w, h) records in
//   dah_nodes  the RFC-6962 tree over rowRoots ‖ colRoots, 8k - 1 digests of 32 B: the 4k leaf hashes, then each
//           level, the data root last (cda_extend_commit_nodes' dah_nodes)
struct SquareView {
  const uint8_t* eds;
  const uint8_t* leaf;
  const uint8_t* levels;
  int log2w;
  const uint8_t* dah_nodes;
};
// records of levels 1 .. h - 1 of the 4k trees: 2w (w / 2 + .. + w >> (h - 1))
__host__ __device__ inline size_t square_level_offset(int log2w, int h) {
  const size_t w = (size_t)1 << log2w;
  return 2 * w * (w - (w >> (h - 1)));
}

}  // namespace cda

struct cda_square {
  cda_ctx* c = nullptr;  // null once the context was freed
  uint32_t k = 0;
  void* mem = nullptr;  // eds | leaf records | level records | data-root tree (SquareView)
  cda::SquareView view{};
};

namespace cda {

// A square being built (sampling.cpp): square_alloc makes the handle and its one allocation and sets the order-status
// word to "no error"; the caller puts the EDS into `eds` on `s` (the k x k ODS may pass through `levels`, which the
// extension has read before level 1 is written); square_commit commits what lies there (leaf hash, levels, DAH and
// data-root tree), brings the roots back in its one wait and hands the handle out.  Until then the destructor
// releases the half-built square, on every failure path (an exception included).  Lock held throughout.
struct SquareBuild {
  cda_square* sq = nullptr;
  uint8_t* eds = nullptr;
  uint8_t* leaf = nullptr;
  uint8_t* levels = nullptr;
  uint8_t* meta = nullptr;  // status [0, 8) | dah [256, 288) | data-root tree [512, ..)
  size_t eds_b = 0;
  SquareBuild() = default;
  SquareBuild(const SquareBuild&) = delete;
  SquareBuild& operator=(const SquareBuild&) = delete;
  ~SquareBuild();
};
int square_alloc(cda_ctx* c, uint32_t k, SquareBuild& b, hipStream_t s);
int square_commit(cda_ctx* c, uint32_t k, SquareBuild& b, cda_square** out, uint8_t* row_roots, uint8_t* col_roots,
                  uint8_t* dah, cda_err_info* err, hipStream_t s);

// cda_nmt_verify's arguments, all device memory (include/cda.h)
struct VerifyArgs {
  const cda_nmt_proof_desc* descs;
  const uint8_t* namespaces;
  const uint8_t* roots;
  const uint8_t* nodes;
  const uint8_t* leaves;
  uint8_t* ok;
  uint32_t nproofs, nroots, nnodes_total, nleaves_total;
};

// d_share_off (nq words of scratch) and d_shares: both null when the cells are not wanted
int launch_square_prove(const SquareView& v, const cda_range_query* d_q, uint32_t nq, uint32_t max_nodes,
                        int32_t* d_counts, uint8_t* d_nodes, uint32_t* d_share_off, uint8_t* d_shares, hipStream_t s);
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

// cda_share_proofs_validate's arguments, all device memory (include/cda.h), and its workspace.  Each workspace of this
// header has one statement of its layout, a walk over an Arena (arena.h): on a measuring arena it sizes the workspace,
// on the buffer it points the struct's workspace fields into it.
template <class Args>
size_t workspace_bytes(Args a, void (*layout)(Args&, Arena&)) {  // a: the counts the layout reads
  Arena measure;
  layout(a, measure);
  return measure.used();
}
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
// The layout, from a.nproofs and a.nrows.  As validate_workspace: one memset from `pre` clears all of it.
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
// prep (C0-C4), the namespaces (C5), the row proofs (C6: row_proof_verify_kernel), the folds (C7: a chain kernel and a
// workgroup kernel), the commitments (C8), combine; prof: the context, for the per-leg profile scopes
int launch_commitment_proofs_verify(const CommitVerifyArgs& a, void* prof, hipStream_t s);

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

// ranges = false: no descriptor has more than one leaf (the kernel of the longer proofs is not launched)
int launch_nmt_verify(const VerifyArgs& a, bool ranges, hipStream_t s);

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

}  // namespace cda
