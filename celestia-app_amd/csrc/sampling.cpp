// sampling.cpp — C ABI of the sample proofs (include/cda.h): a retained square that proves any of its cells, and
// batched nmt.Proof.VerifyInclusion.
//
//   cda_square_open / close    da.ExtendShares + NewDataAvailabilityHeader once; the EDS and every node of the 4k
//                              trees stay in device memory of the handle
//   cda_square_open_eds        the same for an EDS as it was committed: nothing is extended, the encoding not checked
//   cda_square_prove           wrapper ErasuredNamespacedMerkleTree.ProveRange (pkg/wrapper/nmt_wrapper.go:127-130) of
//                              any row or column tree, many ranges per launch
//   cda_nmt_verify[_device]    nmt Proof.VerifyInclusion as ShareProof.VerifyProof calls it
//                              (pkg/proof/share_proof.go:53-82), many proofs per launch
// The host checks arguments and copies; which nodes make a proof and every hash are sampling_kernels.hip's.  The share
// proofs and the namespace proofs of a retained square are share_proof.cpp and namespace_proof.cpp.
//
// Staging (here and in the other proof files): a call's small arrays go into slots of c->plan that one function of a
// Stage (ctx.h) states; it runs on a measuring arena to size the buffer, then on the buffer to copy.  Nodes and shares
// go through staged_h2d into c->nodes and c->payload.  A verifier's host form stages its arrays and then runs what its
// _device form runs (the *_core functions), with the kernels' workspace after its last slot.  Every ensure of a call
// comes before its first copy: ensure may move a buffer.
//
// Building a square is two steps, square_alloc and square_commit (sampling.h), with the EDS put in place between them:
// by an upload or the extension here, by a device copy or by the assembly and repair of samples in rebuild.cpp.
//
// Ownership: a square's device memory is one allocation of its own, so no other call on the context can touch it.
// The context lists its open squares; cda_free releases their device memory and detaches them (ctx = null), after
// which a handle is good for cda_square_close alone, which then only frees the host struct.  As for every other
// call, cda_free must not run concurrently with calls on the context or its squares.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "nmt_verify_rule.h"
#include "sampling.h"

using namespace cda;

namespace {

void release_square_memory(cda_square* sq) {
  if (sq->mem) (void)hipFree(sq->mem);
  sq->mem = nullptr;
}

}  // namespace

namespace cda {

void release_squares(cda_ctx* c) {
  for (cda_square* sq : c->squares) {
    release_square_memory(sq);
    sq->c = nullptr;
  }
  c->squares.clear();
}

// ---- a square being built (sampling.h): what cda_square_open, cda_square_open_eds and rebuild.cpp's calls share ----
SquareBuild::~SquareBuild() {
  if (!sq) return;
  release_square_memory(sq);
  delete sq;
}

int square_alloc(cda_ctx* c, uint32_t k, SquareBuild& b, hipStream_t s) {
  const uint32_t w = 2 * k;
  const int L = ilog2i(w);
  const size_t cells = (size_t)w * w, ods_b = (size_t)k * k * CDA_SHARE, eds_b = cells * CDA_SHARE;
  const size_t leaf_b = cells * CDA_REC_BYTES, levels_b = square_level_offset(L, L + 1) * CDA_REC_BYTES;
  // the ODS is uploaded into the level records' place: the extension has read it before level 1 is written
  // meta: status [0, 8) | dah [256, 288) | data-root tree [512, ..)
  const size_t tail_b = align256(std::max(levels_b, ods_b)), dn = 2 * (size_t)(2 * w) - 1, meta_b = 512 + dn * 32;
  b.sq = new cda_square();
  fault_point("alloc");
  if (!dev_ok(c, hipMalloc(&b.sq->mem, eds_b + align256(leaf_b) + tail_b + meta_b), "hipMalloc")) return CDA_E_DEVICE;
  b.eds = (uint8_t*)b.sq->mem;
  b.eds_b = eds_b;
  b.leaf = b.eds + eds_b;
  b.levels = b.leaf + align256(leaf_b);
  b.meta = b.levels + tail_b;
  if (!dev_ok(c, hipMemsetAsync(b.meta, 0xFF, 8, s), "memset")) return CDA_E_DEVICE;
  return CDA_OK;
}

int square_commit(cda_ctx* c, uint32_t k, SquareBuild& b, cda_square** out, uint8_t* row_roots, uint8_t* col_roots,
                  uint8_t* dah, cda_err_info* err, hipStream_t s) {
  const uint32_t w = 2 * k;
  const int L = ilog2i(w);
  cda_square* sq = b.sq;
  uint8_t* d_eds = b.eds;
  uint8_t* d_leaf = b.leaf;
  uint8_t* d_levels = b.levels;
  uint8_t* meta = b.meta;
  unsigned long long* d_status = (unsigned long long*)meta;
  uint8_t* d_dah = meta + 256;
  uint8_t* d_dnodes = meta + 512;
  auto level = [&](int h) { return d_levels + square_level_offset(L, h) * CDA_REC_BYTES; };
  int rc;
  {
    ProfScope ps(c, "leaf_hash", s);
    if (launch_leaf_hash(d_eds, d_leaf, d_status, (int)k, 1, s)) return CDA_E_DEVICE;
  }
  // the per-level path of the node export (inclusion.cpp), every level's records in a place of their own
  for (int h = 1; h <= L; h++) {
    ProfScope ps(c, h == 1 ? "nmt_level1" : "nmt_level", s);
    if (launch_nmt_level(h == 1 ? d_leaf : level(h - 1), level(h), h == 1, (int)k, 1, h, s)) return CDA_E_DEVICE;
  }
  uint8_t* d_roots = level(L);  // 2w root records, rows then columns
  {  // the DAH, and from the same launch the RFC-6962 tree over rowRoots ‖ colRoots, which stays with the square: a
     // share proof's leaf hashes and aunts
    ProfScope ps(c, "dah", s);
    const int lr = launch_dah_tree(d_roots, d_dah, d_dnodes, (int)(2 * w), s);
    if (lr) return lr == -2 ? CDA_E_UNSUPPORTED : CDA_E_DEVICE;
  }
  // the root records end the level area and the status word and the DAH follow within a few hundred bytes: one copy
  // brings all three back (three small pageable copies cost more than the launch that keeps the data-root tree)
  const size_t meta_at = (size_t)(meta - d_roots), back_b = meta_at + 288;
  std::vector<uint8_t> recs(back_b);
  uint64_t st = 0;
  if (!dev_ok(c, hipMemcpyAsync(recs.data(), d_roots, back_b, hipMemcpyDeviceToHost, s), "D2H") ||
      !dev_ok(c, hipStreamSynchronize(s), "sync"))
    return CDA_E_DEVICE;
  memcpy(&st, recs.data() + meta_at, 8);
  memcpy(dah, recs.data() + meta_at + 256, 32);
  flush_profile(c);
  pack_roots(recs.data(), w, row_roots);
  pack_roots(recs.data() + (size_t)w * CDA_REC_BYTES, w, col_roots);
  if ((rc = map_status(st, 0, err))) return rc;
  sq->c = c;
  sq->k = k;
  sq->view = SquareView{d_eds, d_leaf, d_levels, L, d_dnodes};
  c->squares.push_back(sq);
  b.sq = nullptr;
  *out = sq;
  return CDA_OK;
}

}  // namespace cda

namespace {

// What cda_square_open and cda_square_open_eds share: the handle's allocation, the EDS into it, its commitment, the
// one copy back and the handle.  extended = false: `src` is the k x k ODS and is extended into the EDS area first;
// true: `src` is the (2k)^2 EDS and is retained as it is.  Lock held.
int open_square(cda_ctx* c, uint32_t k, const uint8_t* src, bool extended, cda_square** out, uint8_t* row_roots,
                uint8_t* col_roots, uint8_t* dah, cda_err_info* err) {
  hipStream_t s = c->stream;
  SquareBuild b;
  int rc;
  if ((rc = square_alloc(c, k, b, s))) return rc;
  if (extended) {
    if ((rc = staged_h2d(c, b.eds, src, b.eds_b, s))) return rc;
  } else {
    const size_t ods_b = (size_t)k * k * CDA_SHARE;
    if (!dev_ok(c, hipMemcpyAsync(b.levels, src, ods_b, hipMemcpyHostToDevice, s), "H2D")) return CDA_E_DEVICE;
    if ((rc = enqueue_rs(c, k, 1, b.levels, b.eds, s))) return rc;
  }
  return square_commit(c, k, b, out, row_roots, col_roots, dah, err, s);
}

// ---- the verifier (as every verifier's file has them): the arguments of a call as the caller gave them (host pointers
// in the host form, device pointers in the _device form; the struct's own order), the sections a call may not leave
// out, and what both forms end in once every pointer is device memory: the launches. ----
VerifyArgs verify_args(const void* descs, const void* namespaces, const void* roots, const void* nodes,
                       const void* leaves, void* ok, uint32_t nproofs, uint32_t nroots, uint32_t nnodes_total,
                       uint32_t nleaves_total) {
  return VerifyArgs{(const cda_nmt_proof_desc*)descs, (const uint8_t*)namespaces, (const uint8_t*)roots,
                    (const uint8_t*)nodes, (const uint8_t*)leaves, (uint8_t*)ok, nproofs, nroots, nnodes_total,
                    nleaves_total};
}
bool missing(const VerifyArgs& a) {
  return !a.descs || !a.namespaces || !a.ok || (a.nroots && !a.roots) || (a.nnodes_total && !a.nodes) ||
         (a.nleaves_total && !a.leaves);
}
int nmt_verify_core(cda_ctx* c, const VerifyArgs& a, bool ranges, hipStream_t s) {
  ProfScope ps(c, "nmt_verify", s);
  return launch_nmt_verify(a, ranges, s) ? CDA_E_DEVICE : CDA_OK;
}

}  // namespace

extern "C" {

int cda_square_open(cda_ctx* c, uint32_t count, uint32_t share_len, const uint8_t* shares, cda_square** out,
                    uint8_t* row_roots, uint8_t* col_roots, uint8_t* dah, cda_err_info* err) {
  CDA_API_TRY
  set_err(err, CDA_OK, -1, -1, -1, -1);
  if (out) *out = nullptr;
  if (!c || !shares || !out || !row_roots || !col_roots || !dah) return CDA_E_ARG;
  uint32_t k = 0;
  if (int rc = square_k(count, share_len, &k, err)) return rc;
  Lock l(c);
  return open_square(c, k, shares, false, out, row_roots, col_roots, dah, err);
  CDA_API_CATCH(c)
}

int cda_square_open_eds(cda_ctx* c, uint32_t k, const uint8_t* eds, cda_square** out, uint8_t* row_roots,
                        uint8_t* col_roots, uint8_t* dah, cda_err_info* err) {
  CDA_API_TRY
  set_err(err, CDA_OK, -1, -1, -1, -1);
  if (out) *out = nullptr;
  if (!c || !eds || !out || !row_roots || !col_roots || !dah) return CDA_E_ARG;
  if (!is_pow2(k)) return CDA_E_NOT_POW2;
  if (k > kMaxDeviceK) return CDA_E_UNSUPPORTED;
  Lock l(c);
  return open_square(c, k, eds, true, out, row_roots, col_roots, dah, err);
  CDA_API_CATCH(c)
}

void cda_square_close(cda_square* sq) {
  if (!sq) return;
  try {
    if (cda_ctx* c = sq->c) {
      Lock l(c);
      (void)hipStreamSynchronize(c->stream);
      c->squares.erase(std::remove(c->squares.begin(), c->squares.end(), sq), c->squares.end());
      release_square_memory(sq);
    }
  } catch (...) {  // nothing may escape the C ABI
  }
  delete sq;
}

int cda_square_prove(cda_square* sq, uint32_t nq, const cda_range_query* q, uint32_t max_nodes, int32_t* counts,
                     uint8_t* nodes, uint8_t* shares_or_null, uint64_t shares_cap) {
  cda_ctx* c = sq ? sq->c : nullptr;
  CDA_API_TRY
  if (!c) return CDA_E_ARG;  // null, or a square whose context was freed
  if (nq == 0) return CDA_OK;
  if (!q || !counts || !nodes) return CDA_E_ARG;
  if (nq > (1u << 24)) return CDA_E_UNSUPPORTED;
  const uint32_t w = 2 * sq->k;
  if (max_nodes < 2 * (uint32_t)sq->view.log2w) return CDA_E_ARG;
  uint64_t ncells = 0;
  for (uint32_t i = 0; i < nq; i++) {
    if (q[i].axis > 1 || q[i].index >= w || q[i].start >= q[i].end || q[i].end > w) return CDA_E_ARG;
    ncells += q[i].end - q[i].start;
  }
  if (shares_or_null && ncells * CDA_SHARE > shares_cap) return CDA_E_ARG;
  if (ncells > 0xFFFFFFFFull) return CDA_E_UNSUPPORTED;
  Lock l(c);
  hipStream_t s = c->stream;
  // staging in the context's workspace: queries | counts | share offsets, the nodes, the cells
  const size_t nodes_b = (size_t)nq * max_nodes * CDA_NODE_SIZE, shares_b = shares_or_null ? ncells * CDA_SHARE : 0;
  const cda_range_query* d_q = nullptr;
  int32_t* d_counts = nullptr;
  uint32_t* d_off = nullptr;
  auto lay = [&](Stage& st) {
    d_q = st.stage(q, nq);
    d_counts = st.ar.take<int32_t>(nq);
    d_off = st.ar.take<uint32_t>(nq);
  };
  int rc;
  if ((rc = ensure(c, c->plan, staged_bytes(lay))) || (rc = ensure(c, c->nodes, nodes_b)) ||
      (shares_b && (rc = ensure(c, c->payload, shares_b))))
    return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  uint8_t* d_shares = shares_b ? (uint8_t*)c->payload.p : nullptr;
  {
    ProfScope ps(c, "square_prove", s);
    if (launch_square_prove(sq->view, d_q, nq, max_nodes, d_counts, (uint8_t*)c->nodes.p, d_shares ? d_off : nullptr,
                            d_shares, s))
      return CDA_E_DEVICE;
  }
  if (!copy_any(c, counts, d_counts, (size_t)nq * 4, s) || !copy_any(c, nodes, c->nodes.p, nodes_b, s) ||
      !copy_any(c, shares_or_null, d_shares, shares_b, s) || !dev_ok(c, hipStreamSynchronize(s), "sync"))
    return CDA_E_DEVICE;
  flush_profile(c);
  return CDA_OK;
  CDA_API_CATCH(c)
}

int cda_nmt_verify(cda_ctx* c, uint32_t nproofs, const cda_nmt_proof_desc* descs, const uint8_t* namespaces,
                   const uint8_t* roots, uint32_t nroots, const uint8_t* nodes, uint32_t nnodes_total,
                   const uint8_t* leaves, uint32_t nleaves_total, uint8_t* ok) {
  CDA_API_TRY
  if (!c) return CDA_E_ARG;
  if (nproofs == 0) return CDA_OK;
  const VerifyArgs h = verify_args(descs, namespaces, roots, nodes, leaves, ok, nproofs, nroots, nnodes_total,
                                   nleaves_total);
  if (missing(h)) return CDA_E_ARG;
  bool ranges = false;
  for (uint32_t i = 0; i < nproofs; i++) {
    if (descs[i].end > kVerifyMaxEnd) return CDA_E_ARG;
    ranges = ranges || (descs[i].start < descs[i].end && descs[i].end - descs[i].start > 1);
  }
  Lock l(c);
  hipStream_t s = c->stream;
  const size_t nodes_b = (size_t)nnodes_total * CDA_NODE_SIZE, leaves_b = (size_t)nleaves_total * CDA_SHARE;
  VerifyArgs a = h;  // the same call on the staged copies
  auto lay = [&](Stage& st) {
    a.descs = st.stage(h.descs, nproofs);
    a.namespaces = st.stage(h.namespaces, (size_t)nproofs * CDA_NAMESPACE_SIZE);
    a.ok = st.ar.take<uint8_t>(nproofs);
    a.roots = st.stage(h.roots, (size_t)nroots * CDA_NODE_SIZE);
  };
  int rc;
  if ((rc = ensure(c, c->plan, staged_bytes(lay))) || (rc = ensure(c, c->nodes, nodes_b)) ||
      (rc = ensure(c, c->payload, leaves_b)))
    return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  a.nodes = (const uint8_t*)c->nodes.p;
  a.leaves = (const uint8_t*)c->payload.p;
  if (nodes_b && (rc = staged_h2d(c, c->nodes.p, nodes, nodes_b, s))) return rc;
  if (leaves_b && (rc = staged_h2d(c, c->payload.p, leaves, leaves_b, s))) return rc;
  if ((rc = nmt_verify_core(c, a, ranges, s))) return rc;
  return verdicts_back(c, ok, a.ok, nproofs, s);
  CDA_API_CATCH(c)
}

int cda_nmt_verify_device(cda_ctx* c, uint32_t nproofs, const void* d_descs, const void* d_namespaces,
                          const void* d_roots, uint32_t nroots, const void* d_nodes, uint32_t nnodes_total,
                          const void* d_leaves, uint32_t nleaves_total, void* d_ok, void* stream) {
  CDA_API_TRY
  if (!c) return CDA_E_ARG;
  if (nproofs == 0) return CDA_OK;
  const VerifyArgs a = verify_args(d_descs, d_namespaces, d_roots, d_nodes, d_leaves, d_ok, nproofs, nroots,
                                   nnodes_total, nleaves_total);
  if (missing(a)) return CDA_E_ARG;
  // the kernels read shares 16 bytes and nodes, roots and descriptors 4 bytes at a time
  if (((uintptr_t)d_leaves & 15) || (((uintptr_t)d_nodes | (uintptr_t)d_roots | (uintptr_t)d_descs) & 3))
    return CDA_E_ARG;
  DevLock dl(c, (hipStream_t)stream);
  // the descriptors are device memory: whether any proof has more than one leaf is not known here
  return nmt_verify_core(c, a, true, dl.s);
  CDA_API_CATCH(c)
}

}  // extern "C"
