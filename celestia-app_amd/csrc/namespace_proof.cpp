// namespace_proof.cpp — C ABI of namespace data with completeness proofs (include/cda.h).
//
//   cda_square_prove_namespace nmt ProveNamespace of any row or column tree: the namespace's shares with an inclusion
//                              proof, or an absence or an empty proof, many queries per launch
//   cda_nmt_verify_namespace[_device]   nmt Proof.VerifyNamespace (completeness included) of a batch
// The host checks arguments and copies; which nodes make a proof and every hash are namespace_kernels.hip's.
// Staging, the two forms of the verifier and the workspace as in sampling.cpp.
#include <hip/hip_runtime.h>

#include "ctx.h"
#include "namespace_proof.h"
#include "nmt_verify_rule.h"

using namespace cda;

namespace {

NsVerifyArgs ns_verify_args(const void* descs, const void* namespaces, const void* roots, const void* nodes,
                            const void* leaf_hashes, const void* leaves, void* ok, uint32_t nproofs, uint32_t nroots,
                            uint32_t nnodes_total, uint32_t nleaf_hashes, uint32_t nleaves_total) {
  return NsVerifyArgs{(const cda_nmt_ns_proof_desc*)descs, (const uint8_t*)namespaces, (const uint8_t*)roots,
                      (const uint8_t*)nodes, (const uint8_t*)leaf_hashes, (const uint8_t*)leaves, (uint8_t*)ok,
                      nproofs, nroots, nnodes_total, nleaf_hashes, nleaves_total};
}
bool missing(const NsVerifyArgs& a) {
  return !a.descs || !a.namespaces || !a.ok || (a.nroots && !a.roots) || (a.nnodes_total && !a.nodes) ||
         (a.nleaf_hashes && !a.leaf_hashes) || (a.nleaves_total && !a.leaves);
}
int ns_verify_core(cda_ctx* c, NsVerifyArgs& a, Arena ws, hipStream_t s) {
  ns_verify_workspace(a, ws);
  ProfScope ps(c, "nmt_verify_namespace", s);
  return launch_nmt_verify_namespace(a, s) ? CDA_E_DEVICE : CDA_OK;
}

}  // namespace

extern "C" {

int cda_square_prove_namespace(cda_square* sq, uint32_t nq, const cda_namespace_query* q, uint32_t max_nodes,
                               cda_namespace_result* results, uint8_t* nodes, uint8_t* leaf_hashes,
                               uint8_t* shares_or_null, uint64_t shares_cap, uint64_t* nshares_total) {
  cda_ctx* c = sq ? sq->c : nullptr;
  CDA_API_TRY
  if (nshares_total) *nshares_total = 0;
  if (!c || !nshares_total) return CDA_E_ARG;  // null, or a square whose context was freed
  if (nq == 0) return CDA_OK;
  if (!q || !results || !nodes || !leaf_hashes) return CDA_E_ARG;
  if (nq > (1u << 24)) return CDA_E_UNSUPPORTED;
  const uint32_t w = 2 * sq->k;
  if (max_nodes < 2 * (uint32_t)sq->view.log2w) return CDA_E_ARG;
  for (uint32_t i = 0; i < nq; i++)
    if (q[i].axis > 1 || q[i].index >= w) return CDA_E_ARG;
  if ((uint64_t)nq * w > 0xFFFFFFFFull) return CDA_E_UNSUPPORTED;  // share offsets are 32-bit
  Lock l(c);
  hipStream_t s = c->stream;
  // staging in the context's workspace: queries | results | leaf hashes | the share total, the nodes, the shares
  const size_t nodes_b = (size_t)nq * max_nodes * CDA_NODE_SIZE;
  const cda_namespace_query* d_q = nullptr;
  cda_namespace_result* d_res = nullptr;
  uint8_t* d_lh = nullptr;
  unsigned long long* d_total = nullptr;
  auto lay = [&](Stage& st) {
    d_q = st.stage(q, nq);
    d_res = st.ar.take<cda_namespace_result>(nq);
    d_lh = st.ar.take<uint8_t>((size_t)nq * CDA_NODE_SIZE);
    d_total = st.ar.take<unsigned long long>(1);
  };
  int rc;
  if ((rc = ensure(c, c->plan, staged_bytes(lay))) || (rc = ensure(c, c->nodes, nodes_b))) return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  {
    ProfScope ps(c, "square_prove_namespace", s);
    if (launch_square_prove_namespace(sq->view, d_q, nq, max_nodes, d_res, (uint8_t*)c->nodes.p, d_lh, d_total, s))
      return CDA_E_DEVICE;
  }
  // How many shares the namespaces hold is the data's to say: with the shares wanted the host waits here, once, for
  // the total that sizes their staging; without them the total comes back with everything else.
  unsigned long long total = 0;
  if (!dev_ok(c, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, s), "D2H")) return CDA_E_DEVICE;
  bool fits = true;
  size_t shares_b = 0;
  if (shares_or_null) {
    if (!dev_ok(c, hipStreamSynchronize(s), "sync")) return CDA_E_DEVICE;
    *nshares_total = total;
    fits = total * CDA_SHARE <= shares_cap;
    shares_b = fits ? (size_t)total * CDA_SHARE : 0;
    if (shares_b) {
      if ((rc = ensure(c, c->payload, shares_b))) return rc;
      ProfScope ps(c, "namespace_shares", s);
      if (launch_namespace_shares(sq->view, d_q, nq, d_res, (uint8_t*)c->payload.p, s)) return CDA_E_DEVICE;
    }
  }
  if (!copy_any(c, results, d_res, (size_t)nq * sizeof(cda_namespace_result), s) ||
      !copy_any(c, nodes, c->nodes.p, nodes_b, s) || !copy_any(c, leaf_hashes, d_lh, (size_t)nq * CDA_NODE_SIZE, s) ||
      !copy_any(c, shares_or_null, c->payload.p, shares_b, s) || !dev_ok(c, hipStreamSynchronize(s), "sync"))
    return CDA_E_DEVICE;
  *nshares_total = total;
  flush_profile(c);
  return fits ? CDA_OK : CDA_E_ARG;
  CDA_API_CATCH(c)
}

int cda_nmt_verify_namespace(cda_ctx* c, uint32_t nproofs, const cda_nmt_ns_proof_desc* descs,
                             const uint8_t* namespaces, const uint8_t* roots, uint32_t nroots, const uint8_t* nodes,
                             uint32_t nnodes_total, const uint8_t* leaf_hashes, uint32_t nleaf_hashes,
                             const uint8_t* leaves, uint32_t nleaves_total, uint8_t* ok) {
  CDA_API_TRY
  if (!c) return CDA_E_ARG;
  if (nproofs == 0) return CDA_OK;
  const NsVerifyArgs h = ns_verify_args(descs, namespaces, roots, nodes, leaf_hashes, leaves, ok, nproofs, nroots,
                                        nnodes_total, nleaf_hashes, nleaves_total);
  if (missing(h)) return CDA_E_ARG;
  for (uint32_t i = 0; i < nproofs; i++)
    if (descs[i].end > kVerifyMaxEnd) return CDA_E_ARG;
  Lock l(c);
  hipStream_t s = c->stream;
  const size_t nodes_b = (size_t)nnodes_total * CDA_NODE_SIZE, leaves_b = (size_t)nleaves_total * CDA_SHARE;
  NsVerifyArgs a = h;  // the same call on the staged copies; the kernels' workspace follows the leaf hashes
  auto lay = [&](Stage& st) {
    a.descs = st.stage(h.descs, nproofs);
    a.namespaces = st.stage(h.namespaces, (size_t)nproofs * CDA_NAMESPACE_SIZE);
    a.ok = st.ar.take<uint8_t>(nproofs);
    a.roots = st.stage(h.roots, (size_t)nroots * CDA_NODE_SIZE);
    a.leaf_hashes = st.stage(h.leaf_hashes, (size_t)nleaf_hashes * CDA_NODE_SIZE);
  };
  int rc;
  if ((rc = ensure(c, c->plan, staged_bytes(lay) + workspace_bytes(a, ns_verify_workspace))) ||
      (rc = ensure(c, c->nodes, nodes_b)) || (rc = ensure(c, c->payload, leaves_b)))
    return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  a.nodes = (const uint8_t*)c->nodes.p;
  a.leaves = (const uint8_t*)c->payload.p;
  if (nodes_b && (rc = staged_h2d(c, c->nodes.p, nodes, nodes_b, s))) return rc;
  if (leaves_b && (rc = staged_h2d(c, c->payload.p, leaves, leaves_b, s))) return rc;
  if ((rc = ns_verify_core(c, a, st.ar, s))) return rc;
  return verdicts_back(c, ok, a.ok, nproofs, s);
  CDA_API_CATCH(c)
}

int cda_nmt_verify_namespace_device(cda_ctx* c, uint32_t nproofs, const void* d_descs, const void* d_namespaces,
                                    const void* d_roots, uint32_t nroots, const void* d_nodes, uint32_t nnodes_total,
                                    const void* d_leaf_hashes, uint32_t nleaf_hashes, const void* d_leaves,
                                    uint32_t nleaves_total, void* d_ok, void* stream) {
  CDA_API_TRY
  if (!c) return CDA_E_ARG;
  if (nproofs == 0) return CDA_OK;
  NsVerifyArgs a = ns_verify_args(d_descs, d_namespaces, d_roots, d_nodes, d_leaf_hashes, d_leaves, d_ok, nproofs,
                                  nroots, nnodes_total, nleaf_hashes, nleaves_total);
  if (missing(a)) return CDA_E_ARG;
  // the kernels read shares 16 bytes and nodes, roots, leaf hashes and descriptors 4 bytes at a time
  if (((uintptr_t)d_leaves & 15) ||
      (((uintptr_t)d_nodes | (uintptr_t)d_roots | (uintptr_t)d_leaf_hashes | (uintptr_t)d_descs) & 3))
    return CDA_E_ARG;
  DevLock dl(c, (hipStream_t)stream);
  if (int rc = ensure(c, c->plan, workspace_bytes(a, ns_verify_workspace))) return rc;
  return ns_verify_core(c, a, Arena(c->plan.p), dl.s);
  CDA_API_CATCH(c)
}

}  // extern "C"
