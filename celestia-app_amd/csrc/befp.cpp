// befp.cpp — C ABI of the bad-encoding fraud proofs (include/cda.h): batched Validate of proofs that an
// axis of a committed square is not a Reed-Solomon codeword (specs fraud_proofs.md; rsmt2d ErrByzantineData is what
// cda_repair reports as CDA_E_BYZANTINE).  The host checks arguments and copies; every check of a proof is the
// kernels': befp_kernels.hip around the verify launch and the completion of the axes (complete_axes, axis_half.h) the
// library already has, on one stream with no host wait between them.
#include <hip/hip_runtime.h>

#include "axis_half.h"
#include "befp.h"
#include "ctx.h"

using namespace cda;

namespace {

// The arguments of a call as the caller gave them: host pointers in the host form, device pointers in the _device form.
BefpArgs befp_args(uint32_t k, uint32_t nproofs, const void* descs, const void* entries, uint32_t nentries,
                   const void* shares, const void* nodes, uint32_t nnodes_total, const void* roots, uint32_t nroots,
                   void* verdicts) {
  return BefpArgs{(const cda_befp_desc*)descs, (const cda_befp_entry*)entries, (const uint8_t*)shares,
                  (const uint8_t*)nodes, (const uint8_t*)roots, (int32_t*)verdicts, k, nproofs, nentries,
                  nnodes_total, nroots};
}
// the sections a call may not leave out
bool missing(const BefpArgs& a) {
  return !a.descs || !a.verdicts || (a.nentries && (!a.entries || !a.shares)) || (a.nnodes_total && !a.nodes) ||
         (a.nroots && !a.roots);
}
size_t axes_bytes(const BefpArgs& a) { return (size_t)a.nproofs * 2 * a.k * CDA_SHARE; }

// What both forms end in once every pointer of `a` is device memory: the workspace bound at `ws`, the axis buffers
// [nproofs][2k][512] in c->scratch (the caller has sized both), the seven launches.
int enqueue_befp(cda_ctx* c, BefpArgs& a, Arena ws, hipStream_t s) {
  befp_workspace(a, ws);
  a.axes = (uint8_t*)c->scratch.p;
  const uint32_t slots = a.nproofs * 2 * a.k;
  {
    ProfScope ps(c, "befp_prep", s);
    if (launch_befp_prep(a, s)) return CDA_E_DEVICE;
  }
  {
    const VerifyArgs n{a.nmt_descs, a.nmt_ns, a.roots, a.nodes, a.shares, a.nmt_ok, slots, a.nroots, a.nnodes_total,
                       a.nentries};
    ProfScope ps(c, "befp_nmt_verify", s);
    if (launch_nmt_verify(n, false, s)) return CDA_E_DEVICE;
  }
  {
    ProfScope ps(c, "befp_gather", s);
    if (launch_befp_gather(a, s)) return CDA_E_DEVICE;
  }
  if (int rc = complete_axes(c, AxisBufs{a.axes, a.cw_off, a.cw_stride, a.mask, a.axis_idx, a.recs, a.status},
                             a.nproofs, a.k, true,
                             AxisScopes{"befp_rs_decode", "befp_rs_encode8", "befp_rs_encode16", "befp_axis_roots"}, s))
    return rc;
  {
    ProfScope ps(c, "befp_combine", s);
    if (launch_befp_combine(a, s)) return CDA_E_DEVICE;
  }
  return CDA_OK;
}

}  // namespace

extern "C" {

int cda_befp_validate(cda_ctx* c, uint32_t k, uint32_t nproofs, const cda_befp_desc* descs,
                      const cda_befp_entry* entries, uint32_t nentries, const uint8_t* shares, const uint8_t* nodes,
                      uint32_t nnodes_total, const uint8_t* roots, uint32_t nroots, int32_t* verdicts) {
  CDA_API_TRY
  if (!c) return CDA_E_ARG;
  if (int rc = check_axis_shape(k, nproofs, CDA_E_ARG)) return rc;
  if (nproofs == 0) return CDA_OK;
  const BefpArgs h = befp_args(k, nproofs, descs, entries, nentries, shares, nodes, nnodes_total, roots, nroots,
                               verdicts);
  if (missing(h)) return CDA_E_ARG;
  Lock l(c);
  hipStream_t s = c->stream;
  const size_t nodes_b = (size_t)nnodes_total * CDA_NODE_SIZE, shares_b = (size_t)nentries * CDA_SHARE;
  BefpArgs a = h;  // the same call on the staged copies; the kernels' workspace follows the verdicts
  auto lay = [&](Stage& st) {
    a.descs = st.stage(h.descs, nproofs);
    a.entries = st.stage(h.entries, nentries);
    a.roots = st.stage(h.roots, (size_t)nroots * CDA_NODE_SIZE);
    a.verdicts = st.ar.take<int32_t>(nproofs);
  };
  int rc;
  if ((rc = ensure(c, c->plan, staged_bytes(lay) + workspace_bytes(a, befp_workspace))) ||
      (rc = ensure(c, c->nodes, nodes_b)) || (rc = ensure(c, c->payload, shares_b)) ||
      (rc = ensure(c, c->scratch, axes_bytes(a))))
    return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  a.nodes = (const uint8_t*)c->nodes.p;
  a.shares = (const uint8_t*)c->payload.p;
  if (nodes_b && (rc = staged_h2d(c, c->nodes.p, nodes, nodes_b, s))) return rc;
  if (shares_b && (rc = staged_h2d(c, c->payload.p, shares, shares_b, s))) return rc;
  if ((rc = enqueue_befp(c, a, st.ar, s))) return rc;
  return verdicts_back(c, verdicts, a.verdicts, (size_t)nproofs * 4, s);
  CDA_API_CATCH(c)
}

int cda_befp_validate_device(cda_ctx* c, uint32_t k, uint32_t nproofs, const void* d_descs, const void* d_entries,
                             uint32_t nentries, const void* d_shares, const void* d_nodes, uint32_t nnodes_total,
                             const void* d_roots, uint32_t nroots, void* d_verdicts, void* stream) {
  CDA_API_TRY
  if (!c) return CDA_E_ARG;
  if (int rc = check_axis_shape(k, nproofs, CDA_E_ARG)) return rc;
  if (nproofs == 0) return CDA_OK;
  BefpArgs a = befp_args(k, nproofs, d_descs, d_entries, nentries, d_shares, d_nodes, nnodes_total, d_roots, nroots,
                         d_verdicts);
  if (missing(a)) return CDA_E_ARG;
  // shares are read 16 bytes at a time, everything else in 4-byte words
  if (((uintptr_t)d_shares & 15) || (((uintptr_t)d_descs | (uintptr_t)d_entries | (uintptr_t)d_nodes |
                                      (uintptr_t)d_roots | (uintptr_t)d_verdicts) & 3))
    return CDA_E_ARG;
  DevLock dl(c, (hipStream_t)stream);
  int rc;
  if ((rc = ensure(c, c->plan, workspace_bytes(a, befp_workspace))) || (rc = ensure(c, c->scratch, axes_bytes(a))))
    return rc;
  return enqueue_befp(c, a, Arena(c->plan.p), dl.s);
  CDA_API_CATCH(c)
}

}  // extern "C"
