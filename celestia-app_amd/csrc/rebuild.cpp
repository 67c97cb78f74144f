// rebuild.cpp — C ABI of a square rebuilt from proved samples (include/cda.h): the step between
// cda_nmt_verify and cda_repair, and the chain around it.
//
//   cda_samples_assemble_device   verify + place, every pointer device memory: the accepted cells into a square with
//                                 its presence map, a status per sample (sample_place_rule.h)
//   cda_square_open_eds_device    cda_square_open_eds for a square already in this GPU's memory
//   cda_square_rebuild            samples in host memory -> a retained square: stage, assemble into the handle's EDS
//                                 area, rsmt2d Repair there, commit in place
// rsmt2d has no assemble step (its Repair is handed a square with holes); the placement rule is this library's.  The
// repair is repair.cpp's and the commitment sampling.cpp's, both unchanged.  The host checks arguments and copies;
// every check of a sample is the kernels': rebuild_kernels.hip around launch_nmt_verify.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ctx.h"
#include "rebuild.h"

using namespace cda;

namespace cda {

// ---- the head and the tail of a rebuild (rebuild.h): what cda_square_rebuild and cda_square_rebuild_axes share ----
RebuildHost::RebuildHost(uint32_t k, const uint8_t* rr, const uint8_t* cr, uint8_t* present_or_null)
    : row_roots(rr), col_roots(cr), roots(4 * (size_t)k * CDA_NODE_SIZE),
      own_present(present_or_null ? 0 : 4 * (size_t)k * k),
      present(present_or_null ? present_or_null : own_present.data()) {
  const size_t roots_b = 2 * (size_t)k * CDA_NODE_SIZE;
  memcpy(roots.data(), rr, roots_b);
  memcpy(roots.data() + roots_b, cr, roots_b);
}

int rebuild_finish(cda_ctx* c, uint32_t k, SquareBuild& b, const uint8_t* d_present, const uint8_t* d_statuses,
                   uint32_t n, uint8_t* statuses, RebuildHost& h, uint8_t* eds_or_null, cda_square** out, uint8_t* dah,
                   cda_err_info* err, const char* call, hipStream_t s) {
  const size_t cells = 4 * (size_t)k * k, roots_b = h.roots.size() / 2;
  int rc;
  // the presence map and the statuses back in one wait: the repair plans on the host
  if (!dev_ok(c, hipMemcpyAsync(h.present, d_present, cells, hipMemcpyDeviceToHost, s), "D2H") ||
      (n && !dev_ok(c, hipMemcpyAsync(statuses, d_statuses, n, hipMemcpyDeviceToHost, s), "D2H")) ||
      !dev_ok(c, hipStreamSynchronize(s), "sync"))
    return CDA_E_DEVICE;
  flush_profile(c);
  const int repaired = repair_resident(c, k, b.eds, h.present, h.row_roots, h.col_roots, err, s);
  if (repaired != CDA_OK && repaired != CDA_E_UNREPAIRABLE && repaired != CDA_E_BYZANTINE) return repaired;
  // the square as far as rsmt2d got (cda_repair's return), or the repaired one
  if (eds_or_null && (rc = staged_d2h(c, eds_or_null, b.eds, b.eds_b, s))) return rc;
  if (repaired != CDA_OK) return repaired;  // `b` releases the handle's memory
  std::vector<uint8_t> got(2 * roots_b);
  if ((rc = square_commit(c, k, b, out, got.data(), got.data() + roots_b, dah, err, s))) return rc;
  // an OK repair has checked every axis against its root
  if (memcmp(got.data(), h.roots.data(), h.roots.size()) != 0) {
    cda_square_close(*out);
    *out = nullptr;
    c->last_err = std::string(call) + ": the repaired square does not commit to the given roots";
    return CDA_E_INTERNAL;
  }
  return CDA_OK;
}

}  // namespace cda

namespace {

constexpr uint32_t kMaxSamples = 1u << 24;  // as the proof calls' query counts

// k and nsamples of a call
int check_shape(uint32_t k, uint32_t nsamples) {
  if (!is_pow2(k)) return CDA_E_NOT_POW2;
  if (k > kMaxDeviceK || nsamples > kMaxSamples) return CDA_E_UNSUPPORTED;
  return CDA_OK;
}

// The arguments of a call as the caller gave them: host pointers in cda_square_rebuild (where eds, present and
// statuses are bound later), device pointers in the _device form.
AssembleArgs assemble_args(uint32_t k, uint32_t nsamples, const void* descs, const void* shares, const void* nodes,
                           uint32_t nnodes_total, const void* roots, void* eds, void* present, void* statuses) {
  return AssembleArgs{(const cda_sample_desc*)descs, (const uint8_t*)shares, (const uint8_t*)nodes,
                      (const uint8_t*)roots,         (uint8_t*)eds,          (uint8_t*)present,
                      (uint8_t*)statuses,            k,                      nsamples,
                      nnodes_total};
}
// the sections a call may not leave out (the outputs and the roots are checked by each form)
bool missing(const AssembleArgs& a) {
  return (a.nsamples && (!a.descs || !a.shares || !a.statuses)) || (a.nnodes_total && !a.nodes);
}
size_t cells_of(uint32_t k) { return 4 * (size_t)k * k; }

// What both forms end in once every pointer of `a` is device memory: the square and its presence map cleared (an
// unplaced cell is zero, as in the repair's sparse upload), the workspace bound at `ws`, then prep, the verifier of
// one-leaf proofs, claim and place.
int assemble_core(cda_ctx* c, AssembleArgs& a, Arena ws, hipStream_t s) {
  assemble_workspace(a, ws);
  const size_t cells = cells_of(a.k);
  if (!dev_ok(c, hipMemsetAsync(a.eds, 0, cells * CDA_SHARE, s), "memset") ||
      !dev_ok(c, hipMemsetAsync(a.present, 0, cells, s), "memset"))
    return CDA_E_DEVICE;
  if (a.nsamples == 0) return CDA_OK;
  if (!dev_ok(c, hipMemsetAsync(a.owner, 0xFF, cells * sizeof(uint32_t), s), "memset")) return CDA_E_DEVICE;
  {
    ProfScope ps(c, "sample_prep", s);
    if (launch_sample_prep(a, s)) return CDA_E_DEVICE;
  }
  {
    const VerifyArgs n{a.nmt_descs, a.nmt_ns, a.roots, a.nodes, a.shares, a.ok, a.nsamples, 4 * a.k, a.nnodes_total,
                       a.nsamples};
    ProfScope ps(c, "sample_nmt_verify", s);
    if (launch_nmt_verify(n, false, s)) return CDA_E_DEVICE;
  }
  {
    ProfScope ps(c, "sample_claim", s);
    if (launch_sample_claim(a, s)) return CDA_E_DEVICE;
  }
  {
    ProfScope ps(c, "sample_place", s);
    if (launch_sample_place(a, s)) return CDA_E_DEVICE;
  }
  return CDA_OK;
}

}  // namespace

extern "C" {

int cda_samples_assemble_device(cda_ctx* c, uint32_t k, uint32_t nsamples, const void* d_descs, const void* d_shares,
                                const void* d_nodes, uint32_t nnodes_total, const void* d_roots, void* d_eds,
                                void* d_present, void* d_statuses, void* stream) {
  CDA_API_TRY
  if (!c) return CDA_E_ARG;
  AssembleArgs a = assemble_args(k, nsamples, d_descs, d_shares, d_nodes, nnodes_total, d_roots, d_eds, d_present,
                                 d_statuses);
  if (missing(a) || !d_roots || !d_eds || !d_present) return CDA_E_ARG;
  if (int rc = check_shape(k, nsamples)) return rc;
  // shares and cells move 16 bytes at a time, everything else is read in 4-byte words
  if ((((uintptr_t)d_shares | (uintptr_t)d_eds) & 15) ||
      (((uintptr_t)d_descs | (uintptr_t)d_nodes | (uintptr_t)d_roots | (uintptr_t)d_present | (uintptr_t)d_statuses) &
       3))
    return CDA_E_ARG;
  DevLock dl(c, (hipStream_t)stream);
  if (int rc = ensure(c, c->plan, workspace_bytes(a, assemble_workspace))) return rc;
  return assemble_core(c, a, Arena(c->plan.p), dl.s);
  CDA_API_CATCH(c)
}

int cda_square_open_eds_device(cda_ctx* c, uint32_t k, const void* d_eds, cda_square** out, uint8_t* row_roots,
                               uint8_t* col_roots, uint8_t* dah, cda_err_info* err, void* stream) {
  CDA_API_TRY
  set_err(err, CDA_OK, -1, -1, -1, -1);
  if (out) *out = nullptr;
  if (!c || !d_eds || !out || !row_roots || !col_roots || !dah || ((uintptr_t)d_eds & 15)) return CDA_E_ARG;
  if (int rc = check_shape(k, 0)) return rc;
  DevLock dl(c, (hipStream_t)stream);
  SquareBuild b;
  if (int rc = square_alloc(c, k, b, dl.s)) return rc;
  if (!dev_ok(c, hipMemcpyAsync(b.eds, d_eds, b.eds_b, hipMemcpyDeviceToDevice, dl.s), "D2D")) return CDA_E_DEVICE;
  return square_commit(c, k, b, out, row_roots, col_roots, dah, err, dl.s);
  CDA_API_CATCH(c)
}

int cda_square_rebuild(cda_ctx* c, uint32_t k, uint32_t nsamples, const cda_sample_desc* descs, const uint8_t* shares,
                       const uint8_t* nodes, uint32_t nnodes_total, const uint8_t* row_roots, const uint8_t* col_roots,
                       cda_square** out, uint8_t* statuses, uint8_t* present_or_null, uint8_t* eds_or_null,
                       uint8_t* dah, cda_err_info* err) {
  CDA_API_TRY
  set_err(err, CDA_OK, -1, -1, -1, -1);
  if (out) *out = nullptr;
  if (!c || !out || !row_roots || !col_roots || !dah) return CDA_E_ARG;
  const AssembleArgs h = assemble_args(k, nsamples, descs, shares, nodes, nnodes_total, nullptr, nullptr, nullptr,
                                       statuses);
  if (missing(h)) return CDA_E_ARG;
  if (int rc = check_shape(k, nsamples)) return rc;
  const size_t cells = cells_of(k);
  RebuildHost host(k, row_roots, col_roots, present_or_null);
  Lock l(c);
  hipStream_t s = c->stream;
  int rc;
  // the handle's memory first: the samples are assembled straight into its EDS area
  SquareBuild b;
  if ((rc = square_alloc(c, k, b, s))) return rc;
  // staging in the context's workspace: descriptors | roots | statuses | presence map, then the kernels' workspace;
  // the nodes and the shares
  const size_t nodes_b = (size_t)nnodes_total * CDA_NODE_SIZE, shares_b = (size_t)nsamples * CDA_SHARE;
  AssembleArgs a = h;  // the same call on the staged copies
  a.eds = b.eds;
  auto lay = [&](Stage& st) {
    a.descs = st.stage(h.descs, nsamples);
    a.roots = st.stage(host.roots.data(), host.roots.size());
    a.statuses = st.ar.take<uint8_t>(nsamples);
    a.present = st.ar.take<uint8_t>(cells);
  };
  if ((rc = ensure(c, c->plan, staged_bytes(lay) + workspace_bytes(a, assemble_workspace))) ||
      (rc = ensure(c, c->nodes, nodes_b)) || (rc = ensure(c, c->payload, shares_b)))
    return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  a.nodes = (const uint8_t*)c->nodes.p;
  a.shares = (const uint8_t*)c->payload.p;
  if (nodes_b && (rc = staged_h2d(c, c->nodes.p, nodes, nodes_b, s))) return rc;
  if (shares_b && (rc = staged_h2d(c, c->payload.p, shares, shares_b, s))) return rc;
  if ((rc = assemble_core(c, a, st.ar, s))) return rc;
  return rebuild_finish(c, k, b, a.present, a.statuses, nsamples, statuses, host, eds_or_null, out, dah, err,
                        "cda_square_rebuild", s);
  CDA_API_CATCH(c)
}

}  // extern "C"
