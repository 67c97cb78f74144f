// axis_half.cpp — C ABI of the row and column halves (include/cda.h): celestia-node's shwap.Row, k
// consecutive cells of an axis sent with no proof, which the receiver checks by completing the axis with the codec
// and comparing the wrapper tree's root with the committed one (Row.Verify).
//
//   cda_square_axis_halves            serve halves out of a retained square
//   cda_axis_halves_verify[_device]   batched Row.Verify: a status per half, the completed axes on request
//   cda_axis_halves_assemble_device   verify + place, every pointer device memory (axis_half_rule.h)
//   cda_square_rebuild_axes           halves in host memory -> a retained square: stage, assemble into the handle's
//                                     EDS area, rsmt2d Repair there, commit in place
// The host checks arguments and copies; every check of a half is the kernels': axis_half_kernels.hip around the
// decode, encode and axis-root launches the library already has (complete_axes, which befp.cpp runs too), on one
// stream with no host wait between them.  The repair and the commitment of a rebuild are rebuild.cpp's
// rebuild_finish, shared with cda_square_rebuild.
#include <hip/hip_runtime.h>

#include "axis_half.h"
#include "ctx.h"
#include "rebuild.h"

using namespace cda;

namespace cda {

int check_axis_shape(uint32_t k, uint32_t n, int not_pow2) {
  if (!is_pow2(k)) return not_pow2;
  if (2 * (uint64_t)k > (uint64_t)kAxisRootsMaxLeaves) return CDA_E_UNSUPPORTED;
  if ((uint64_t)n * 2 * k > 0x7FFFFFFFull) return CDA_E_UNSUPPORTED;  // slots are 32-bit, launches take int
  return CDA_OK;
}

int complete_axes(cda_ctx* c, const AxisBufs& b, uint32_t n, uint32_t k, bool decode, const AxisScopes& scopes,
                  hipStream_t s) {
  const uint32_t w = 2 * k;
  int lr;
  if (decode) {
    ProfScope ps(c, scopes.decode, s);
    if ((lr = launch_rs_decode(b.axes, b.cw_off, b.cw_stride, b.mask, (int)n, (int)k, CDA_SHARE, s)))
      return code_of(lr);
  }
  {  // slots [k, 2k) of every buffer := Encode(slots [0, k)); of a decoded axis that is what was sent
    RsJob j{};
    j.src = b.axes;
    j.src_cw = (long long)w * CDA_SHARE;
    j.src_sh = CDA_SHARE;
    j.dst = b.axes + (size_t)k * CDA_SHARE;
    j.dst_cw = (long long)w * CDA_SHARE;
    j.dst_sh = CDA_SHARE;
    j.k = (int)k;
    j.cw_per_blk = (int)n;
    j.nblk = 1;
    j.shard_len = CDA_SHARE;
    const bool ff8 = w <= 256;
    ProfScope ps(c, ff8 ? scopes.encode8 : scopes.encode16, s);
    if ((lr = ff8 ? launch_rs_encode8(j, s) : launch_rs_encode16(j, s))) return code_of(lr);
  }
  {
    ProfScope ps(c, scopes.roots, s);
    if ((lr = launch_axis_roots(b.axes, (long long)w * CDA_SHARE, (int)w, k, b.axis_idx, (int)n, b.recs, b.status, s)))
      return code_of(lr);
  }
  return CDA_OK;
}

}  // namespace cda

namespace {

// The arguments of a call as the caller gave them: host pointers in the host forms (where the outputs are bound
// later), device pointers in the _device forms.
AxisHalfArgs half_args(uint32_t k, uint32_t nhalves, const void* descs, const void* shares, const void* roots,
                       uint32_t nroots, void* statuses, bool assembling) {
  AxisHalfArgs a{};
  a.descs = (const cda_axis_half_desc*)descs;
  a.shares = (const uint8_t*)shares;
  a.roots = (const uint8_t*)roots;
  a.statuses = (uint8_t*)statuses;
  a.k = k;
  a.nhalves = nhalves;
  a.nroots = nroots;
  a.assembling = assembling;
  return a;
}
// the sections a call may not leave out (the square's outputs are checked by each form)
bool missing(const AxisHalfArgs& a) {
  return (a.nhalves && (!a.descs || !a.shares || !a.statuses)) || (a.nroots && !a.roots);
}
size_t axes_bytes(const AxisHalfArgs& a) { return (size_t)a.nhalves * 2 * a.k * CDA_SHARE; }
size_t shares_bytes(const AxisHalfArgs& a) { return (size_t)a.nhalves * a.k * CDA_SHARE; }
size_t cells_of(uint32_t k) { return 4 * (size_t)k * k; }
bool any_second_side(const cda_axis_half_desc* descs, uint32_t n) {
  for (uint32_t p = 0; p < n; p++)
    if (descs[p].side == CDA_SIDE_SECOND) return true;
  return false;
}

// H0-H2 once every pointer of `a` is device memory, the workspace is bound and a.axes points at nhalves x 2k x 512 B
// (the caller has sized both): the six launches.  decode: some half may be a second side (a device form cannot know);
// slots [0, k) of the second sides' buffers := Decode(slots [k, 2k)).
int verify_core(cda_ctx* c, const AxisHalfArgs& a, bool decode, hipStream_t s) {
  {
    ProfScope ps(c, "axis_half_prep", s);
    if (launch_axis_half_prep(a, s)) return CDA_E_DEVICE;
  }
  {
    ProfScope ps(c, "axis_half_scatter", s);
    if (launch_axis_half_scatter(a, s)) return CDA_E_DEVICE;
  }
  if (int rc = complete_axes(c, AxisBufs{a.axes, a.cw_off, a.cw_stride, a.mask, a.axis_idx, a.recs, a.status},
                             a.nhalves, a.k, decode,
                             AxisScopes{"axis_half_rs_decode", "axis_half_rs_encode8", "axis_half_rs_encode16",
                                        "axis_half_axis_roots"},
                             s))
    return rc;
  {
    ProfScope ps(c, "axis_half_combine", s);
    if (launch_axis_half_combine(a, s)) return CDA_E_DEVICE;
  }
  return CDA_OK;
}

// Verify and place: the square and its presence map cleared (an unplaced cell is zero, as in the repair's sparse
// upload), H0-H2, then claim and place.
int assemble_core(cda_ctx* c, const AxisHalfArgs& a, bool decode, hipStream_t s) {
  const size_t cells = cells_of(a.k);
  if (!dev_ok(c, hipMemsetAsync(a.eds, 0, cells * CDA_SHARE, s), "memset") ||
      !dev_ok(c, hipMemsetAsync(a.present, 0, cells, s), "memset"))
    return CDA_E_DEVICE;
  if (a.nhalves == 0) return CDA_OK;
  if (!dev_ok(c, hipMemsetAsync(a.axis_owner, 0xFF, 4 * (size_t)a.k * sizeof(uint32_t), s), "memset"))
    return CDA_E_DEVICE;
  if (int rc = verify_core(c, a, decode, s)) return rc;
  {
    ProfScope ps(c, "axis_half_claim", s);
    if (launch_axis_half_claim(a, s)) return CDA_E_DEVICE;
  }
  {
    ProfScope ps(c, "axis_half_place", s);
    if (launch_axis_half_place(a, s)) return CDA_E_DEVICE;
  }
  return CDA_OK;
}

}  // namespace

extern "C" {

int cda_square_axis_halves(cda_square* sq, uint32_t nq, const cda_axis_half_desc* q, uint8_t* shares,
                           uint64_t shares_cap) {
  cda_ctx* c = sq ? sq->c : nullptr;
  CDA_API_TRY
  if (!c) return CDA_E_ARG;  // null, or a square whose context was freed
  if (nq == 0) return CDA_OK;
  if (!q || !shares) return CDA_E_ARG;
  if (nq > (1u << 24)) return CDA_E_UNSUPPORTED;
  const uint32_t k = sq->k, w = 2 * k;
  for (uint32_t i = 0; i < nq; i++)
    if (q[i].axis > 1 || q[i].index >= w || q[i].side > 1) return CDA_E_ARG;
  const size_t shares_b = (size_t)nq * k * CDA_SHARE;
  if (shares_b > shares_cap) return CDA_E_ARG;
  Lock l(c);
  hipStream_t s = c->stream;
  const cda_axis_half_desc* d_q = nullptr;
  auto lay = [&](Stage& st) { d_q = st.stage(q, nq); };
  int rc;
  if ((rc = ensure(c, c->plan, staged_bytes(lay))) || (rc = ensure(c, c->payload, shares_b))) return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  {
    ProfScope ps(c, "axis_half_gather", s);
    if (launch_axis_half_gather(sq->view, d_q, nq, (uint8_t*)c->payload.p, s)) return CDA_E_DEVICE;
  }
  if (!copy_any(c, shares, c->payload.p, shares_b, s) || !dev_ok(c, hipStreamSynchronize(s), "sync"))
    return CDA_E_DEVICE;
  flush_profile(c);
  return CDA_OK;
  CDA_API_CATCH(c)
}

int cda_axis_halves_verify(cda_ctx* c, uint32_t k, uint32_t nhalves, const cda_axis_half_desc* descs,
                           const uint8_t* shares, const uint8_t* roots, uint32_t nroots, uint8_t* statuses,
                           uint8_t* axes_or_null) {
  CDA_API_TRY
  if (int rc = check_axis_shape(k, nhalves, CDA_E_NOT_POW2)) return rc;
  if (!c) return CDA_E_ARG;
  const AxisHalfArgs h = half_args(k, nhalves, descs, shares, roots, nroots, statuses, false);
  if (missing(h)) return CDA_E_ARG;
  if (nhalves == 0) return CDA_OK;
  Lock l(c);
  hipStream_t s = c->stream;
  AxisHalfArgs a = h;  // the same call on the staged copies; the kernels' workspace follows the statuses
  auto lay = [&](Stage& st) {
    a.descs = st.stage(h.descs, nhalves);
    a.roots = st.stage(h.roots, (size_t)nroots * CDA_NODE_SIZE);
    a.statuses = st.ar.take<uint8_t>(nhalves);
  };
  int rc;
  if ((rc = ensure(c, c->plan, staged_bytes(lay) + workspace_bytes(a, axis_half_workspace))) ||
      (rc = ensure(c, c->payload, shares_bytes(a))) || (rc = ensure(c, c->scratch, axes_bytes(a))))
    return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  axis_half_workspace(a, st.ar);
  a.shares = (const uint8_t*)c->payload.p;
  a.axes = (uint8_t*)c->scratch.p;
  if ((rc = staged_h2d(c, c->payload.p, shares, shares_bytes(a), s))) return rc;
  if ((rc = verify_core(c, a, any_second_side(descs, nhalves), s))) return rc;
  if ((rc = verdicts_back(c, statuses, a.statuses, nhalves, s))) return rc;
  return axes_or_null ? staged_d2h(c, axes_or_null, a.axes, axes_bytes(a), s) : CDA_OK;
  CDA_API_CATCH(c)
}

int cda_axis_halves_verify_device(cda_ctx* c, uint32_t k, uint32_t nhalves, const void* d_descs,
                                  const void* d_shares, const void* d_roots, uint32_t nroots, void* d_statuses,
                                  void* d_axes_or_null, void* stream) {
  CDA_API_TRY
  if (int rc = check_axis_shape(k, nhalves, CDA_E_NOT_POW2)) return rc;
  if (!c) return CDA_E_ARG;
  AxisHalfArgs a = half_args(k, nhalves, d_descs, d_shares, d_roots, nroots, d_statuses, false);
  if (missing(a)) return CDA_E_ARG;
  // shares and axes move 16 bytes at a time, everything else is read in 4-byte words
  if ((((uintptr_t)d_shares | (uintptr_t)d_axes_or_null) & 15) ||
      (((uintptr_t)d_descs | (uintptr_t)d_roots | (uintptr_t)d_statuses) & 3))
    return CDA_E_ARG;
  if (nhalves == 0) return CDA_OK;
  DevLock dl(c, (hipStream_t)stream);
  int rc;
  if ((rc = ensure(c, c->plan, workspace_bytes(a, axis_half_workspace))) ||
      (!d_axes_or_null && (rc = ensure(c, c->scratch, axes_bytes(a)))))
    return rc;
  Arena ws(c->plan.p);
  axis_half_workspace(a, ws);
  // the caller's axes are the axis buffers: completed in place
  a.axes = d_axes_or_null ? (uint8_t*)d_axes_or_null : (uint8_t*)c->scratch.p;
  return verify_core(c, a, true, dl.s);
  CDA_API_CATCH(c)
}

int cda_axis_halves_assemble_device(cda_ctx* c, uint32_t k, uint32_t nhalves, const void* d_descs,
                                    const void* d_shares, const void* d_roots, void* d_eds, void* d_present,
                                    void* d_statuses, void* stream) {
  CDA_API_TRY
  if (int rc = check_axis_shape(k, nhalves, CDA_E_NOT_POW2)) return rc;
  if (!c) return CDA_E_ARG;
  AxisHalfArgs a = half_args(k, nhalves, d_descs, d_shares, d_roots, 4 * k, d_statuses, true);
  if (missing(a) || !d_eds || !d_present) return CDA_E_ARG;
  if ((((uintptr_t)d_shares | (uintptr_t)d_eds) & 15) ||
      (((uintptr_t)d_descs | (uintptr_t)d_roots | (uintptr_t)d_present | (uintptr_t)d_statuses) & 3))
    return CDA_E_ARG;
  a.eds = (uint8_t*)d_eds;
  a.present = (uint8_t*)d_present;
  DevLock dl(c, (hipStream_t)stream);
  int rc;
  if ((rc = ensure(c, c->plan, workspace_bytes(a, axis_half_workspace))) ||
      (rc = ensure(c, c->scratch, axes_bytes(a))))
    return rc;
  Arena ws(c->plan.p);
  axis_half_workspace(a, ws);
  a.axes = (uint8_t*)c->scratch.p;
  return assemble_core(c, a, true, dl.s);
  CDA_API_CATCH(c)
}

int cda_square_rebuild_axes(cda_ctx* c, uint32_t k, uint32_t nhalves, const cda_axis_half_desc* descs,
                            const uint8_t* shares, const uint8_t* row_roots, const uint8_t* col_roots,
                            cda_square** out, uint8_t* statuses, uint8_t* present_or_null, uint8_t* eds_or_null,
                            uint8_t* dah, cda_err_info* err) {
  CDA_API_TRY
  set_err(err, CDA_OK, -1, -1, -1, -1);
  if (out) *out = nullptr;
  if (int rc = check_axis_shape(k, nhalves, CDA_E_NOT_POW2)) return rc;
  if (!c || !out || !row_roots || !col_roots || !dah) return CDA_E_ARG;
  const AxisHalfArgs h = half_args(k, nhalves, descs, shares, nullptr, 4 * k, statuses, true);
  if (nhalves && (!descs || !shares || !statuses)) return CDA_E_ARG;
  const size_t cells = cells_of(k);
  RebuildHost host(k, row_roots, col_roots, present_or_null);
  Lock l(c);
  hipStream_t s = c->stream;
  int rc;
  // the handle's memory first: the halves are assembled straight into its EDS area
  SquareBuild b;
  if ((rc = square_alloc(c, k, b, s))) return rc;
  // staging in the context's workspace: descriptors | roots | statuses | presence map, then the kernels' workspace;
  // the shares; the axis buffers
  AxisHalfArgs a = h;  // the same call on the staged copies
  a.eds = b.eds;
  auto lay = [&](Stage& st) {
    a.descs = st.stage(h.descs, nhalves);
    a.roots = st.stage(host.roots.data(), host.roots.size());
    a.statuses = st.ar.take<uint8_t>(nhalves);
    a.present = st.ar.take<uint8_t>(cells);
  };
  if ((rc = ensure(c, c->plan, staged_bytes(lay) + workspace_bytes(a, axis_half_workspace))) ||
      (rc = ensure(c, c->payload, shares_bytes(a))) || (rc = ensure(c, c->scratch, axes_bytes(a))))
    return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  axis_half_workspace(a, st.ar);
  a.shares = (const uint8_t*)c->payload.p;
  a.axes = (uint8_t*)c->scratch.p;
  if (nhalves && (rc = staged_h2d(c, c->payload.p, shares, shares_bytes(a), s))) return rc;
  if ((rc = assemble_core(c, a, nhalves && any_second_side(descs, nhalves), s))) return rc;
  return rebuild_finish(c, k, b, a.present, a.statuses, nhalves, statuses, host, eds_or_null, out, dah, err,
                        "cda_square_rebuild_axes", s);
  CDA_API_CATCH(c)
}

}  // extern "C"
