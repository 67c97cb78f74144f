// befp.cpp — C ABI of the bad-encoding fraud proofs (include/cda.h): batched Validate of proofs that an
// axis of a committed square is not a Reed-Solomon codeword (specs fraud_proofs.md; rsmt2d ErrByzantineData is what
// cda_repair reports as CDA_E_BYZANTINE).  The host checks arguments and copies; every check of a proof is the
// kernels': befp_kernels.hip around the verify, decode, encode and axis-root launches the library already has, on one
// stream with no host wait between them.
#include <hip/hip_runtime.h>

#include "ctx.h"
#include "sampling.h"

using namespace cda;

namespace {

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// k of a call: a power of two the axis-root kernel takes whole (2k leaves in one workgroup's LDS)
int check_k(uint32_t k, uint32_t nproofs) {
  if (!is_pow2(k)) return CDA_E_ARG;
  if (2 * (uint64_t)k > (uint64_t)kAxisRootsMaxLeaves) return CDA_E_UNSUPPORTED;
  if ((uint64_t)nproofs * 2 * k > 0x7FFFFFFFull) return CDA_E_UNSUPPORTED;  // slots are 32-bit, launches take int
  return CDA_OK;
}

int code_of(int lr) { return lr == -2 ? CDA_E_UNSUPPORTED : CDA_E_DEVICE; }

// The seven launches.  a: arguments and workspace bound, a.axes sized [nproofs][2k][512].
int enqueue_befp(cda_ctx* c, const BefpArgs& a, hipStream_t s) {
  const uint32_t k = a.k, w = 2 * k, slots = a.nproofs * w;
  int lr;
  {
    ProfScope ps(c, "befp_prep", s);
    if (launch_befp_prep(a, s)) return CDA_E_DEVICE;
  }
  {
    VerifyArgs n{};
    n.descs = a.nmt_descs;
    n.namespaces = a.nmt_ns;
    n.roots = a.roots;
    n.nodes = a.nodes;
    n.leaves = a.shares;
    n.ok = a.nmt_ok;
    n.nproofs = slots;
    n.nroots = a.nroots;
    n.nnodes_total = a.nnodes_total;
    n.nleaves_total = a.nentries;
    ProfScope ps(c, "befp_nmt_verify", s);
    if (launch_nmt_verify(n, false, s)) return CDA_E_DEVICE;
  }
  {
    ProfScope ps(c, "befp_gather", s);
    if (launch_befp_gather(a, s)) return CDA_E_DEVICE;
  }
  {
    ProfScope ps(c, "befp_rs_decode", s);
    if ((lr = launch_rs_decode(a.axes, a.cw_off, a.cw_stride, a.mask, (int)a.nproofs, (int)k, CDA_SHARE, s)))
      return code_of(lr);
  }
  {  // slots [k, 2k) of every buffer := Encode(slots [0, k))
    RsJob j{};
    j.src = a.axes;
    j.src_cw = (long long)w * CDA_SHARE;
    j.src_sh = CDA_SHARE;
    j.dst = a.axes + (size_t)k * CDA_SHARE;
    j.dst_cw = (long long)w * CDA_SHARE;
    j.dst_sh = CDA_SHARE;
    j.k = (int)k;
    j.cw_per_blk = (int)a.nproofs;
    j.nblk = 1;
    j.shard_len = CDA_SHARE;
    const bool ff8 = w <= 256;
    ProfScope ps(c, ff8 ? "befp_rs_encode8" : "befp_rs_encode16", s);
    if ((lr = ff8 ? launch_rs_encode8(j, s) : launch_rs_encode16(j, s))) return code_of(lr);
  }
  {
    ProfScope ps(c, "befp_axis_roots", s);
    if ((lr = launch_axis_roots(a.axes, (long long)w * CDA_SHARE, (int)w, k, a.axis_idx, (int)a.nproofs, a.recs,
                                a.status, s)))
      return code_of(lr);
  }
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
  if (int rc = check_k(k, nproofs)) return rc;
  if (nproofs == 0) return CDA_OK;
  if (!descs || !verdicts || (nentries && (!entries || !shares)) || (nnodes_total && !nodes) || (nroots && !roots))
    return CDA_E_ARG;
  Lock l(c);
  hipStream_t s = c->stream;
  // descriptors | entries | roots | verdicts | the kernels' workspace, the nodes, the shares, the axis buffers
  const size_t desc_b = align256((size_t)nproofs * sizeof(cda_befp_desc));
  const size_t ent_b = align256((size_t)nentries * sizeof(cda_befp_entry));
  const size_t roots_b = align256((size_t)nroots * CDA_NODE_SIZE), ver_b = align256((size_t)nproofs * 4);
  const size_t nodes_b = (size_t)nnodes_total * CDA_NODE_SIZE, shares_b = (size_t)nentries * CDA_SHARE;
  int rc;
  if ((rc = ensure(c, c->plan, desc_b + ent_b + roots_b + ver_b + befp_workspace_bytes(k, nproofs))) ||
      (rc = ensure(c, c->nodes, nodes_b)) || (rc = ensure(c, c->payload, shares_b)) ||
      (rc = ensure(c, c->scratch, (size_t)nproofs * 2 * k * CDA_SHARE)))
    return rc;
  uint8_t* p = (uint8_t*)c->plan.p;
  auto up = [&](const void* src, size_t n, size_t slot) -> uint8_t* {  // null: the copy failed
    uint8_t* at = p;
    p += slot;
    if (n && !dev_ok(c, hipMemcpyAsync(at, src, n, hipMemcpyHostToDevice, s), "H2D")) return nullptr;
    return at;
  };
  BefpArgs a{};
  a.k = k;
  a.nproofs = nproofs;
  a.nentries = nentries;
  a.nnodes_total = nnodes_total;
  a.nroots = nroots;
  if (!(a.descs = (const cda_befp_desc*)up(descs, (size_t)nproofs * sizeof(cda_befp_desc), desc_b)) ||
      !(a.entries = (const cda_befp_entry*)up(entries, (size_t)nentries * sizeof(cda_befp_entry), ent_b)) ||
      !(a.roots = up(roots, (size_t)nroots * CDA_NODE_SIZE, roots_b)))
    return CDA_E_DEVICE;
  a.verdicts = (int32_t*)p;
  befp_workspace_bind(a, p + ver_b);
  a.nodes = (const uint8_t*)c->nodes.p;
  a.shares = (const uint8_t*)c->payload.p;
  a.axes = (uint8_t*)c->scratch.p;
  if (nodes_b && (rc = staged_h2d(c, c->nodes.p, nodes, nodes_b, s))) return rc;
  if (shares_b && (rc = staged_h2d(c, c->payload.p, shares, shares_b, s))) return rc;
  if ((rc = enqueue_befp(c, a, s))) return rc;
  if (!dev_ok(c, hipMemcpyAsync(verdicts, a.verdicts, (size_t)nproofs * 4, hipMemcpyDeviceToHost, s), "D2H") ||
      !dev_ok(c, hipStreamSynchronize(s), "sync"))
    return CDA_E_DEVICE;
  flush_profile(c);
  return CDA_OK;
  CDA_API_CATCH(c)
}

int cda_befp_validate_device(cda_ctx* c, uint32_t k, uint32_t nproofs, const void* d_descs, const void* d_entries,
                             uint32_t nentries, const void* d_shares, const void* d_nodes, uint32_t nnodes_total,
                             const void* d_roots, uint32_t nroots, void* d_verdicts, void* stream) {
  CDA_API_TRY
  if (!c) return CDA_E_ARG;
  if (int rc = check_k(k, nproofs)) return rc;
  if (nproofs == 0) return CDA_OK;
  if (!d_descs || !d_verdicts || (nentries && (!d_entries || !d_shares)) || (nnodes_total && !d_nodes) ||
      (nroots && !d_roots))
    return CDA_E_ARG;
  // shares are read 16 bytes at a time, everything else in 4-byte words
  if (((uintptr_t)d_shares & 15) || (((uintptr_t)d_descs | (uintptr_t)d_entries | (uintptr_t)d_nodes |
                                      (uintptr_t)d_roots | (uintptr_t)d_verdicts) & 3))
    return CDA_E_ARG;
  BefpArgs a{};
  a.descs = (const cda_befp_desc*)d_descs;
  a.entries = (const cda_befp_entry*)d_entries;
  a.shares = (const uint8_t*)d_shares;
  a.nodes = (const uint8_t*)d_nodes;
  a.roots = (const uint8_t*)d_roots;
  a.verdicts = (int32_t*)d_verdicts;
  a.k = k;
  a.nproofs = nproofs;
  a.nentries = nentries;
  a.nnodes_total = nnodes_total;
  a.nroots = nroots;
  DevLock dl(c, (hipStream_t)stream);
  int rc;
  if ((rc = ensure(c, c->plan, befp_workspace_bytes(k, nproofs))) ||
      (rc = ensure(c, c->scratch, (size_t)nproofs * 2 * k * CDA_SHARE)))
    return rc;
  befp_workspace_bind(a, c->plan.p);
  a.axes = (uint8_t*)c->scratch.p;
  return enqueue_befp(c, a, dl.s);
  CDA_API_CATCH(c)
}

}  // extern "C"
