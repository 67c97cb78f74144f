// mixed.cpp — blocks of different sizes in one call: cda_extend_commit_mixed (host buffers) and
// cda_extend_commit_mixed_device (include/cda.h).  The routing is mixed_route.h's: blocks with k at most the context's
// small limit (CDA_OPT_MIXED_SMALL_MAX) go together, whatever their sizes, into one launch of small_square_kernel; the
// others run through the block pipeline (engine.cpp enqueue_pipeline) -- the host form groups them by k and gathers
// each group into the workspace, the device form takes each run of consecutive blocks of equal k where it lies.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ctx.h"
#include "mixed_route.h"
#include "small_square.h"

using namespace cda;

namespace {

int check_ks(const uint32_t* ks, uint32_t nblocks, cda_err_info* err) {
  uint32_t bad = 0;
  const int r = mixed_check_ks(ks, nblocks, kMaxDeviceK, &bad);
  if (!r) return CDA_OK;
  const int code = r == 1 ? CDA_E_NOT_POW2 : CDA_E_UNSUPPORTED;
  set_err(err, code, -1, -1, -1, (int)bad);
  return code;
}

// leaf and level records of the largest pipeline call ahead, so that no call in between regrows the workspace
int ensure_records(cda_ctx* c, uint64_t cells) {
  if (cells == 0) return CDA_OK;
  if (int rc = ensure(c, c->leaf, cells * CDA_REC_BYTES)) return rc;
  return ensure(c, c->scratch, 2 * cells * CDA_REC_BYTES);
}

// The fused launch over `blocks` (indices into ks) of buffers packed as `off`: the descriptor table goes through the
// context's staging slot (c->plan), which the lock the caller holds orders against every other user on any stream.
int enqueue_small(cda_ctx* c, const uint32_t* ks, const std::vector<uint32_t>& blocks, const MixedOffsets& off,
                  const uint8_t* d_ods, uint8_t* d_eds, void* d_roots, void* d_dah, unsigned long long* d_status,
                  hipStream_t s) {
  if (blocks.empty()) return CDA_OK;
  uint32_t kmax = 0;
  const std::vector<SmallSquareDesc> descs = small_square_descs(ks, blocks, off, &kmax);
  const SmallSquareDesc* d_descs = nullptr;
  auto lay = [&](Stage& st) { d_descs = st.stage(descs.data(), descs.size()); };
  if (int rc = ensure(c, c->plan, staged_bytes(lay))) return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  ProfScope ps(c, "small_square", s);
  const int lr = launch_small_squares(d_descs, (uint32_t)descs.size(), kmax, d_ods, d_eds, d_roots, d_dah, d_status, s);
  if (lr) return lr == -2 ? CDA_E_UNSUPPORTED : CDA_E_DEVICE;
  return CDA_OK;
}

}  // namespace

extern "C" {

int cda_extend_commit_mixed(cda_ctx* c, uint32_t nblocks, const uint32_t* ks, const uint8_t* ods, uint8_t* eds_or_null,
                            uint8_t* row_roots, uint8_t* col_roots, uint8_t* dah, cda_err_info* err) {
  CDA_API_TRY
  set_err(err, CDA_OK, -1, -1, -1, -1);
  if (!c || !ks || !ods || !row_roots || !col_roots || !dah || nblocks == 0) return CDA_E_ARG;
  if (int rc = check_ks(ks, nblocks, err)) return rc;
  Lock l(c);
  const uint32_t small_max = (uint32_t)c->mixed_small_max;
  const MixedOffsets in = mixed_offsets(ks, nblocks);
  // workspace order: the small blocks in input order, then each group; pos[b] = block b's place in it
  const std::vector<uint32_t> small = mixed_small_blocks(ks, nblocks, small_max);
  const std::vector<MixedGroup> groups = mixed_groups(ks, nblocks, small_max);
  std::vector<uint32_t> order(small), wks(nblocks), pos(nblocks);
  for (const MixedGroup& g : groups) order.insert(order.end(), g.blocks.begin(), g.blocks.end());
  for (uint32_t p = 0; p < nblocks; p++) {
    wks[p] = ks[order[p]];
    pos[order[p]] = p;
  }
  const MixedOffsets ws = mixed_offsets(wks.data(), nblocks);
  const size_t roots_b = (size_t)ws.roots[nblocks] * 2 * CDA_REC_BYTES;
  uint64_t max_cells = 0;
  for (const MixedGroup& g : groups) max_cells = std::max<uint64_t>(max_cells, (uint64_t)g.blocks.size() * 4 * g.k * g.k);
  int rc;
  if ((rc = ensure(c, c->ods, ws.ods[nblocks])) || (rc = ensure(c, c->eds, ws.eds[nblocks])) ||
      (rc = ensure(c, c->roots, roots_b)) || (rc = ensure(c, c->dah, (size_t)nblocks * 32)) ||
      (rc = ensure(c, c->status, (size_t)nblocks * 8)) || (rc = ensure_records(c, max_cells)))
    return rc;
  hipStream_t s = c->stream;
  uint8_t* d_ods = (uint8_t*)c->ods.p;
  uint8_t* d_eds = (uint8_t*)c->eds.p;
  // one copy per stretch of blocks that are neighbours both in the caller's buffer and in the workspace
  auto stretches = [&](auto&& copy) {
    for (uint32_t b = 0; b < nblocks;) {
      uint32_t e = b + 1;
      while (e < nblocks && pos[e] == pos[e - 1] + 1) e++;
      if (!copy(b, e)) return false;
      b = e;
    }
    return true;
  };
  if (!stretches([&](uint32_t b, uint32_t e) {
        return dev_ok(c, hipMemcpyAsync(d_ods + ws.ods[pos[b]], ods + in.ods[b], in.ods[e] - in.ods[b],
                                        hipMemcpyHostToDevice, s), "H2D");
      }))
    return CDA_E_DEVICE;
  if (!dev_ok(c, hipMemsetAsync(c->status.p, 0xFF, (size_t)nblocks * 8, s), "hipMemsetAsync")) return CDA_E_DEVICE;
  // the small blocks lead the workspace, so their descriptors are those of the first small.size() workspace blocks
  {
    std::vector<uint32_t> lead(small.size());
    for (uint32_t p = 0; p < lead.size(); p++) lead[p] = p;
    if ((rc = enqueue_small(c, wks.data(), lead, ws, d_ods, d_eds, c->roots.p, c->dah.p,
                            (unsigned long long*)c->status.p, s)))
      return rc;
  }
  uint32_t p0 = (uint32_t)small.size();
  for (const MixedGroup& g : groups) {
    const uint32_t cnt = (uint32_t)g.blocks.size();
    if ((rc = enqueue_pipeline(c, g.k, cnt, d_ods + ws.ods[p0], d_eds + ws.eds[p0],
                               (uint8_t*)c->roots.p + ws.roots[p0] * 2 * CDA_REC_BYTES, (uint8_t*)c->dah.p + (size_t)p0 * 32,
                               (unsigned long long*)c->status.p + p0, s)))
      return rc;
    p0 += cnt;
  }
  if (eds_or_null && !stretches([&](uint32_t b, uint32_t e) {
        return dev_ok(c, hipMemcpyAsync(eds_or_null + in.eds[b], d_eds + ws.eds[pos[b]], in.eds[e] - in.eds[b],
                                        hipMemcpyDeviceToHost, s), "D2H");
      }))
    return CDA_E_DEVICE;
  std::vector<uint8_t> recs(roots_b), wdah((size_t)nblocks * 32);
  std::vector<uint64_t> st(nblocks);
  if (!dev_ok(c, hipMemcpyAsync(recs.data(), c->roots.p, roots_b, hipMemcpyDeviceToHost, s), "D2H") ||
      !dev_ok(c, hipMemcpyAsync(wdah.data(), c->dah.p, wdah.size(), hipMemcpyDeviceToHost, s), "D2H") ||
      !dev_ok(c, hipMemcpyAsync(st.data(), c->status.p, (size_t)nblocks * 8, hipMemcpyDeviceToHost, s), "D2H") ||
      !dev_ok(c, hipStreamSynchronize(s), "sync"))
    return CDA_E_DEVICE;
  flush_profile(c);
  for (uint32_t b = 0; b < nblocks; b++) {
    const uint32_t p = pos[b], w = 2 * ks[b];
    const uint8_t* r = recs.data() + (size_t)ws.roots[p] * 2 * CDA_REC_BYTES;
    pack_roots(r, w, row_roots + (size_t)in.roots[b] * CDA_NODE_SIZE);
    pack_roots(r + (size_t)w * CDA_REC_BYTES, w, col_roots + (size_t)in.roots[b] * CDA_NODE_SIZE);
    memcpy(dah + (size_t)b * 32, wdah.data() + (size_t)p * 32, 32);
  }
  for (uint32_t b = 0; b < nblocks; b++)
    if ((rc = map_status(st[pos[b]], (int)b, err))) return rc;
  return CDA_OK;
  CDA_API_CATCH(c)
}

int cda_extend_commit_mixed_device(cda_ctx* c, uint32_t nblocks, const uint32_t* ks, const void* d_ods, void* d_eds,
                                   void* d_roots, void* d_dah, void* d_status, void* stream) {
  CDA_API_TRY
  if (!c || !ks || !d_ods || !d_eds || !d_roots || !d_dah || !d_status || nblocks == 0) return CDA_E_ARG;
  if (int rc = check_ks(ks, nblocks, nullptr)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : nullptr;
  DevLock l(c, s);
  const uint32_t small_max = (uint32_t)c->mixed_small_max;
  const MixedOffsets off = mixed_offsets(ks, nblocks);
  const std::vector<MixedRun> runs = mixed_runs(ks, nblocks, small_max);
  uint64_t max_cells = 0;
  for (const MixedRun& r : runs) max_cells = std::max<uint64_t>(max_cells, (uint64_t)r.count * 4 * r.k * r.k);
  int rc;
  if ((rc = ensure_records(c, max_cells))) return rc;
  if (!dev_ok(c, hipMemsetAsync(d_status, 0xFF, (size_t)nblocks * 8, s), "hipMemsetAsync")) return CDA_E_DEVICE;
  if ((rc = enqueue_small(c, ks, mixed_small_blocks(ks, nblocks, small_max), off, (const uint8_t*)d_ods,
                          (uint8_t*)d_eds, d_roots, d_dah, (unsigned long long*)d_status, s)))
    return rc;
  for (const MixedRun& r : runs)
    if ((rc = enqueue_pipeline(c, r.k, r.count, (const uint8_t*)d_ods + off.ods[r.first],
                               (uint8_t*)d_eds + off.eds[r.first],
                               (uint8_t*)d_roots + off.roots[r.first] * 2 * CDA_REC_BYTES,
                               (uint8_t*)d_dah + (size_t)r.first * 32, (unsigned long long*)d_status + r.first, s)))
      return rc;
  return CDA_OK;
  CDA_API_CATCH(c)
}

}  // extern "C"
