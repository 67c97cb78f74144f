// blob.cpp — C ABI of reading a retained square back (include/cda.h):
//   cda_square_index   every sequence of the square under share_index_rule.h (blob_kernels.hip's scan), and the share
//                      commitment of every clean blob out of the retained tree nodes
//   cda_square_read    the payload bytes of sequences, share headers stripped (blob_kernels.hip's gather)
// The commitments are cda_square_commitment_proofs' in its commitments-only form, called with the ranges the scan
// found: the records come to the host in the scan's wait, the clean blobs' ranges go back in that call (a second wait).
// Its gather and commitment_roots_kernel stay the only copies.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "blob.h"
#include "ctx.h"
#include "share_index_rule.h"

using namespace cda;

namespace {

bool device_memory(const void* p) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory is not an error here
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

}  // namespace

extern "C" {

int cda_square_index(cda_square* sq, uint32_t subtree_root_threshold, uint32_t cap, cda_sequence* seqs,
                     uint8_t* commitments, cda_square_summary* summary) {
  cda_ctx* c = sq ? sq->c : nullptr;
  CDA_API_TRY
  if (!c) return CDA_E_ARG;  // null, or a square whose context was freed
  if (!summary || (cap && !seqs) || (commitments && subtree_root_threshold == 0)) return CDA_E_ARG;
  const uint32_t k = sq->k, n = k * k;
  if (k > kMaxBlobK) return CDA_E_UNSUPPORTED;
  Lock l(c);
  hipStream_t s = c->stream;
  const uint32_t nblk = (n + 1023) / 1024, first = cap < n ? cap : n;  // no square has more than n sequences
  const uint32_t init[4] = {0, 0, 0, kNoShare};
  uint32_t* d_counters = nullptr;
  uint32_t* d_blk_mark = nullptr;
  uint32_t* d_blk_count = nullptr;
  auto lay = [&](Stage& st) {
    d_counters = st.stage(init, 4);
    d_blk_mark = st.ar.take<uint32_t>(nblk);
    d_blk_count = st.ar.take<uint32_t>(nblk);
  };
  const size_t recs_b = (size_t)n * sizeof(cda_sequence);
  int rc;
  if ((rc = ensure(c, c->plan, staged_bytes(lay))) || (rc = ensure(c, c->scratch, recs_b))) return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  cda_sequence* d_recs = (cda_sequence*)c->scratch.p;
  {
    ProfScope ps(c, "square_index", s);
    if (!dev_ok(c, hipMemsetAsync(d_recs, 0, recs_b, s), "memset")) return CDA_E_DEVICE;
    if (launch_share_index(sq->view, k, subtree_root_threshold, d_blk_mark, d_blk_count, d_recs, d_counters, s))
      return CDA_E_DEVICE;
  }
  // the scan's wait: the counters, and with them the records the caller has room for (the commitments' ranges)
  uint32_t got[4] = {};
  std::vector<cda_sequence> recs(commitments ? first : 0);
  if (!dev_ok(c, hipMemcpyAsync(got, d_counters, sizeof got, hipMemcpyDeviceToHost, s), "D2H") ||
      (!recs.empty() &&
       !dev_ok(c, hipMemcpyAsync(recs.data(), d_recs, recs.size() * sizeof(cda_sequence), hipMemcpyDeviceToHost, s),
               "D2H")) ||
      !dev_ok(c, hipStreamSynchronize(s), "sync"))
    return CDA_E_DEVICE;
  const uint32_t nw = got[0] < cap ? got[0] : cap;
  // The commitments first: the caller's arrays and the summary are written only once nothing can fail but a copy.
  // That call leaves c->scratch, where the records lie, alone.
  std::vector<uint8_t> com;
  if (commitments && nw) {
    std::vector<cda_blob_range> ranges;
    std::vector<uint32_t> at;
    for (uint32_t i = 0; i < nw; i++)
      if (recs[i].kind == CDA_SEQ_KIND_BLOB && recs[i].status == 0) {
        ranges.push_back(cda_blob_range{recs[i].start, recs[i].nshares});
        at.push_back(i);
      }
    com.assign((size_t)nw * 32, 0);
    if (!ranges.empty()) {
      std::vector<uint8_t> packed(ranges.size() * 32);
      if ((rc = cda_square_commitment_proofs(sq, (uint32_t)ranges.size(), ranges.data(), subtree_root_threshold, 0, 0, 0,
                                             nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                             packed.data(), nullptr)))
        return rc;
      for (size_t i = 0; i < at.size(); i++) memcpy(&com[(size_t)at[i] * 32], &packed[i * 32], 32);
    }
  }
  if (!copy_any(c, seqs, d_recs, (size_t)nw * sizeof(cda_sequence), s) ||
      !copy_any(c, commitments, com.data(), com.size(), s))
    return CDA_E_DEVICE;
  if (!dev_ok(c, hipStreamSynchronize(s), "sync")) return CDA_E_DEVICE;  // com and the caller's arrays are done with
  summary->k = k;
  summary->nseq = got[0];
  summary->npadding = got[1];
  summary->norphans = got[2];
  summary->first_orphan = got[3];
  flush_profile(c);
  return CDA_OK;
  CDA_API_CATCH(c)
}

int cda_square_read(cda_square* sq, uint32_t nq, const cda_sequence_range* q, const uint64_t* data_off,
                    uint64_t data_cap, uint8_t* data) {
  cda_ctx* c = sq ? sq->c : nullptr;
  CDA_API_TRY
  if (!c) return CDA_E_ARG;  // null, or a square whose context was freed
  if (nq == 0) return CDA_OK;
  if (!q || !data_off) return CDA_E_ARG;
  if (nq > (1u << 24)) return CDA_E_UNSUPPORTED;
  const uint32_t k = sq->k;
  const uint64_t n = (uint64_t)k * k;
  std::vector<uint32_t> unit_off((size_t)nq + 1);
  uint64_t units = 0, bytes = 0;
  for (uint32_t i = 0; i < nq; i++) {
    const uint32_t need = seq_shares_needed(q[i].compact != 0, q[i].seq_len);
    if ((uint64_t)q[i].start + q[i].nshares > n || need > q[i].nshares || data_off[i] > data_cap ||
        q[i].seq_len > data_cap - data_off[i])
      return CDA_E_ARG;
    unit_off[i] = (uint32_t)units;
    units += need;
    bytes += q[i].seq_len;
    if (units > kMaxReadUnits) return CDA_E_UNSUPPORTED;
  }
  unit_off[nq] = (uint32_t)units;
  if (units == 0) return CDA_OK;
  if (!data) return CDA_E_ARG;
  Lock l(c);
  hipStream_t s = c->stream;
  // to device memory the bytes go where the caller wants them; to host memory they are packed in the context's
  // workspace, query after query, and copied out run by run (queries that follow each other in `data` as one run), so
  // that nothing between the ranges is written
  const bool direct = device_memory(data);
  std::vector<unsigned long long> dst(nq);
  uint64_t cursor = 0;
  for (uint32_t i = 0; i < nq; i++) {
    dst[i] = direct ? data_off[i] : cursor;
    cursor += q[i].seq_len;
  }
  const cda_sequence_range* d_q = nullptr;
  const uint32_t* d_unit_off = nullptr;
  const unsigned long long* d_dst = nullptr;
  auto lay = [&](Stage& st) {
    d_q = st.stage(q, nq);
    d_unit_off = st.stage(unit_off.data(), unit_off.size());
    d_dst = st.stage(dst.data(), dst.size());
  };
  int rc;
  if ((rc = ensure(c, c->plan, staged_bytes(lay))) || (!direct && (rc = ensure(c, c->payload, bytes)))) return rc;
  Stage st{c, s, Arena(c->plan.p)};
  lay(st);
  if (!st.ok) return CDA_E_DEVICE;
  uint8_t* d_out = direct ? data : (uint8_t*)c->payload.p;
  {
    ProfScope ps(c, "square_read", s);
    if (launch_sequence_read(sq->view, k, d_q, nq, d_unit_off, d_dst, (uint32_t)units, d_out, s)) return CDA_E_DEVICE;
  }
  if (!direct) {
    for (uint32_t i = 0; i < nq;) {
      uint32_t j = i;
      uint64_t len = q[i].seq_len;
      while (j + 1 < nq && data_off[j + 1] == data_off[j] + q[j].seq_len) len += q[++j].seq_len;
      if (len && (rc = staged_d2h(c, data + data_off[i], d_out + dst[i], len, s))) return rc;
      i = j + 1;
    }
  }
  if (!dev_ok(c, hipStreamSynchronize(s), "sync")) return CDA_E_DEVICE;
  flush_profile(c);
  return CDA_OK;
  CDA_API_CATCH(c)
}

}  // extern "C"
