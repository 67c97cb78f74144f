// share_index_rule.h — the rule that reads the sequences of a square back from its shares: which ODS
// shares start a sequence, how many shares it claims, which shares belong to it and what is wrong with it.  Shared by
// the scan kernels (blob_kernels.hip), the host call (blob.cpp) and the stand-alone program of tests/san, which builds
// it with a plain C++ compiler; cda/blob.py index_host is its Python mirror.
//
// Parity unpinned: go-square's shares package (ParseBlobs, ParseTxs) is not in the reference tree (go.mod:9).  The
// rule restates specs/src/specs/shares.md:27-107 and the namespace ranges of specs/src/specs/namespace.md.
//
// Of share g (row-major in the k x k ODS) only bytes [0, 34) are read: ns = [0, 29), version = b[29] >> 1,
// start = b[29] & 1, seq_len = the big-endian u32 at [30, 34) (meaningful when start is set).
//   compact namespace  TRANSACTION (0..01) or PAY_FOR_BLOB (0..04)
//   padding share      start && seq_len == 0 outside the compact namespaces (namespace, reserved and tail padding)
//   sequence           a start share s that is not padding; kind TX / PFB / BLOB (every other namespace); it claims
//                      n(s) shares [s, s + n): SparseSharesNeeded(seq_len) for a blob, CompactSharesNeeded(seq_len)
//                      for the compact kinds, where a compact start share with seq_len == 0 is one share of no bytes
//   last(g)            the largest start-share index <= g, padding shares included
// The ordered scan carries mark(g) = 0 for a continuation share and ((g << 1 | sequence) + 1) for a start share;
// prev(g) = max of mark over [0, g).  For a continuation share prev(g) names last(g); for a start share it names
// last(g - 1).  share_role says from (g, its header, prev(g), the header prev names) alone what share g does to the
// sequence before it, so the result does not depend on the order in which shares are looked at:
//   a start share inside the claim of the sequence prev names           -> that sequence is BROKEN
//   a continuation share inside that claim, other namespace or version  -> that sequence is BROKEN
//   a continuation share with no start before it, after a padding share, or past the claim  -> an orphan
// The other status bits are the start share's own (own_status).  Nothing outside the square is ever read: a claim
// past k * k is TRUNCATED, not followed.
#pragma once
#include <stdint.h>

#include "../../include/cda.h"
#include "commitment_rule.h"

namespace cda {

constexpr uint32_t kSparseFirst = 478, kSparseNext = 482;    // payload bytes of a blob's first / later shares
constexpr uint32_t kCompactFirst = 474, kCompactNext = 478;  // the same of a compact sequence
constexpr uint32_t kNoShare = 0xFFFFFFFFu;

// The shares that seq_len payload bytes take (0 for none).  In 64 bits: seq_len is a hostile 32-bit field, and
// seq_len - first + next - 1 wraps in 32 bits from 0xFFFFFFFD on; the count itself is at most 8,910,721.
CDA_HD uint32_t seq_shares_needed(bool compact, uint32_t seq_len) {
  const uint64_t first = compact ? kCompactFirst : kSparseFirst, next = compact ? kCompactNext : kSparseNext;
  return seq_len == 0 ? 0u : seq_len <= first ? 1u : (uint32_t)(1 + ((uint64_t)seq_len - first + next - 1) / next);
}

// Bytes [0, 34) of a share as little-endian words: w[i] = bytes [4i, 4i + 4), w[8] = bytes 32 and 33.
struct ShareHead {
  uint32_t w[9];

  CDA_HD void from_bytes(const uint8_t* b) {
    for (int i = 0; i < 8; i++)
      w[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 |
             (uint32_t)b[4 * i + 3] << 24;
    w[8] = (uint32_t)b[32] | (uint32_t)b[33] << 8;
  }
  CDA_HD bool start() const { return (w[7] >> 8) & 1; }
  CDA_HD uint32_t version() const { return (w[7] >> 9) & 0x7F; }
  CDA_HD uint32_t seq_len() const {
    return ((w[7] >> 16) & 0xFF) << 24 | (w[7] >> 24) << 16 | (w[8] & 0xFF) << 8 | ((w[8] >> 8) & 0xFF);
  }
  CDA_HD uint32_t ns_byte(int i) const { return (w[i >> 2] >> (8 * (i & 3))) & 0xFF; }
  // bytes [0, 28) are zero: namespace version 0 and an id of at most 255
  CDA_HD bool low_ns() const { return !(w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6]); }
  CDA_HD bool compact() const { return low_ns() && ((w[7] & 0xFF) == 1 || (w[7] & 0xFF) == 4); }
  CDA_HD bool padding() const { return start() && !compact() && seq_len() == 0; }
  CDA_HD bool sequence() const { return start() && !padding(); }
  CDA_HD uint32_t kind() const {
    return !compact() ? CDA_SEQ_KIND_BLOB : (w[7] & 0xFF) == 1 ? CDA_SEQ_KIND_TX : CDA_SEQ_KIND_PFB;
  }
  // n(s) of a sequence's start share: what its seq_len needs, and one share for an empty compact sequence
  CDA_HD uint32_t nshares() const {
    const uint32_t n = seq_shares_needed(compact(), seq_len());
    return n ? n : 1u;
  }
  // the same namespace and share version (the start bit aside)
  CDA_HD bool same_sequence(const ShareHead& o) const {
    bool same = ((w[7] ^ o.w[7]) & 0xFEFF) == 0;
    for (int i = 0; i < 7; i++) same = same && w[i] == o.w[i];
    return same;
  }
  CDA_HD uint32_t mark(uint32_t g) const { return start() ? ((g << 1) | (sequence() ? 1u : 0u)) + 1 : 0; }
  // The status bits a sequence's start share s decides alone.  threshold == 0: no commitment is asked for and
  // CDA_SEQ_UNALIGNED is not looked at.
  CDA_HD uint32_t own_status(uint32_t s, uint32_t k, uint32_t threshold) const {
    const uint32_t n = nshares();
    uint32_t st = 0;
    if ((uint64_t)s + n > (uint64_t)k * k) st |= CDA_SEQ_TRUNCATED;
    if (version()) st |= CDA_SEQ_VERSION;
    if (kind() == CDA_SEQ_KIND_BLOB) {
      if (low_ns() || ns_byte(0) == 0xFF) st |= CDA_SEQ_RESERVED_NS;
      if (threshold) {
        const uint32_t W = sub_tree_width(n, threshold);
        if (W > k || s % W) st |= CDA_SEQ_UNALIGNED;
      }
    }
    return st;
  }
  CDA_HD void record(uint32_t s, uint32_t k, uint32_t threshold, cda_sequence& r) const {
    r.start = s;
    r.nshares = nshares();
    r.seq_len = seq_len();
    r.kind = (uint8_t)kind();
    r.share_version = (uint8_t)version();
    r.status = (uint8_t)own_status(s, k, threshold);
    r.pad_ = 0;
    for (int i = 0; i < 29; i++) r.ns[i] = (uint8_t)ns_byte(i);
    r.pad2_[0] = r.pad2_[1] = r.pad2_[2] = 0;
  }
};

// the scan's values
CDA_HD bool mark_is_sequence(uint32_t m) { return m && ((m - 1) & 1); }
CDA_HD uint32_t mark_share(uint32_t m) { return (m - 1) >> 1; }

enum ShareRole : uint32_t { kRoleNone = 0, kRoleOrphan = 1, kRoleBreaks = 2 };
// What share g (header h) does, given prev = the scan's value over [0, g) and, when prev names a sequence, that
// sequence's start share `owner` (not read otherwise).
CDA_HD ShareRole share_role(uint32_t g, const ShareHead& h, uint32_t prev, const ShareHead& owner) {
  if (!mark_is_sequence(prev)) return h.start() ? kRoleNone : kRoleOrphan;
  const bool inside = (uint64_t)g < (uint64_t)mark_share(prev) + owner.nshares();
  if (h.start()) return inside ? kRoleBreaks : kRoleNone;
  if (!inside) return kRoleOrphan;
  return h.same_sequence(owner) ? kRoleNone : kRoleBreaks;
}

// The host form: the sequences of the k x k ODS whose share g = r * k + c lies at q0 + r * row_pitch + c * 512, in
// ascending order.  Writes min(nseq, cap) records (status bits of every kind included) and the summary.
inline void share_index_host(const uint8_t* q0, size_t row_pitch, uint32_t k, uint32_t threshold, uint32_t cap,
                             cda_sequence* out, cda_square_summary* sum) {
  uint32_t prev = 0, nseq = 0, npad = 0, norph = 0, first = kNoShare;
  ShareHead owner{};
  for (uint32_t g = 0; g < k * k; g++) {
    ShareHead h;
    h.from_bytes(q0 + (size_t)(g / k) * row_pitch + (size_t)(g % k) * 512);
    const ShareRole role = share_role(g, h, prev, owner);
    if (role == kRoleOrphan) {
      if (!norph++) first = g;
    } else if (role == kRoleBreaks && nseq - 1 < cap) {
      out[nseq - 1].status |= CDA_SEQ_BROKEN;
    }
    if (!h.start()) continue;
    prev = h.mark(g);
    if (!h.sequence()) {
      npad++;
      continue;
    }
    owner = h;
    if (nseq < cap) h.record(g, k, threshold, out[nseq]);
    nseq++;
  }
  sum->k = k;
  sum->nseq = nseq;
  sum->npadding = npad;
  sum->norphans = norph;
  sum->first_orphan = first;
}

// ---- cda_square_read: where the payload of a sequence lies in its shares ----
// share j of a sequence holds its payload bytes from seq_share_off(j) on, after a header of seq_share_strip(j) bytes
CDA_HD uint32_t seq_share_strip(bool compact, uint32_t j) {
  return 512 - (j ? (compact ? kCompactNext : kSparseNext) : (compact ? kCompactFirst : kSparseFirst));
}
CDA_HD uint64_t seq_share_off(bool compact, uint32_t j) {
  const uint32_t first = compact ? kCompactFirst : kSparseFirst, next = compact ? kCompactNext : kSparseNext;
  return j ? (uint64_t)first + (uint64_t)(j - 1) * next : 0;
}

}  // namespace cda
