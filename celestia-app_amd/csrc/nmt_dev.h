// nmt_dev.h — device building blocks of the NMT and RFC-6962 hash kernels (nmt_kernels.hip, split_kernels.hip,
// inclusion_kernels.hip): the leaf message and record, the inner node in its three forms and level 1 by 2x2 cell quads
// in two, 96-B records to and from registers, the push-order compare, RFC-6962 digests and levels, and the level loops
// several kernels share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cda_internal.h"
#include "sha256_dev.h"

namespace cda {

__device__ __forceinline__ void load16(const uint4* p, uint32_t* w) {  // 4 x 16 B -> 16 words
#pragma unroll
  for (int i = 0; i < 4; i++) {
    uint4 v = p[i];
    w[4 * i + 0] = v.x;
    w[4 * i + 1] = v.y;
    w[4 * i + 2] = v.z;
    w[4 * i + 3] = v.w;
  }
}
// A 96-B record (6 x 16 B) to and from its 24 words
__device__ __forceinline__ void load_rec(const uint4* p, uint32_t (&r)[24]) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const uint4 v = p[i];
    r[4 * i + 0] = v.x;
    r[4 * i + 1] = v.y;
    r[4 * i + 2] = v.z;
    r[4 * i + 3] = v.w;
  }
}
__device__ __forceinline__ void store_rec(uint4* p, const uint32_t (&o)[24]) {
#pragma unroll
  for (int i = 0; i < 6; i++) p[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
}

// Big-endian namespace words of a 29-byte namespace held little-endian in n[0..7]
// (n[7] byte 0 = ns[28]) compared lexicographically: returns -1/0/1.
__device__ __forceinline__ int ns_cmp(const uint32_t* a, const uint32_t* b) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint32_t x = bswap(a[i]), y = bswap(b[i]);
    if (i == 7) {
      x >>= 24;
      y >>= 24;
    }
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}
// Push order (nmt ErrInvalidPushOrder): whether the share or leaf record at `next` has a smaller namespace than the
// one whose first words are in A.  Callers test Q0 neighbours only: parity leaves carry 0xFF x 29, the maximum.
__device__ __forceinline__ bool ns_below(const uint4* next, const uint32_t* A) {
  const uint4 v0 = next[0], v1 = next[1];
  const uint32_t nb[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
  return ns_cmp(nb, A) < 0;
}

// ---------------------------------------------------------------------------
// Leaf hashing: one thread per share.  The message is 0x00 ‖ ns ‖ share (542 bytes, 9 blocks), the record
// ns ‖ ns ‖ SHA256(message) ‖ 6 zero bytes, ns = share[0:29] if q0 else 0xFF x 29.
// ---------------------------------------------------------------------------
// A parity leaf's first block starts 0x00 ‖ 0xFF x 29 (message words 0..6 constant): its working state after rounds
// 0..6 is a constant, so those rounds are skipped (3 in 4 cells of a square are parity leaves).
constexpr uint32_t kParityLeafMid7[8] = {0x1ca5c518, 0x33e5c969, 0xbd2d00ce, 0xa4502bae,
                                         0xce23fa11, 0x90a5b516, 0x5df56d75, 0xf3f677da};
#ifndef CDA_NO_PARITY_MID
#define CDA_NO_PARITY_MID 0  // diagnostic A/B: every leaf and inner node through all 64 rounds of its first block
#endif

// Words 0..7 of block 0, 0x00 ‖ ns[0..29) ‖ share[0..2), for the namespace in the eight little-endian words NS (29
// bytes: the upper three bytes of NS[7] are not read) and the share's first word a0
__device__ __forceinline__ void leaf_block0_ns_words(const uint32_t* NS, uint32_t a0, uint32_t (&m)[16]) {
  m[0] = be_window(0u, NS[0], 3);
#pragma unroll
  for (int i = 1; i < 7; i++) m[i] = be_window(NS[i - 1], NS[i], 3);
  // bytes 28..31 = ns[27], ns[28], share[0], share[1]
  m[7] = (be_window(NS[6], NS[7], 3) & 0xFFFF0000u) | (bswap(a0) >> 16);
}
// Block 0 from the first 64 share bytes A: 0x00 ‖ ns[0..29) ‖ share[0..34), ns = share[0:29] if q0 else 0xFF x 29;
// with NS (a compile-time choice of the caller), the namespace supplied there instead
__device__ __forceinline__ void leaf_block0_words(const uint32_t (&A)[16], bool q0, uint32_t (&m)[16],
                                                  const uint32_t* NS = nullptr) {
  if (NS) {
    leaf_block0_ns_words(NS, A[0], m);
  } else if (q0) {
    leaf_block0_ns_words(A, A[0], m);
  } else {
    m[0] = 0x00FFFFFFu;
#pragma unroll
    for (int i = 1; i < 7; i++) m[i] = 0xFFFFFFFFu;
    m[7] = 0xFFFF0000u | (bswap(A[0]) >> 16);
  }
#pragma unroll
  for (int i = 8; i < 16; i++) m[i] = be_window(A[i - 8], A[i - 7], 2);
}
// Block j (1..8) holds share bytes 64j - 30 .. 64j + 33: windows of H = share words 16j - 8 .. 16j - 1 and
// C = share words 16j .. 16j + 15.  The last block (j = 8, no C) ends the message: share bytes 482..511, 0x80,
// zeros, the bit length.
__device__ __forceinline__ void leaf_block_words(const uint32_t* H, const uint32_t* C, bool last, uint32_t (&m)[16]) {
#pragma unroll
  for (int i = 0; i < 7; i++) m[i] = be_window(H[i], H[i + 1], 2);
  if (!last) {
    m[7] = be_window(H[7], C[0], 2);
#pragma unroll
    for (int i = 8; i < 16; i++) m[i] = be_window(C[i - 8], C[i - 7], 2);
  } else {
    m[7] = be_window(H[7], 0x80u, 2);
#pragma unroll
    for (int i = 8; i < 15; i++) m[i] = 0;
    m[15] = 542u * 8u;
  }
}
// Block j (1..8) read from the share itself (C stays unread, and is not loaded, for the last block)
__device__ __forceinline__ void leaf_block_words(const uint4* sh, int j, uint32_t (&m)[16]) {
  uint32_t H[8], C[16];
  {
    const uint4 a = sh[4 * j - 2], b = sh[4 * j - 1];
    H[0] = a.x, H[1] = a.y, H[2] = a.z, H[3] = a.w, H[4] = b.x, H[5] = b.y, H[6] = b.z, H[7] = b.w;
  }
  const bool last = !(j < 8);
  if (!last) load16(sh + 4 * j, C);
  leaf_block_words(H, C, last, m);
}

// Words 14..23 of a record: the namespace range's last two bytes (the low half of w14) ‖ the digest of the final
// state st ‖ 6 zero bytes
__device__ __forceinline__ void rec_digest_words(uint32_t w14, const uint32_t* st, uint32_t (&o)[24]) {
  uint32_t d[8];
#pragma unroll
  for (int i = 0; i < 8; i++) d[i] = bswap(st[i]);
  o[14] = (w14 & 0xFFFFu) | (d[0] << 16);
#pragma unroll
  for (int i = 15; i < 22; i++) o[i] = le_window(d[i - 15], d[i - 14], 2);
  o[22] = d[7] >> 16;
  o[23] = 0;
}

// The leaf record ns ‖ ns ‖ digest from the namespace words (as leaf_block0_ns_words takes them) and the final state
__device__ __forceinline__ void leaf_record_words(const uint32_t (&ns)[8], const uint32_t (&st)[8],
                                                  uint32_t (&o)[24]) {
#pragma unroll
  for (int i = 0; i < 7; i++) o[i] = ns[i];
  o[7] = (ns[7] & 0xFFu) | (ns[0] << 8);
#pragma unroll
  for (int i = 8; i < 14; i++) o[i] = le_window(ns[i - 8], ns[i - 7], 3);
  rec_digest_words(le_window(ns[6], ns[7], 3), st, o);
}
// The leaf record from the final state
__device__ __forceinline__ void leaf_record_out(const uint32_t (&A)[16], bool q0, const uint32_t (&st)[8], uint4* out) {
  uint32_t ns[8], o[24];
#pragma unroll
  for (int i = 0; i < 8; i++) ns[i] = q0 ? A[i] : 0xFFFFFFFFu;
  leaf_record_words(ns, st, o);
  store_rec(out, o);
}

// Leaf record of one 512-B share whose first 64 bytes are already in A.
// Blocks 1..7 stay a loop (one copy of the compression code: measured as fast as
// the unrolled form on MI355X, with half the instruction footprint).
// The share is read one 128-B line at a time (two 64-B chunks loaded together, the odd chunk held in N until its
// block): loaded a compression apart, the line's second half missed in L2 often enough that the leaf kernel fetched
// 1.31x its bytes (all 128-B requests, profiles/r04_rdreq_sizes.json).  PAIRS = false: one chunk per block (16
// fewer VGPRs; repair's root check, whose kernel would otherwise pass 128).
// leaf_digest_state is the hashing alone (st = the final state); with NS (a compile-time choice of the caller) the
// leaf's namespace is the one supplied there instead of a derived one: nmt Proof.VerifyInclusion's leaf (q0 is then not
// read, and NS is read for block 0 only: the caller builds the record with leaf_record_words).
template <bool PAIRS = true>
__device__ __forceinline__ void leaf_digest_state(const uint4* sh, const uint32_t (&A)[16], bool q0,
                                                  const uint32_t* NS, uint32_t (&st)[8]) {
  uint32_t N[16];
  if (PAIRS) load16(sh + 4, N);  // chunk 1, the rest of the line A came from
  uint32_t m[16];
  sha256_init(st);
  leaf_block0_words(A, q0, m, NS);
  // wave-uniform only (a wave of parity and Q0 cells runs all 64 rounds), and one copy of rounds 7..63 for both
  // cases: in a wave of parity cells m[0..6] already hold the constant words the schedule reads
  uint32_t mid[8];
#pragma unroll
  for (int i = 0; i < 8; i++) mid[i] = kParityLeafMid7[i];
  sha256_compress_skip<7>(st, mid, m, !NS && !CDA_NO_PARITY_MID && __all(!q0));
  uint32_t H[8];  // the upper half of the previous 16-word chunk
#pragma unroll
  for (int i = 0; i < 8; i++) H[i] = A[8 + i];
#pragma unroll 1
  for (int j = 1; j < 8; j++) {
    uint32_t C[16];
    if (!PAIRS) {
      load16(sh + 4 * j, C);
    } else if (j & 1) {  // odd chunk: loaded with the even one before it
#pragma unroll
      for (int i = 0; i < 16; i++) C[i] = N[i];
    } else {
      load16(sh + 4 * j, C);
      load16(sh + 4 * (j + 1), N);
    }
    leaf_block_words(H, C, false, m);
    sha256_compress(st, m);
#pragma unroll
    for (int i = 0; i < 8; i++) H[i] = C[8 + i];
  }
  leaf_block_words(H, nullptr, true, m);
  sha256_compress(st, m);
}
template <bool PAIRS = true>
__device__ __forceinline__ void leaf_record(const uint4* sh, const uint32_t (&A)[16], bool q0, uint4* out) {
  uint32_t st[8];
  leaf_digest_state<PAIRS>(sh, A, q0, nullptr, st);
  leaf_record_out(A, q0, st, out);
}

// One EDS cell `gid` (= blk * w^2 + r * w + c) of a batch: push-order check against
// its Q0 right / lower neighbours, then its 96-B leaf record.  With ods (the contiguous k x k ODS blocks, optional) a
// Q0 cell and its neighbours are read from there (rows k shares apart) and Q0 of eds is not read at all.
__device__ __forceinline__ void leaf_cell(const uint8_t* __restrict__ eds, uint4* __restrict__ nodes,
                                          unsigned long long* __restrict__ status, int k, int log2w, uint32_t gid,
                                          const uint8_t* __restrict__ ods = nullptr) {
  const int w = 1 << log2w;
  const uint32_t cell = gid & ((1u << (2 * log2w)) - 1);
  const uint32_t blk = gid >> (2 * log2w);
  const int r = (int)(cell >> log2w), c = (int)(cell & (w - 1));
  const bool q0 = (r < k) && (c < k);
  const bool from_ods = ods && q0;
  const uint4* sh = reinterpret_cast<const uint4*>(
      from_ods ? ods + ((size_t)blk * k * k + (size_t)r * k + c) * CDA_SHARE : eds + (size_t)gid * CDA_SHARE);

  uint32_t A[16];
  load16(sh, A);
  if (q0) {
    if (c + 1 < k && ns_below(sh + CDA_SHARE / 16, A)) {
      unsigned long long key = ((unsigned long long)CDA_AXIS_ROW << 40) | ((unsigned long long)r << 20) | (c + 1);
      atomicMin(status + blk, key);
    }
    if (r + 1 < k && ns_below(sh + (size_t)(from_ods ? k : w) * (CDA_SHARE / 16), A)) {
      unsigned long long key = ((unsigned long long)CDA_AXIS_COL << 40) | ((unsigned long long)c << 20) | (r + 1);
      atomicMin(status + blk, key);
    }
  }

  leaf_record(sh, A, q0, nodes + (size_t)gid * 6);
}

// ---------------------------------------------------------------------------
// Inner NMT node (also the in-place mountain fold of inclusion_kernels.hip).
// ---------------------------------------------------------------------------
// The node record from words 0..14 of both children (their namespace ranges) and the digest state:
// min = L.min; max = R.min == parity ns ? L.max : R.max.
__device__ __forceinline__ void node_record(const uint32_t* L, const uint32_t* R, const uint32_t (&st)[8],
                                            uint32_t (&o)[24]) {
  bool rmin_max = true;
#pragma unroll
  for (int i = 0; i < 7; i++) rmin_max &= (R[i] == 0xFFFFFFFFu);
  rmin_max &= ((R[7] & 0xFFu) == 0xFFu);
  uint32_t S[16];
#pragma unroll
  for (int i = 7; i < 15; i++) S[i] = rmin_max ? L[i] : R[i];
#pragma unroll
  for (int i = 0; i < 7; i++) o[i] = L[i];
  o[7] = (L[7] & 0xFFu) | (S[7] & 0xFFFFFF00u);
#pragma unroll
  for (int i = 8; i < 14; i++) o[i] = S[i];
  rec_digest_words(S[14], st, o);
}

// Message blocks 0..2 of an inner node, 0x01 ‖ L[0..90) ‖ R[0..90) ‖ 0x80 ‖ 0.. ‖ len(1448 bits) (48 words), from the
// child records in memory.  Block 0 takes a laundered pointer; blocks 1 and 2 launder theirs after `after` (a word of
// the previous compression's state), see hash_node_mem.  ns_lds (optional): the first 64 B of L (block 0) / R (block
// 1) are parked there.
__device__ __forceinline__ void node_mem_block0(const uint4* pl, uint32_t (&m)[16], uint4* ns_lds = nullptr) {
  // words 0..15 <- L words 0..15
  uint32_t L[16];
  load16(pl, L);
  m[0] = be_window(0x01000000u, L[0], 3);
#pragma unroll
  for (int i = 1; i < 16; i++) m[i] = be_window(L[i - 1], L[i], 3);
  if (ns_lds)
#pragma unroll
    for (int i = 0; i < 4; i++) ns_lds[i] = make_uint4(L[4 * i], L[4 * i + 1], L[4 * i + 2], L[4 * i + 3]);
}
__device__ __forceinline__ void node_mem_block1(const uint4* pl, const uint4* pr, uint32_t after, uint32_t (&m)[16],
                                                uint4* ns_lds = nullptr) {
  // words 16..31 <- L words 15..22, R words 0..8
  uint32_t L[16], R[16];  // L words 12..27, R words 0..15
  load16(launder_after(pl, after) + 3, L);  // words 12..27: only 12..23 are read
  load16(launder_after(pr, after), R);      // words 0..15: only 0..11 are read
  if (ns_lds)
#pragma unroll
    for (int i = 0; i < 4; i++) ns_lds[4 + i] = make_uint4(R[4 * i], R[4 * i + 1], R[4 * i + 2], R[4 * i + 3]);
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int wi = 16 + i;
    if (wi <= 21) m[i] = be_window(L[wi - 13], L[wi - 12], 3);
    else if (wi == 22) m[i] = be_window(L[9], L[10], 3) | (R[0] & 0xFFu);
    else m[i] = be_window(R[wi - 23], R[wi - 22], 1);
  }
}
__device__ __forceinline__ void node_mem_block2(const uint4* pr, uint32_t after, uint32_t (&m)[16]) {
  // words 32..47 <- R words 8..23
  uint32_t R[16];
  load16(launder_after(pr, after) + 2, R);
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int wi = 32 + i;
    if (wi <= 44) m[i] = be_window(R[wi - 31], R[wi - 30], 1);
    else if (wi == 45) m[i] = be_window(R[14], R[15], 1) | 0x00800000u;
    else if (wi == 46) m[i] = 0;
    else m[i] = 181u * 8u;
  }
}

// Inner node from the two child records at pl / pr, written to po (po may equal
// pl: every read precedes the stores).  The children are read block by block
// through laundered pointers ordered after the previous compression, so the
// reads are neither merged nor hoisted and kept live, and each compression is
// fenced: 89 VGPRs (5 waves/SIMD) instead of 205 when both children stayed in
// registers.
// ns_lds (optional): this thread's 128-B LDS slot; the first 64 B of both children are parked there when loaded for
// blocks 0 / 1 and the namespace range is read back from it instead of from global memory.  With the slots 128 B
// apart, lane i's piece j shares banks with every other lane's piece j (8-way conflicts on ds_write_b128 /
// ds_read_b128).  Swizzling the pieces (piece ^ ((lane ^ lane >> 3) & 7)) removed every conflict of the levels 1-2
// launch (SQ_LDS_BANK_CONFLICT 132 M -> 0) but moved blocks/s by +0.3 / +0.9 % on two boxes (the kernel is
// VALU-bound): below the 1 % bar, not kept.
__device__ __forceinline__ void hash_node_mem(const uint4* pl, const uint4* pr, uint4* po, bool store = true,
                                              uint4* ns_lds = nullptr) {
  uint32_t st[8], m[16];
  sha256_init(st);
  node_mem_block0(launder(pl), m, ns_lds);
  sha256_compress_fenced(st, m);
  node_mem_block1(pl, pr, st[0], m, ns_lds);
  sha256_compress_fenced(st, m);
  node_mem_block2(pr, st[0], m);
  sha256_compress_fenced(st, m);

  // the namespace range comes from the children's first 16 words, read again
  uint32_t L[16], R[16];
  if (ns_lds) {
    uint32_t z = 0;  // an offset tied to the last compression keeps the LDS reads below it (pointer stays in LDS)
    asm volatile("" : "+v"(z) : "v"(st[0]));
    load16(ns_lds + z, L);
    load16(ns_lds + z + 4, R);
#pragma unroll
    for (int i = 0; i < 16; i++) asm volatile("" : "+v"(L[i]), "+v"(R[i]));  // values, not a select of addresses
  } else {
    load16(launder_after(pl, st[0]), L);
    load16(launder_after(pr, st[0]), R);
  }
  uint32_t o[24];
  node_record(L, R, st, o);
  if (store) store_rec(po, o);
}

// Inner node whose children both lie in the parity part of the square: every leaf below them has the parity
// namespace, so each child is 0xFF x 58 ‖ digest ‖ 6 zero bytes.  About 3 in 4 inner nodes of a square are such (rows
// / columns >= k entirely, the right half of the others).  Only record words 12..23 of each child are read (the
// digest and the bytes around it; 96 B per node instead of 256), the constant message words are literals and the
// record's namespace range is 0xFF x 58 without a compare: no LDS parking.  Block 0 is 0x01 ‖ 0xFF x 58 ‖ 5 digest
// bytes: its first 14 rounds run on constant words from a constant state and are skipped (kParityMid14), 14 of the
// node's 192 rounds; w23..w36 = 0xFFFFFFFF, w46 = 0, w47 = 1448 fold into the schedules of blocks 1 and 2.
// For whole waves only: in a wave whose nodes are partly parity both this and hash_node_mem would run (measured 3 %
// slower on the step with the midstate alone, profiles/r06_ab_parity_mid.jsonl), so callers test __all(parity).
// Records as pl / pr / po of hash_node_mem (po may equal pl).
constexpr uint32_t kParityMid14[8] = {0xa8abd42b, 0x092979bd, 0x8d5926ca, 0x8df58526,
                                      0xa812caa9, 0x7cc8da5d, 0x33a85111, 0x7d669380};
// Message blocks of a parity node; pointers and `after` as in node_mem_block*.  Block 0 returns L word 15 (loaded with
// it) for block 1.
__device__ __forceinline__ uint32_t parity_block0(const uint4* pl, uint32_t (&m)[16]) {
  // 0x01 ‖ 0xFF x 58 ‖ L digest bytes 0..4
  const uint4 v = pl[3];
  m[0] = 0x01FFFFFFu;
#pragma unroll
  for (int i = 1; i < 14; i++) m[i] = 0xFFFFFFFFu;
  m[14] = be_window(v.y, v.z, 3);
  m[15] = be_window(v.z, v.w, 3);
  return v.w;
}
__device__ __forceinline__ void parity_block1(const uint4* pl, uint32_t after, uint32_t l15, uint32_t (&m)[16]) {
  uint32_t L[12];  // L words 12..23: 15..22 are read
  L[3] = l15;
  {
    const uint4* p = launder_after(pl, after) + 3;
#pragma unroll
    for (int i = 1; i < 3; i++) {
      const uint4 v = p[i];
      L[4 * i] = v.x, L[4 * i + 1] = v.y, L[4 * i + 2] = v.z, L[4 * i + 3] = v.w;
    }
  }
  // L digest bytes 5..31 ‖ R's 0xFF x 37
#pragma unroll
  for (int i = 0; i < 6; i++) m[i] = be_window(L[3 + i], L[4 + i], 3);  // words 16..21 <- L words 15..21
  m[6] = be_window(L[9], L[10], 3) | 0xFFu;                              // word 22: L bytes 87..89, R byte 0
#pragma unroll
  for (int i = 7; i < 16; i++) m[i] = 0xFFFFFFFFu;
}
__device__ __forceinline__ void parity_block2(const uint4* pr, uint32_t after, uint32_t (&m)[16]) {
  uint32_t R[12];  // R words 12..23: 14..23 are read
  {
    const uint4* p = launder_after(pr, after) + 3;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const uint4 v = p[i];
      R[4 * i] = v.x, R[4 * i + 1] = v.y, R[4 * i + 2] = v.z, R[4 * i + 3] = v.w;
    }
  }
  // R's 0xFF x 21 ‖ R digest ‖ 0x80 ‖ 0.. ‖ len
#pragma unroll
  for (int i = 0; i < 5; i++) m[i] = 0xFFFFFFFFu;
#pragma unroll
  for (int i = 5; i < 13; i++) m[i] = be_window(R[i - 3], R[i - 2], 1);  // words 37..44 <- R words 14..22
  m[13] = be_window(R[10], R[11], 1) | 0x00800000u;
  m[14] = 0;
  m[15] = 181u * 8u;
}
// Block 0 of a parity node into the initial state st, from kParityMid14
__device__ __forceinline__ uint32_t parity_compress_block0(const uint4* pl, uint32_t (&st)[8], uint32_t (&m)[16]) {
  sha256_init(st);
  const uint32_t l15 = parity_block0(pl, m);
  uint32_t mid[8];
#pragma unroll
  for (int i = 0; i < 8; i++) mid[i] = kParityMid14[i];
  sha256_compress_fenced_from<14>(st, mid, m);
  return l15;
}
// The record of a parity node: 0xFF x 58 ‖ digest ‖ 6 zero bytes
__device__ __forceinline__ void parity_record(const uint32_t* st, uint32_t (&o)[24]) {
#pragma unroll
  for (int i = 0; i < 14; i++) o[i] = 0xFFFFFFFFu;
  rec_digest_words(0xFFFFu, st, o);
}
__device__ __forceinline__ void hash_node_parity(const uint4* pl, const uint4* pr, uint4* po, bool store = true) {
  uint32_t st[8], m[16];
  // the words are read block by block, each load ordered after the previous compression (as in hash_node_mem)
  const uint32_t l15 = parity_compress_block0(launder(pl), st, m);
  parity_block1(pl, st[0], l15, m);
  sha256_compress_fenced(st, m);
  parity_block2(pr, st[0], m);
  sha256_compress_fenced(st, m);
  uint32_t o[24];
  parity_record(st, o);
  if (store) store_rec(po, o);
}

// ---------------------------------------------------------------------------
// Level 1 by 2x2 cell quads.  The cells TL, TR / BL, BR at rows 2R, 2R+1 and columns 2C, 2C+1 have four level-1
// parents: row-top (TL, TR), row-bottom (BL, BR), col-left (TL, BL), col-right (TR, BR).  Row-top and col-left share
// their left child, so block 0 (0x01 ‖ L[0..63), left child only) is the same compression from the same IV; in a
// parity quad block 1 (L digest tail ‖ 0xFF x 37) is too.  Row-bottom and col-right share their right child, so block
// 2 (R[37..90) ‖ pad) is one message into two chaining states: one schedule, two round chains
// (sha256_compress_fenced_2s).  Children are read piecewise through laundered pointers ordered after the previous
// compression, as in the node forms above.  Records and their bytes are those of hash_node_mem / hash_node_parity.
// The two nodes of a pair run the same blocks on other children, so each pair is a loop of two trips over one copy of
// the code (18.2 k instead of 27.5 k VALU instructions in nmt_level1_quads_kernel; measured no slower than unrolled,
// DESIGN.md §21); the states the shared block 2 needs leave the loop through statically indexed copies.
// ---------------------------------------------------------------------------
// The record of the node with children pl / pr and final state st, to po: the namespace range from the children's
// first 16 words, read (again) after `after`
__device__ __forceinline__ void node_record_mem(const uint4* pl, const uint4* pr, uint32_t after, const uint32_t* stp,
                                                uint4* po) {
  uint32_t L[16], R[16], st[8], o[24];
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] = stp[i];
  load16(launder_after(pl, after), L);
  load16(launder_after(pr, after), R);
  node_record(L, R, st, o);
  store_rec(po, o);
}
// General form: valid for any quad.
__device__ __forceinline__ void hash_quad_mem(const uint4* tl, const uint4* tr, const uint4* bl, const uint4* br,
                                              uint4* row_top, uint4* row_bot, uint4* col_left, uint4* col_right) {
  uint32_t s0[8], st[8], m[16];
  sha256_init(s0);
  node_mem_block0(launder(tl), m);  // block 0 of TL, once for row-top and col-left
  sha256_compress_fenced(s0, m);
  uint32_t after = s0[0];
#pragma unroll 1
  for (int n = 0; n < 2; n++) {  // row-top (TL, TR), then col-left (TL, BL), both from s0
    const uint4* pr = n == 0 ? tr : bl;
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = s0[i];
    node_mem_block1(tl, pr, after, m);
    sha256_compress_fenced(st, m);
    node_mem_block2(pr, st[0], m);
    sha256_compress_fenced(st, m);
    node_record_mem(tl, pr, st[0], st, n == 0 ? row_top : col_left);
    after = st[0];
  }
  uint32_t S[2][8];  // row-bottom (BL, BR), col-right (TR, BR): blocks 0 and 1 each, block 2 with one schedule
#pragma unroll 1
  for (int n = 0; n < 2; n++) {
    const uint4* pl = n == 0 ? bl : tr;
    sha256_init(st);
    node_mem_block0(launder_after(pl, after), m);
    sha256_compress_fenced(st, m);
    node_mem_block1(pl, br, st[0], m);
    sha256_compress_fenced(st, m);
    after = st[0];
#pragma unroll
    for (int i = 0; i < 8; i++) {  // S[n] would be a runtime index: scratch
      if (n == 0) S[0][i] = st[i];
      else S[1][i] = st[i];
    }
  }
  node_mem_block2(br, after, m);
  sha256_compress_fenced_2s(S, m);
  node_record_mem(bl, br, S[1][0], S[0], row_bot);
  node_record_mem(tr, br, S[1][0], S[1], col_right);
}
// Parity form: every cell of the quad is a parity leaf (whole waves only, as hash_node_parity).  Blocks 0 and 1 of TL
// once; block 2 of row-top (TR) and col-left (BL) are two messages from that one state.
__device__ __forceinline__ void hash_quad_parity(const uint4* tl, const uint4* tr, const uint4* bl, const uint4* br,
                                                 uint4* row_top, uint4* row_bot, uint4* col_left, uint4* col_right) {
  uint32_t S[2][8], m[16], o[24];
  uint32_t after;
  {
    uint32_t s1[8], st[8];
    const uint32_t l15 = parity_compress_block0(launder(tl), s1, m);
    parity_block1(tl, s1[0], l15, m);
    sha256_compress_fenced(s1, m);
    after = s1[0];
    // one after the other, not sha256_compress_n<2, 8>: with two schedules in registers the kernel spilled 44 VGPRs
    // at 128, and at 4 waves per SIMD the second chain's instruction-level parallelism buys nothing
#pragma unroll 1
    for (int n = 0; n < 2; n++) {  // row-top (TR), then col-left (BL)
#pragma unroll
      for (int i = 0; i < 8; i++) st[i] = s1[i];
      parity_block2(n == 0 ? tr : bl, after, m);
      sha256_compress_fenced(st, m);
      parity_record(st, o);
      store_rec(n == 0 ? row_top : col_left, o);
      after = st[0];
    }
  }
#pragma unroll 1
  for (int n = 0; n < 2; n++) {  // row-bottom (BL, BR), col-right (TR, BR)
    const uint4* pl = n == 0 ? bl : tr;
    uint32_t st[8];
    const uint32_t l15 = parity_compress_block0(launder_after(pl, after), st, m);
    parity_block1(pl, st[0], l15, m);
    sha256_compress_fenced(st, m);
    after = st[0];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      if (n == 0) S[0][i] = st[i];
      else S[1][i] = st[i];
    }
  }
  parity_block2(br, after, m);
  sha256_compress_fenced_2s(S, m);
  parity_record(S[0], o);
  store_rec(row_bot, o);
  parity_record(S[1], o);
  store_rec(col_right, o);
}

// Message block B (0..2) of an inner node: 0x01 ‖ L[0..90) ‖ R[0..90) ‖ 0x80 ‖ 0.. ‖ len(1448 bits), children in
// record layout (24 words each).
template <int B>
__device__ __forceinline__ void node_block(const uint32_t (&L)[24], const uint32_t (&R)[24], uint32_t (&m)[16]) {
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int wi = 16 * B + i;
    if (wi == 0) m[i] = be_window(0x01000000u, L[0], 3);
    else if (wi <= 21) m[i] = be_window(L[wi - 1], L[wi], 3);
    else if (wi == 22) m[i] = be_window(L[21], L[22], 3) | (R[0] & 0xFFu);
    else if (wi <= 44) m[i] = be_window(R[wi - 23], R[wi - 22], 1);
    else if (wi == 45) m[i] = be_window(R[22], R[23], 1) | 0x00800000u;
    else if (wi == 46) m[i] = 0;
    else m[i] = 181u * 8u;
  }
}
// hash_node_mem with both children already in registers (24 words each, record layout): the form for latency
// kernels that run one wave per SIMD, where registers are free and a memory round trip per compression is not.
__device__ __forceinline__ void hash_node_regs(const uint32_t (&L)[24], const uint32_t (&R)[24], uint32_t (&o)[24]) {
  uint32_t st[8], m[16];
  sha256_init(st);
  node_block<0>(L, R, m);
  sha256_compress(st, m);
  node_block<1>(L, R, m);
  sha256_compress(st, m);
  node_block<2>(L, R, m);
  sha256_compress(st, m);
  node_record(L, R, st, o);
}

// A tree folded in place in LDS: node i of level l sits at slot i << l of lnodes (a last odd node keeps its slot,
// which is the nmt split at the largest power of two below n).  lds_node_mem hashes one node from its two children
// at level l - 1; lds_level_mem the level's `pairs` nodes by the whole workgroup.
__device__ __forceinline__ void lds_node_mem(uint4* lnodes, int l, int i, bool store = true) {
  hash_node_mem(lnodes + ((size_t)(2 * i) << (l - 1)) * 6, lnodes + ((size_t)(2 * i + 1) << (l - 1)) * 6,
                lnodes + ((size_t)i << l) * 6, store);
}
__device__ __forceinline__ void lds_level_mem(uint4* lnodes, int l, int pairs) {
  for (int i = threadIdx.x; i < pairs; i += blockDim.x) lds_node_mem(lnodes, l, i);
}

// ---------------------------------------------------------------------------
// RFC-6962 (merkle.HashFromByteSlices) over NMT nodes; digests are 8 big-endian words.
// ---------------------------------------------------------------------------
// Leaf digest SHA256(0x00 ‖ record[0..90)) of a node record; message block B of it
template <int B>
__device__ __forceinline__ void dah_leaf_block(const uint32_t (&L)[24], uint32_t (&m)[16]) {
  // 0x00 ‖ root[0..90) ‖ 0x80 ‖ ... ‖ len(91*8)
#pragma unroll
  for (int t = 0; t < 16; t++) {
    const int wi = 16 * B + t;
    if (wi == 0) m[t] = be_window(0u, L[0], 3);
    else if (wi <= 21) m[t] = be_window(L[wi - 1], L[wi], 3);
    else if (wi == 22) m[t] = be_window(L[21], L[22], 3) | 0x80u;
    else if (wi < 31) m[t] = 0;
    else m[t] = 91u * 8u;
  }
}
__device__ __forceinline__ void dah_leaf_digest(const uint32_t (&L)[24], uint32_t (&st)[8]) {
  uint32_t m[16];
  sha256_init(st);
  dah_leaf_block<0>(L, m);
  sha256_compress(st, m);
  dah_leaf_block<1>(L, m);
  sha256_compress(st, m);
}
// Inner node message block B of digests Ld, Rd: 0x01 ‖ Ld ‖ Rd ‖ pad, 65 bytes
template <int B>
__device__ __forceinline__ void rfc_node_block(const uint32_t* Ld, const uint32_t* Rd, uint32_t (&m)[16]) {
  if (B == 0) {
    m[0] = 0x01000000u | (Ld[0] >> 8);
#pragma unroll
    for (int t = 1; t < 8; t++) m[t] = (Ld[t - 1] << 24) | (Ld[t] >> 8);
    m[8] = (Ld[7] << 24) | (Rd[0] >> 8);
#pragma unroll
    for (int t = 9; t < 16; t++) m[t] = (Rd[t - 9] << 24) | (Rd[t - 8] >> 8);
  } else {
    m[0] = (Rd[7] << 24) | 0x00800000u;
#pragma unroll
    for (int t = 1; t < 15; t++) m[t] = 0;
    m[15] = 65u * 8u;
  }
}
// One level by the whole workgroup, a node per thread: the cnt digests at src to (cnt + 1) / 2 at dst.  Levels pair
// (2i, 2i+1) and promote an odd last node, which is the same tree as HashFromByteSlices' "split at the largest power
// of two below n" recursion.  nodes_out (optional): the level's digests as bytes, node i at nodes_out + 32 i.
__device__ __forceinline__ void rfc_level_wide(const uint32_t* src, uint32_t* dst, int cnt, uint32_t* nodes_out) {
  const int out_cnt = (cnt + 1) >> 1;
  for (int i = threadIdx.x; i < out_cnt; i += blockDim.x) {
    uint32_t* o = dst + i * 8;
    const uint32_t* Ld = src + (2 * i) * 8;
    if (2 * i + 1 < cnt) {
      const uint32_t* Rd = src + (2 * i + 1) * 8;
      uint32_t st[8], m[16];
      sha256_init(st);
      rfc_node_block<0>(Ld, Rd, m);
      sha256_compress(st, m);
      rfc_node_block<1>(Ld, Rd, m);
      sha256_compress(st, m);
#pragma unroll
      for (int t = 0; t < 8; t++) o[t] = st[t];
    } else {
#pragma unroll
      for (int t = 0; t < 8; t++) o[t] = Ld[t];
    }
    if (nodes_out) {
#pragma unroll
      for (int t = 0; t < 8; t++) nodes_out[(size_t)i * 8 + t] = bswap(o[t]);
    }
  }
}


// ---------------------------------------------------------------------------
// DAH fold (nmt_kernels.hip dah_kernel / dah_tree_kernel / dah_wide_kernel / trees_lds_kernel, small_square_kernels.hip)
// ---------------------------------------------------------------------------
// RFC-6962 levels over the n leaf digests at sdig ([n + (n+1)/2][8] words of LDS, the first n filled), by the
// calling workgroup (>= 128 threads); the 32-B hash goes to out.  Wide levels a node per thread (rfc_level_wide).  Once
// a level has at most 64 nodes (its chain of dependent compressions is the latency), wave 0 hashes block 0 of each
// node while wave 1 expands the node's second message block into kw (64 x kKwStride words of LDS), and the second
// compression then runs its rounds alone.  NODES: every level's digests also go to nodes_out as bytes, level by level
// after the n leaf digests the caller wrote there (the tree cda_extend_commit_nodes exports as dah_nodes); without
// it the code is what it was.
template <bool NODES = false>
__device__ __forceinline__ void dah_fold_kw(uint32_t* sdig, int n, uint32_t* out, uint32_t* kw,
                                            uint32_t* nodes_out = nullptr) {
  uint32_t* src = sdig;
  uint32_t* dst = sdig + n * 8;
  size_t base = (size_t)n;  // NODES: nodes of the levels below the one being written
  for (int cnt = n; cnt > 1;) {
    const int out_cnt = (cnt + 1) >> 1;
    if (out_cnt > 64) {
      rfc_level_wide(src, dst, cnt, nullptr);
    } else {
      // every lane of waves 0 and 1 computes, with full exec masks (lanes past the level's pairs hash stale,
      // in-bounds LDS words and store nothing), as in trees_lds_kernel
      const int i = threadIdx.x & 63;
      const bool pair = i < out_cnt && 2 * i + 1 < cnt;
      uint32_t st[8];
      if (threadIdx.x < 64) {
        const uint32_t* Ld = src + (2 * i) * 8;
        if (i < out_cnt && !pair)
#pragma unroll
          for (int t = 0; t < 8; t++) dst[i * 8 + t] = Ld[t];
        uint32_t m[16];
        sha256_init(st);
        rfc_node_block<0>(Ld, src + (2 * i + 1) * 8, m);
        sha256_compress(st, m);
      } else if (threadIdx.x < 128) {
        uint32_t m[16];
        rfc_node_block<1>(src + (2 * i) * 8, src + (2 * i + 1) * 8, m);
        sha256_kw_store(m, kw + i * kKwStride);
      }
      __syncthreads();
      if (threadIdx.x < 64) {
        sha256_rounds_kw(st, kw + i * kKwStride);
        if (pair)
#pragma unroll
          for (int t = 0; t < 8; t++) dst[i * 8 + t] = st[t];
      }
    }
    __syncthreads();
    if (NODES) {
      for (int i = threadIdx.x; i < out_cnt * 8; i += blockDim.x) nodes_out[base * 8 + i] = bswap(dst[i]);
      base += out_cnt;
    }
    uint32_t* tmp = src;
    src = dst;
    dst = tmp;
    cnt = out_cnt;
  }
  if (threadIdx.x < 8) out[threadIdx.x] = bswap(src[threadIdx.x]);
}

}  // namespace cda
