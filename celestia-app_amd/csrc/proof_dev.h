// proof_dev.h — the device pieces that more than one of the proof kernel files use (sampling_kernels.hip,
// share_proof_kernels.hip, namespace_kernels.hip, commitment_kernels.hip): where a node of a retained square lies and
// the gather of a range proof out of it, packed nodes into registers and LDS slots, one link of a one-leaf proof's
// chain, and the workgroup fold of a longer span.  Device code only: .hip files include it, no host header does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cda_internal.h"
#include "nmt_dev.h"
#include "nmt_verify_rule.h"
#include "sampling.h"
#include "sha256_dev.h"

namespace cda {

// Record of node (height h, position p) of tree (axis, index) in the retained square
__device__ __forceinline__ const uint8_t* square_node(const SquareView& v, uint32_t axis, uint32_t index, int h,
                                                      uint32_t p) {
  const uint32_t w = 1u << v.log2w;
  if (h == 0) {
    const size_t cell = axis ? (size_t)p * w + index : (size_t)index * w + p;
    return v.leaf + cell * CDA_REC_BYTES;
  }
  const size_t rec = square_level_offset(v.log2w, h) + ((size_t)(axis * w + index) << (v.log2w - h)) + p;
  return v.levels + rec * CDA_REC_BYTES;
}

// Reference semantics (celestia-app @ 2025-02-13, nmt v0.22):
//   ProveRange(start, end) of an erasured tree (pkg/wrapper/nmt_wrapper.go:127-130 -> nmt buildRangeProof): the roots
//   of the maximal subtrees outside [start, end), left to right.  On the perfect tree of 2k leaves these are, left of
//   the range, one node per set bit of start (highest bit first) and, right of it, one per set bit of 2k - end
//   (lowest bit first): no walk of the tree, a node's height and position follow from the bit.
//
// ProveRange(start, end) of tree (axis, index) by a group of 32 lanes (the whole group calls it): lane i finds node i
// of the proof (a bit of start or of 2k - end); the group then copies the nodes slot by slot into `slots` (max_nodes
// slots of 90 B), 2 bytes per lane (a 90-byte slot is 2-byte aligned), and zero-fills the unused slots.  Returns the
// number of nodes.  The one copy of the bit rule: square_prove_kernel and square_share_proofs_kernel both call it.
__device__ __forceinline__ uint32_t gather_range_proof(const SquareView& v, uint32_t axis, uint32_t index,
                                                       uint32_t start, uint32_t end, uint32_t lane, uint32_t max_nodes,
                                                       uint8_t* __restrict__ slots) {
  const uint32_t w = 1u << v.log2w, s = start, r = w - end;
  const uint32_t nl = __popc(s), cnt = nl + __popc(r);
  unsigned long long src = 0;
  if (lane < cnt) {
    int b = 0;
    uint32_t p;
    if (lane < nl) {  // left of the range: the set bits of start, highest first
      uint32_t m = s;
      for (uint32_t i = 0; i <= lane; i++) {
        b = 31 - __clz(m);
        m &= ~(1u << b);
      }
      p = (s >> b) - 1;
    } else {  // right of it: the set bits of 2k - end, lowest first
      uint32_t m = r;
      for (uint32_t i = nl; i <= lane; i++) {
        b = __ffs(m) - 1;
        m &= m - 1;
      }
      p = (w >> b) - (r >> b);
    }
    src = (unsigned long long)(uintptr_t)square_node(v, axis, index, b, p);
  }
  for (uint32_t i = 0; i < max_nodes; i++) {
    const unsigned long long sp = i < 32 ? __shfl(src, (int)i, 32) : 0ull;
    const uint16_t* from = reinterpret_cast<const uint16_t*>((uintptr_t)sp);
    uint16_t* to = reinterpret_cast<uint16_t*>(slots + (size_t)i * CDA_NODE_SIZE);
    for (uint32_t hw = lane; hw < CDA_NODE_SIZE / 2; hw += 32) to[hw] = sp ? from[hw] : (uint16_t)0;
  }
  return cnt;
}

// Row `row`'s root and its RFC-6962 proof in the data root into the slots of row record r, by a group of 32 lanes: the
// root (the one node of level log2(2k)), its leaf hash and aunt h = node (row >> h) ^ 1 of level h of the retained
// data-root tree.  square_share_proofs_kernel and square_commitment_proofs_kernel both call it.
__device__ __forceinline__ void copy_row_root_proof(const SquareView& v, uint32_t row, uint32_t r, uint32_t lane,
                                                    uint8_t* __restrict__ row_roots, uint8_t* __restrict__ leaf_hashes,
                                                    uint8_t* __restrict__ aunts) {
  const uint32_t w = 1u << v.log2w, naunts = (uint32_t)v.log2w + 1;
  const uint16_t* root = reinterpret_cast<const uint16_t*>(square_node(v, CDA_AXIS_ROW, row, v.log2w, 0));
  uint16_t* root_out = reinterpret_cast<uint16_t*>(row_roots + (size_t)r * CDA_NODE_SIZE);
  for (uint32_t hw = lane; hw < CDA_NODE_SIZE / 2; hw += 32) root_out[hw] = root[hw];
  const uint32_t* dn = reinterpret_cast<const uint32_t*>(v.dah_nodes);
  if (lane < 8) reinterpret_cast<uint32_t*>(leaf_hashes)[(size_t)r * 8 + lane] = dn[(size_t)row * 8 + lane];
  uint32_t* aunts_out = reinterpret_cast<uint32_t*>(aunts) + (size_t)r * naunts * 8;
  for (uint32_t i = lane; i < naunts * 8; i += 32) {
    const uint32_t h = i >> 3;
    const size_t node = (size_t)(4 * w - ((4 * w) >> h)) + ((row >> h) ^ 1u);  // level h starts 2N - (2N >> h) nodes in
    aunts_out[i] = dn[node * 8 + (i & 7)];
  }
}

// The 29 namespace bytes at p (any alignment) as the eight words leaf_block0_ns_words takes
__device__ __forceinline__ void load_ns(const uint8_t* p, uint32_t (&ns)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    ns[i] = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (4 * i + j < CDA_NAMESPACE_SIZE) ns[i] |= (uint32_t)p[4 * i + j] << (8 * j);
  }
}

// Node idx of a packed array of 90-byte nodes (base 4-byte aligned) as a record in registers.  A node starts on a
// 4-byte boundary or 2 bytes past one: 22 aligned words plus one halfword cover exactly its 90 bytes in both cases
// (no byte outside the node is read), and the odd case shifts the words by two bytes.
__device__ __forceinline__ void load_node_regs(const uint8_t* base, uint32_t idx, uint32_t (&r)[24]) {
  const uint8_t* p = base + (size_t)idx * CDA_NODE_SIZE;
  const bool odd = idx & 1;  // 90 idx = 2 (mod 4)
  const uint32_t* x = reinterpret_cast<const uint32_t*>(p + (odd ? 2 : 0));
  const uint32_t y = *reinterpret_cast<const uint16_t*>(p + (odd ? 0 : CDA_NODE_SIZE - 2));
  uint32_t prev = y << 16;
#pragma unroll
  for (int i = 0; i < 22; i++) {
    const uint32_t v = x[i];
    r[i] = odd ? __builtin_amdgcn_alignbit(v, prev, 16) : v;
    prev = v;
  }
  r[22] = odd ? prev >> 16 : y;
  r[23] = 0;
}

// nmt ValidateSiblings: left.max (record bytes 29..57) > right.min (bytes 0..28)
__device__ __forceinline__ bool siblings_out_of_order(const uint32_t* L, const uint32_t* R) {
  uint32_t mx[8];
#pragma unroll
  for (int i = 0; i < 8; i++) mx[i] = le_window(L[7 + i], L[8 + i], 1);
  return ns_cmp(mx, R) > 0;
}

// The first 90 bytes of two records
__device__ __forceinline__ bool node_equal(const uint32_t* a, const uint32_t* b) {
  uint32_t diff = (a[22] ^ b[22]) & 0xFFFFu;
#pragma unroll
  for (int i = 0; i < 22; i++) diff |= a[i] ^ b[i];
  return diff == 0;
}

// One link of a one-leaf proof's chain: cur <- node(sibling, cur) if sib_left, else node(cur, sibling), the sibling
// node idx of the packed array `nodes`; returns ValidateSiblings' verdict (true: out of order).  Which child the
// running node is differs from lane to lane, so the children are chosen word by word (one copy of the hash for both
// cases).  The sibling is read again for every message block and for the record, each read ordered after the
// compression before it: with both children held in registers across the three compressions the kernel needs 144
// VGPRs, with the running node alone it stays inside the 128 of 4 waves per SIMD (the re-reads hit in L2: 92 loads
// beside 4,300 instructions of hashing).
__device__ __forceinline__ void chain_children(const uint32_t (&cur)[24], const uint8_t* nodes, uint32_t idx,
                                               bool sib_left, uint32_t (&L)[24], uint32_t (&R)[24]) {
  uint32_t sib[24];
  load_node_regs(nodes, idx, sib);
#pragma unroll
  for (int i = 0; i < 24; i++) {
    L[i] = sib_left ? sib[i] : cur[i];
    R[i] = sib_left ? cur[i] : sib[i];
  }
}
__device__ __forceinline__ bool chain_node(uint32_t (&cur)[24], const uint8_t* nodes, uint32_t idx, bool sib_left) {
  uint32_t st[8], m[16], L[24], R[24];
  sha256_init(st);
  // opaque: the round-0 terms of the constant initial state (bitop3 is not folded) would otherwise be computed once in
  // the leaf's first block and kept in a VGPR for every node
#pragma unroll
  for (int i = 0; i < 8; i++) asm volatile("" : "+v"(st[i]));
  chain_children(cur, launder(nodes), idx, sib_left, L, R);
  node_block<0>(L, R, m);
  sha256_compress_fenced(st, m);
  chain_children(cur, launder_after(nodes, st[0]), idx, sib_left, L, R);
  node_block<1>(L, R, m);
  sha256_compress_fenced(st, m);
  chain_children(cur, launder_after(nodes, st[0]), idx, sib_left, L, R);
  node_block<2>(L, R, m);
  sha256_compress_fenced(st, m);
  chain_children(cur, launder_after(nodes, st[0]), idx, sib_left, L, R);
  const bool bad = siblings_out_of_order(L, R);
  uint32_t o[24];
  node_record(L, R, st, o);
#pragma unroll
  for (int i = 0; i < 24; i++) cur[i] = o[i];
  return bad;
}

// A packed 90-byte node into an LDS record slot (the 6 bytes after it zero), by the first 48 threads
__device__ __forceinline__ void node_to_slot(uint4* slot, const uint8_t* base, uint32_t idx) {
  const uint16_t* src = reinterpret_cast<const uint16_t*>(base + (size_t)idx * CDA_NODE_SIZE);
  if (threadIdx.x < CDA_REC_BYTES / 2)
    reinterpret_cast<uint16_t*>(slot)[threadIdx.x] = threadIdx.x < CDA_NODE_SIZE / 2 ? src[threadIdx.x] : (uint16_t)0;
}

// nlev levels of the rule on the records in `recs` by the whole workgroup: the node with index x at level j of this
// array sits at slot (x - (base >> j)) << j (base: the index of slot 0 at level 0, a multiple of 2^nlev).  The walk's
// span must lie inside the array.  Uniform over the workgroup (every thread holds the same walk).
__device__ __forceinline__ void fold_span(uint4* recs, uint32_t base, int nlev, VerifyWalk& w, const VerifyArgs& a,
                                          const cda_nmt_proof_desc& d, int* bad) {
  for (int j = 0; j < nlev; j++) {
    int left, right;
    w.step(left, right);
    const uint32_t b = base >> j;
    if (left >= 0) node_to_slot(recs + (size_t)((w.lo - b) << j) * 6, a.nodes, d.node_off + (uint32_t)left);
    if (right >= 0) node_to_slot(recs + (size_t)((w.hi - 1 - b) << j) * 6, a.nodes, d.node_off + (uint32_t)right);
    __syncthreads();
    const uint32_t pairs = (w.hi - w.lo) >> 1;  // an odd last node keeps its slot: it goes up unchanged
    for (uint32_t t = threadIdx.x; t < pairs; t += blockDim.x) {
      uint4* pl = recs + (size_t)((w.lo + 2 * t - b) << j) * 6;
      const uint4* pr = recs + (size_t)((w.lo + 2 * t + 1 - b) << j) * 6;
      uint32_t L[16], R[16];
      load16(pl, L);
      load16(pr, R);
      if (siblings_out_of_order(L, R)) *bad = 1;
      hash_node_mem(pl, pr, pl);
    }
    __syncthreads();
    w.up();
  }
}

constexpr int kVerifyChunkLog2 = 9, kVerifyChunk = 1 << kVerifyChunkLog2;
constexpr int kVerifyTops = (int)(kVerifyMaxEnd >> kVerifyChunkLog2);
// w.levels levels of the rule over the span [w.lo, w.hi) of some level of a tree, whose records fill(idx, slot) puts
// into an LDS slot (the thread that is handed position idx).  Returns where the span's top lies.  Shared by the
// range proofs (the bottom level is the leaves, hashed here) and the commitment proofs' rows (it is level log2 W,
// given as subtree roots).
template <class Fill>
__device__ __forceinline__ uint4* fold_chunks(const VerifyArgs& a, const cda_nmt_proof_desc& d, VerifyWalk& w,
                                              uint4* recs, uint4* tops, int& bad, Fill fill) {
  const uint32_t start = w.lo, end = w.hi;
  const int chunk_levels = w.levels < kVerifyChunkLog2 ? w.levels : kVerifyChunkLog2;
  const uint32_t c0 = start >> kVerifyChunkLog2, c1 = (end - 1) >> kVerifyChunkLog2;
  for (uint32_t c = c0; c <= c1; c++) {
    const uint32_t cb = c << kVerifyChunkLog2;
    const uint32_t clo = max(start, cb), chi = min(end, cb + kVerifyChunk);
    __syncthreads();  // the previous chunk's root has been read
    const uint32_t idx = cb + threadIdx.x;
    if (idx >= clo && idx < chi) fill(idx, recs + (size_t)threadIdx.x * 6);
    __syncthreads();
    // the chunk's part of the walk: only the first chunk's span starts off a chunk boundary (left hull nodes) and only
    // the last one's ends off one (nodes behind the span): every other edge stays even through these levels
    VerifyWalk cw = w;
    cw.lo = clo;
    cw.hi = chi;
    if (c != c1) cw.nnodes = cw.rp;
    fold_span(recs, cb, chunk_levels, cw, a, d, &bad);
    w.lp = cw.lp;
    w.rp = cw.rp;
    if (w.levels > kVerifyChunkLog2 && threadIdx.x < 6) tops[(size_t)c * 6 + threadIdx.x] = recs[threadIdx.x];
  }
  uint4* top = recs;
  if (w.levels > kVerifyChunkLog2) {
    __syncthreads();
    w.lo = c0;
    w.hi = c1 + 1;
    fold_span(tops, 0, w.levels - kVerifyChunkLog2, w, a, d, &bad);
    top = tops;
  }
  return top;
}

constexpr uint32_t kVerifyGrid = 1024;  // workgroups of the range kernel: two rounds of the 512 resident ones

}  // namespace cda
