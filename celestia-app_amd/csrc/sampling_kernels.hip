// sampling_kernels.hip — sample proofs on a retained square (gfx950): the gather of wrapper.ProveRange proofs
// (cda_square_prove) and batched nmt.Proof.VerifyInclusion (cda_nmt_verify, cda_nmt_verify_device); share proofs to the
// data root (cda_square_share_proofs) and batched ShareProof.Validate (cda_share_proofs_validate) after them; namespace
// data with completeness proofs (cda_square_prove_namespace, cda_nmt_verify_namespace: nmt ProveNamespace /
// VerifyNamespace); blob commitment proofs (cda_square_commitment_proofs, cda_commitment_proofs_verify: ADR-011's blob
// inclusion proof, rules C0-C8 of DESIGN §23) at the end.
//
// Reference semantics (celestia-app @ 2025-02-13, nmt v0.22):
//   ProveRange(start, end) of an erasured tree (pkg/wrapper/nmt_wrapper.go:127-130 -> nmt buildRangeProof): the roots
//   of the maximal subtrees outside [start, end), left to right.  On the perfect tree of 2k leaves these are, left of
//   the range, one node per set bit of start (highest bit first) and, right of it, one per set bit of 2k - end
//   (lowest bit first): no walk of the tree, a node's height and position follow from the bit.
//   VerifyInclusion (nmt proof.go, as ShareProof.VerifyProof calls it, pkg/proof/share_proof.go:53-82): leaf =
//   nid ‖ nid ‖ SHA256(0x00 ‖ nid ‖ share) with the SUPPLIED namespace; inner nodes as hasher.go:271-310 with
//   IgnoreMaxNamespace; siblings with left.max > right.min are rejected (ValidateSiblings); the schedule of nodes is
//   nmt_verify_rule.h.
//
// Design: a proof of one cell (the sampling case: 9 leaf + 3 log2(2k) node compressions) is a chain, so one lane runs
// one proof with the running node in registers and every lane of a wave is a different proof: leaf hashes and node
// hashes are lane-parallel across the batch, there is no workspace and nothing to synchronise.  A proof of a longer
// range is a tree, so one workgroup runs it: its leaves 512 at a time, a lane each, into LDS; nine levels folded in
// place there (nmt_dev.h's LDS layout: node i of level l at slot i << l), the proof's own nodes put at the span's
// ends as the rule says; the 512-leaf subtree roots (at most 128: no axis is wider than 65,536) collect in a second
// LDS array that the same fold finishes.  Neither kernel has a private segment or a global scratch buffer, so the
// device form needs no context workspace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cda_internal.h"
#include "commitment_rule.h"
#include "merkle_walk_rule.h"
#include "nmt_dev.h"
#include "nmt_namespace_rule.h"
#include "nmt_verify_rule.h"
#include "sampling.h"
#include "sha256_dev.h"

namespace cda {

// ---------------------------------------------------------------------------
// cda_square_prove
// ---------------------------------------------------------------------------
// share_off[q] = cells of the queries before q (where query q's cells go in the packed output): one workgroup, each
// thread a run of consecutive queries, the run sums scanned in LDS.
__global__ void __launch_bounds__(1024) square_share_offsets_kernel(const cda_range_query* __restrict__ q, uint32_t nq,
                                                                    uint32_t* __restrict__ share_off) {
  __shared__ uint32_t part[1024];
  const uint32_t t = threadIdx.x, run = (nq + 1023) / 1024;
  const uint32_t lo = min(nq, t * run), hi = min(nq, lo + run);
  uint32_t sum = 0;
#pragma unroll 8  // independent loads: several in flight (one after the other the two passes took 125 us at 65,536 queries)
  for (uint32_t i = lo; i < hi; i++) sum += q[i].end - q[i].start;
  part[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint32_t v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t off = part[t] - sum;
#pragma unroll 8
  for (uint32_t i = lo; i < hi; i++) {
    share_off[i] = off;
    off += q[i].end - q[i].start;
  }
}

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

// One query per 32 lanes: the proof's nodes (gather_range_proof), then the range's cells 16 bytes per lane.  The host
// has checked every query against the square.
__global__ void __launch_bounds__(256) square_prove_kernel(SquareView v, const cda_range_query* __restrict__ q,
                                                           uint32_t nq, uint32_t max_nodes, int32_t* __restrict__ counts,
                                                           uint8_t* __restrict__ nodes_out,
                                                           const uint32_t* __restrict__ share_off,
                                                           uint8_t* __restrict__ shares_out) {
  const uint32_t g = (blockIdx.x * blockDim.x + threadIdx.x) >> 5, lane = threadIdx.x & 31;
  if (g >= nq) return;
  const cda_range_query qq = q[g];
  const uint32_t w = 1u << v.log2w, s = qq.start;
  const uint32_t cnt = gather_range_proof(v, qq.axis, qq.index, s, qq.end, lane, max_nodes,
                                          nodes_out + (size_t)g * max_nodes * CDA_NODE_SIZE);
  if (lane == 0) counts[g] = (int32_t)cnt;
  if (!shares_out) return;
  const uint4* eds = reinterpret_cast<const uint4*>(v.eds);
  uint4* out = reinterpret_cast<uint4*>(shares_out) + (size_t)share_off[g] * (CDA_SHARE / 16);
  for (uint32_t c = 0; c < qq.end - s; c++) {
    const size_t cell = qq.axis ? (size_t)(s + c) * w + qq.index : (size_t)qq.index * w + s + c;
    out[(size_t)c * (CDA_SHARE / 16) + lane] = eds[cell * (CDA_SHARE / 16) + lane];
  }
}

int launch_square_prove(const SquareView& v, const cda_range_query* d_q, uint32_t nq, uint32_t max_nodes,
                        int32_t* d_counts, uint8_t* d_nodes, uint32_t* d_share_off, uint8_t* d_shares, hipStream_t s) {
  if (nq == 0) return 0;
  if (d_shares) hipLaunchKernelGGL(square_share_offsets_kernel, dim3(1), dim3(1024), 0, s, d_q, nq, d_share_off);
  const uint32_t grid = (uint32_t)(((size_t)nq * 32 + 255) / 256);
  hipLaunchKernelGGL(square_prove_kernel, dim3(grid), dim3(256), 0, s, v, d_q, nq, max_nodes, d_counts, d_nodes,
                     d_share_off, d_shares);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------
// cda_square_share_proofs
// ---------------------------------------------------------------------------
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

// One row record per 32 lanes: the group finds its query (the last q with row_off[q] <= record), takes the row and its
// leaf range from the query (pkg/proof/proof.go:61-64, :129-139), gathers the NMT proof with the routine
// square_prove_kernel uses, copies the row root (the one node of level log2(2k)), its leaf hash and aunt h = node
// (row >> h) ^ 1 of level h of the retained data-root tree, and the row's cells 16 bytes per lane.  The host has
// checked every query against the square.
__global__ void __launch_bounds__(256) square_share_proofs_kernel(SquareView v, const cda_share_range* __restrict__ q,
                                                                  uint32_t nq, const uint32_t* __restrict__ row_off,
                                                                  const uint32_t* __restrict__ share_off,
                                                                  uint32_t nrows, uint32_t max_nodes,
                                                                  ShareProofsOut out) {
  const uint32_t r = (blockIdx.x * blockDim.x + threadIdx.x) >> 5, lane = threadIdx.x & 31;
  if (r >= nrows) return;
  uint32_t lo = 0, hi = nq;  // row_off[lo] <= r < row_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (row_off[mid] <= r) lo = mid;
    else hi = mid;
  }
  const cda_share_range qq = q[lo];
  const uint32_t w = 1u << v.log2w, k = w >> 1, naunts = (uint32_t)v.log2w + 1;
  const uint32_t row = qq.start / k + (r - row_off[lo]), end_row = (qq.end - 1) / k;
  const uint32_t s = row * k < qq.start ? qq.start - row * k : 0, e = row == end_row ? (qq.end - 1) % k + 1 : k;
  const uint32_t cnt = gather_range_proof(v, CDA_AXIS_ROW, row, s, e, lane, max_nodes,
                                          out.nodes + (size_t)r * max_nodes * CDA_NODE_SIZE);
  if (lane == 0) {
    cda_share_row rec;
    rec.nmt_start = (int32_t)s;
    rec.nmt_end = (int32_t)e;
    rec.node_off = r * max_nodes;
    rec.nnodes = cnt;
    rec.total = 2 * (int64_t)w;
    rec.index = row;
    rec.aunt_off = r * naunts;
    rec.naunts = naunts;
    rec.row = row;
    rec.pad_ = 0;
    out.rows[r] = rec;
  }
  copy_row_root_proof(v, row, r, lane, out.row_roots, out.leaf_hashes, out.aunts);
  if (!out.shares) return;
  const uint4* cells = reinterpret_cast<const uint4*>(v.eds) + ((size_t)row * w + s) * (CDA_SHARE / 16);
  uint4* to = reinterpret_cast<uint4*>(out.shares) +
              ((size_t)share_off[lo] + ((size_t)row * k + s - qq.start)) * (CDA_SHARE / 16);
  const uint32_t n16 = (e - s) * (CDA_SHARE / 16);  // the row's cells are contiguous in the EDS and in the output
#pragma unroll 4
  for (uint32_t i = lane; i < n16; i += 32) to[i] = cells[i];
}

int launch_square_share_proofs(const SquareView& v, const cda_share_range* d_q, uint32_t nq, const uint32_t* d_row_off,
                               const uint32_t* d_share_off, uint32_t nrows, uint32_t max_nodes,
                               const ShareProofsOut& out, hipStream_t s) {
  if (nq == 0 || nrows == 0) return 0;
  const uint32_t grid = (uint32_t)(((size_t)nrows * 32 + 255) / 256);
  hipLaunchKernelGGL(square_share_proofs_kernel, dim3(grid), dim3(256), 0, s, v, d_q, nq, d_row_off, d_share_off, nrows,
                     max_nodes, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------
// cda_nmt_verify
// ---------------------------------------------------------------------------
// A descriptor the kernels may read through: inside every total, a range, no wider than the widest axis
__device__ __forceinline__ bool desc_valid(const cda_nmt_proof_desc& d, const VerifyArgs& a) {
  return d.start < d.end && d.end <= kVerifyMaxEnd && d.root < a.nroots &&
         (unsigned long long)d.node_off + d.nnodes <= a.nnodes_total &&
         (unsigned long long)d.leaf_off + (d.end - d.start) <= a.nleaves_total;
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

// VerifyInclusion's leaf record of the share at sh under the namespace at nsp.  The namespace is read twice, for the
// first block and again (through a pointer ordered after the hashing) for the record: held in registers across the
// nine compressions it would not fit beside them in 128 VGPRs, and held in SGPRs (one proof per workgroup) the
// message words made of it become scalar code that runs out of SGPRs.
__device__ __forceinline__ void verify_leaf_record(const uint8_t* nsp, const uint4* sh, uint32_t (&o)[24]) {
  uint32_t ns[8], A[16], st[8];
  load_ns(launder(nsp), ns);
  load16(sh, A);
  leaf_digest_state<false>(sh, A, false, ns, st);
  load_ns(launder_after(nsp, st[0]), ns);
  leaf_record_words(ns, st, o);
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

// Proofs of one leaf, a lane each.  The span of every level is one node: the rule's step gives either a node in
// front of it (the running node is the right child) or one behind it, or neither (it goes up unchanged); the nodes
// left after the subtree are all behind it.
// 4 waves per SIMD asked for explicitly, as for nmt_levels_kernel: the budget of the hash kernels.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) nmt_verify_cells_kernel(VerifyArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nproofs) return;
  uint32_t cur[24];
  {
    const cda_nmt_proof_desc d = a.descs[p];
    if (!desc_valid(d, a) || VerifyWalk::popcount(d.start) > d.nnodes) {
      a.ok[p] = 0;
      return;
    }
    if (d.end - d.start != 1) return;  // nmt_verify_ranges_kernel's
    verify_leaf_record(a.namespaces + (size_t)p * CDA_NAMESPACE_SIZE,
                       reinterpret_cast<const uint4*>(a.leaves + (size_t)d.leaf_off * CDA_SHARE), cur);
  }
  // the descriptor is read again and the walk is set up only now, for the same reason as the namespace
  // (the proof's index made opaque, so that it and not a pointer derived from it lives through the leaf)
  uint32_t q = p;
  asm volatile("" : "+v"(q) : "v"(cur[14]));
  const cda_nmt_proof_desc d = a.descs[q];
  VerifyWalk w;
  w.init(d.start, d.end, d.nnodes);
  bool bad = false;
#pragma unroll 1
  for (;;) {
    int left = -1, right = -1;
    if (w.levels > 0) {
      w.step(left, right);
      w.up();
      w.levels--;
      if (left < 0 && right < 0) continue;
    } else if (w.rp < w.nnodes) {
      right = (int)w.rp++;
    } else {
      break;
    }
    bad |= chain_node(cur, a.nodes, d.node_off + (uint32_t)(left >= 0 ? left : right), left >= 0);
  }
  uint32_t root[24];
  asm volatile("" : "+v"(q) : "v"(cur[14]));
  load_node_regs(a.roots, a.descs[q].root, root);
  a.ok[q] = (!bad && node_equal(cur, root)) ? 1 : 0;
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

// One proof of two or more leaves (a descriptor that passed desc_valid) by the whole workgroup (the header comment has
// the plan).  512 threads and 512-leaf chunks: recs = the current chunk's leaves and the levels above them, tops = the
// roots of the chunks' subtrees (indices 0..127 of level 9); 62 KiB of LDS per workgroup, two workgroups = 4 waves per
// SIMD.  Uniform over the workgroup.
__device__ __forceinline__ void verify_range_proof(const VerifyArgs& a, uint32_t p, uint4* recs, uint4* tops,
                                                   int& bad) {
  const cda_nmt_proof_desc d = a.descs[p];
  VerifyWalk w;
  if (!w.init(d.start, d.end, d.nnodes)) {
    if (threadIdx.x == 0) a.ok[p] = 0;
    return;
  }
  __syncthreads();  // the proof before this one is done with the LDS arrays
  if (threadIdx.x == 0) bad = 0;
  uint4* top = fold_chunks(a, d, w, recs, tops, bad, [&](uint32_t idx, uint4* slot) {
    const uint4* sh = reinterpret_cast<const uint4*>(a.leaves + ((size_t)d.leaf_off + (idx - d.start)) * CDA_SHARE);
    uint32_t o[24];
    verify_leaf_record(a.namespaces + (size_t)p * CDA_NAMESPACE_SIZE, sh, o);
    store_rec(slot, o);
  });
  // the nodes left over are right siblings up to the root: a chain, one after the other
  for (uint32_t i = w.rp; i < d.nnodes; i++) {
    node_to_slot(top + 6, a.nodes, d.node_off + i);
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t L[16], R[16];
      load16(top, L);
      load16(top + 6, R);
      if (siblings_out_of_order(L, R)) bad = 1;
      hash_node_mem(top, top + 6, top);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    uint32_t got[24], root[24];
    load_rec(top, got);
    load_node_regs(a.roots, d.root, root);
    a.ok[p] = (!bad && node_equal(got, root)) ? 1 : 0;
  }
}

// The proofs of two or more leaves of a batch.  Most batches have few or none (a sampler's proofs are of one cell), so
// the grid is a fixed number of workgroups and not one per proof (65,536 workgroups that only read a descriptor took
// 64 us, a third of the call): workgroup b looks at proofs b, b + G, b + 2G, ..., 512 of them at a time (a thread
// each), lists those that are its to verify and verifies them one after the other.  Neighbouring proofs land in
// different workgroups, so a run of long proofs in the batch spreads over the device.
__global__ void __launch_bounds__(kVerifyChunk) __attribute__((amdgpu_waves_per_eu(4)))
nmt_verify_ranges_kernel(VerifyArgs a) {
  __shared__ uint4 recs[kVerifyChunk * 6];
  __shared__ uint4 tops[kVerifyTops * 6];
  __shared__ uint32_t list[kVerifyChunk];
  __shared__ uint32_t nlist;
  __shared__ int bad;
  for (unsigned long long base = blockIdx.x; base < a.nproofs; base += (unsigned long long)gridDim.x * kVerifyChunk) {
    __syncthreads();
    if (threadIdx.x == 0) nlist = 0;
    __syncthreads();
    const unsigned long long p = base + (unsigned long long)gridDim.x * threadIdx.x;
    if (p < a.nproofs) {
      const cda_nmt_proof_desc d = a.descs[p];
      if (desc_valid(d, a) && d.end - d.start >= 2) list[atomicAdd(&nlist, 1u)] = (uint32_t)p;  // else the cells kernel's
    }
    __syncthreads();
    const uint32_t n = nlist;
    for (uint32_t i = 0; i < n; i++) verify_range_proof(a, list[i], recs, tops, bad);
  }
}

constexpr uint32_t kVerifyGrid = 1024;  // workgroups of the range kernel: two rounds of the 512 resident ones
int launch_nmt_verify(const VerifyArgs& a, bool ranges, hipStream_t s) {
  if (a.nproofs == 0) return 0;
  hipLaunchKernelGGL(nmt_verify_cells_kernel, dim3((a.nproofs + 255) / 256), dim3(256), 0, s, a);
  if (ranges)
    hipLaunchKernelGGL(nmt_verify_ranges_kernel, dim3(a.nproofs < kVerifyGrid ? a.nproofs : kVerifyGrid),
                       dim3(kVerifyChunk), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------
// cda_share_proofs_validate
// ---------------------------------------------------------------------------
// ShareProof.Validate (pkg/proof/share_proof.go:16-51) of a batch in three legs and a combine:
//   prep     a lane per proof: the descriptor against the totals, the counting checks in Validate's order, and for a
//            proof that passes them the NMT leg's descriptors (row record r verifies against row_roots[r], its leaves
//            follow those of the rows before it, its namespace is the proof's);
//   NMT      launch_nmt_verify over every row record (ShareProof.VerifyProof, :53-82);
//   rows     a lane per row record: merkle Proof.Verify of the row root in the proof's data root (row_proof.go:26-48);
//   combine  a lane per proof: Validate's precedence.
// Row records that two proofs claim make both proofs malformed (the legs' per-record results would depend on which
// proof wrote last): every proof of a batch owns its records.
__device__ __forceinline__ uint32_t proof_records(const cda_share_proof_desc& d) {
  return max(d.nshare_proofs, max(d.nrow_roots, d.nrow_proofs));
}

__global__ void __launch_bounds__(256) share_validate_prep_kernel(ValidateArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nproofs) return;
  const cda_share_proof_desc& d = a.descs[p];
  const uint32_t nrec = proof_records(d), r0 = d.row_off;
  if ((unsigned long long)r0 + nrec > a.nrows || (unsigned long long)d.leaf_off + d.nleaves > a.nleaves ||
      d.data_root >= a.nroots) {
    a.pre[p] = CDA_SP_MALFORMED;
    return;
  }
  for (uint32_t i = 0; i < nrec; i++) {
    atomicAdd(&a.claims[r0 + i], 1u);
    a.owner[r0 + i] = p;
  }
  int v = CDA_SP_VALID;
  if (d.nshare_proofs != d.nrow_roots) {
    v = CDA_SP_PROOF_COUNT;
  } else {
    long long in_proofs = 0;
    for (uint32_t i = 0; i < d.nshare_proofs; i++)
      in_proofs += (long long)a.rows[r0 + i].nmt_end - a.rows[r0 + i].nmt_start;
    if (in_proofs != (long long)d.nleaves) v = CDA_SP_DATA_COUNT;
    for (uint32_t i = 0; i < d.nshare_proofs && !v; i++) {
      const int32_t s = a.rows[r0 + i].nmt_start, e = a.rows[r0 + i].nmt_end;
      if (s < 0) v = CDA_SP_NEG_START;
      else if ((long long)e - s <= 0) v = CDA_SP_EMPTY_RANGE;
    }
    if (!v && (long long)d.end_row - (long long)d.start_row + 1 != (long long)d.nrow_roots) v = CDA_SP_ROW_COUNT;
    if (!v && d.nrow_proofs != d.nrow_roots) v = CDA_SP_ROW_PROOFS;
  }
  a.pre[p] = v;
  if (v) return;  // the NMT descriptors of its records stay empty: rejected without a read
  uint32_t leaf = d.leaf_off;  // every range is positive and they sum to nleaves: inside the proof's data
  for (uint32_t i = 0; i < nrec; i++) {
    const cda_share_row& row = a.rows[r0 + i];
    cda_nmt_proof_desc nd;
    nd.start = (uint32_t)row.nmt_start;
    nd.end = (uint32_t)row.nmt_end;
    nd.node_off = row.node_off;
    nd.nnodes = row.nnodes;
    nd.leaf_off = leaf;
    nd.root = r0 + i;
    a.nmt_descs[r0 + i] = nd;
    leaf += nd.end - nd.start;
    for (int b = 0; b < CDA_NAMESPACE_SIZE; b++) a.nmt_ns[(size_t)(r0 + i) * CDA_NAMESPACE_SIZE + b] = d.ns[b];
  }
}

// merkle Proof.Verify of row record r's root, a lane each: SHA256(0x00 ‖ rowRoot) (two blocks) against leaf_hash, then
// the aunts folded by merkle_walk_rule.h (two blocks each) against the data root of the proof that owns the record.
__global__ void __launch_bounds__(256) row_proof_verify_kernel(ValidateArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nrows) return;
  const uint32_t p = a.owner[r];
  if (p == ~0u) return;  // no proof of the batch holds this record
  const cda_share_row& rec = a.rows[r];
  const uint32_t naunts = rec.naunts, aunt_off = rec.aunt_off;
  MerkleWalk w;
  if (!w.init(rec.total, rec.index, naunts) || (unsigned long long)aunt_off + naunts > a.naunts) {
    a.row_ok[r] = 0;
    return;
  }
  uint32_t h[8], diff = 0;
  {
    uint32_t L[24];
    load_node_regs(a.row_roots, r, L);
    dah_leaf_digest(L, h);
    const uint32_t* lh = reinterpret_cast<const uint32_t*>(a.leaf_hashes) + (size_t)r * 8;
#pragma unroll
    for (int t = 0; t < 8; t++) diff |= h[t] ^ bswap(lh[t]);
  }
#pragma unroll 1
  for (int j = 0; j < w.depth; j++) {
    const uint32_t* au = reinterpret_cast<const uint32_t*>(a.aunts) + ((size_t)aunt_off + j) * 8;
    const bool left = w.aunt_on_left(j);
    uint32_t Ld[8], Rd[8], st[8], m[16];
#pragma unroll
    for (int t = 0; t < 8; t++) {
      const uint32_t x = bswap(au[t]);
      Ld[t] = left ? x : h[t];
      Rd[t] = left ? h[t] : x;
    }
    sha256_init(st);
    rfc_node_block<0>(Ld, Rd, m);
    sha256_compress(st, m);
    rfc_node_block<1>(Ld, Rd, m);
    sha256_compress(st, m);
#pragma unroll
    for (int t = 0; t < 8; t++) h[t] = st[t];
  }
  const uint32_t* want = reinterpret_cast<const uint32_t*>(a.data_roots) + (size_t)a.descs[p].data_root * 8;
#pragma unroll
  for (int t = 0; t < 8; t++) diff |= h[t] ^ bswap(want[t]);
  a.row_ok[r] = diff == 0 ? 1 : 0;
}

__global__ void __launch_bounds__(256) share_validate_combine_kernel(ValidateArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nproofs) return;
  int v = a.pre[p];
  if (v != CDA_SP_MALFORMED) {
    const cda_share_proof_desc& d = a.descs[p];
    const uint32_t nrec = proof_records(d), r0 = d.row_off;
    bool shared = false, rows_ok = true, nmt_ok = true;
    for (uint32_t i = 0; i < nrec; i++) {
      shared = shared || a.claims[r0 + i] != 1;
      rows_ok = rows_ok && a.row_ok[r0 + i];
      nmt_ok = nmt_ok && a.nmt_ok[r0 + i];
    }
    if (shared) v = CDA_SP_MALFORMED;
    else if (!v) v = !rows_ok ? CDA_SP_ROW_PROOF : (!nmt_ok ? CDA_SP_SHARE_PROOF : CDA_SP_VALID);
  }
  a.verdicts[p] = v;
}

int launch_share_proofs_validate(const ValidateArgs& a, hipStream_t s) {
  if (a.nproofs == 0) return 0;
  // everything zero (no claims, empty NMT descriptors, verdicts "fails") but the owners: none
  if (hipMemsetAsync(a.pre, 0, workspace_bytes(a, validate_workspace), s) != hipSuccess) return -1;
  if (a.nrows && hipMemsetAsync(a.owner, 0xFF, (size_t)a.nrows * 4, s) != hipSuccess) return -1;
  const dim3 pgrid((a.nproofs + 255) / 256), block(256);
  hipLaunchKernelGGL(share_validate_prep_kernel, pgrid, block, 0, s, a);
  if (a.nrows) {
    VerifyArgs n{};
    n.descs = a.nmt_descs;
    n.namespaces = a.nmt_ns;
    n.roots = a.row_roots;
    n.nodes = a.nodes;
    n.leaves = a.leaves;
    n.ok = a.nmt_ok;
    n.nproofs = a.nrows;
    n.nroots = a.nrows;
    n.nnodes_total = a.nnodes;
    n.nleaves_total = a.nleaves;
    if (launch_nmt_verify(n, true, s)) return -1;
    hipLaunchKernelGGL(row_proof_verify_kernel, dim3((a.nrows + 255) / 256), block, 0, s, a);
  }
  hipLaunchKernelGGL(share_validate_combine_kernel, pgrid, block, 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------
// cda_square_prove_namespace
// ---------------------------------------------------------------------------
// nmt ProveNamespace of one tree per 32 lanes (rules P1-P3).  The root record decides P1.  The bounds are
// counts, not a bisection: lane i compares the namespaces of leaves i, i + 32, ... with the query's (the first 32 bytes
// of a leaf record hold its 29; a column's leaves lie 2k records apart) and the group sums the counts -- the axis is
// sorted, so #(< ns) is the run's start and #(<= ns) its end; 2k = 1024 is 32 steps, every lane busy in all of them.
// Then the gather square_prove_kernel uses and, for an absence proof, the record of the first leaf above the
// namespace.  The host has checked every query's axis and index against the square.
__global__ void __launch_bounds__(256)
square_prove_namespace_kernel(SquareView v, const cda_namespace_query* __restrict__ q, uint32_t nq, uint32_t max_nodes,
                              cda_namespace_result* __restrict__ results, uint8_t* __restrict__ nodes_out,
                              uint8_t* __restrict__ leaf_hashes) {
  const uint32_t g = (blockIdx.x * blockDim.x + threadIdx.x) >> 5, lane = threadIdx.x & 31;
  if (g >= nq) return;
  const uint32_t axis = q[g].axis, index = q[g].index, w = 1u << v.log2w;
  uint32_t nid[8];
  load_ns(q[g].ns, nid);
  bool outside;
  {
    uint32_t R[16], mx[8];  // min = bytes 0..28, max = bytes 29..57 of the root record
    load16(reinterpret_cast<const uint4*>(square_node(v, axis, index, v.log2w, 0)), R);
#pragma unroll
    for (int i = 0; i < 8; i++) mx[i] = le_window(R[7 + i], R[8 + i], 1);
    outside = ns_cmp(nid, R) < 0 || ns_cmp(nid, mx) > 0;
  }
  uint32_t below = 0, upto = 0;
  if (!outside) {
    for (uint32_t i = lane; i < w; i += 32) {
      const uint4* rec = reinterpret_cast<const uint4*>(square_node(v, axis, index, 0, i));
      const uint4 v0 = rec[0], v1 = rec[1];
      const uint32_t ln[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
      const int c = ns_cmp(ln, nid);
      below += c < 0;
      upto += c <= 0;
    }
  }
  for (int d = 16; d; d >>= 1) {
    below += __shfl_xor(below, d, 32);
    upto += __shfl_xor(upto, d, 32);
  }
  // inside the root's range a leaf with a namespace >= the query's exists (the root's max is a leaf's): below < 2k.
  // Held to here as well, so that no index derived from the data can leave the axis.
  if (below >= w) outside = true;
  uint32_t kind = CDA_NSP_EMPTY, start = 0, end = 0;
  if (!outside) {
    kind = below < upto ? CDA_NSP_INCLUSION : CDA_NSP_ABSENCE;
    start = below;
    end = below < upto ? upto : below + 1;
  }
  uint8_t* slots = nodes_out + (size_t)g * max_nodes * CDA_NODE_SIZE;
  uint32_t cnt = 0;
  if (kind != CDA_NSP_EMPTY) {
    cnt = gather_range_proof(v, axis, index, start, end, lane, max_nodes, slots);
  } else {
    uint16_t* z = reinterpret_cast<uint16_t*>(slots);
    for (uint32_t hw = lane; hw < max_nodes * (CDA_NODE_SIZE / 2); hw += 32) z[hw] = 0;
  }
  const uint16_t* leaf = kind == CDA_NSP_ABSENCE
                             ? reinterpret_cast<const uint16_t*>(square_node(v, axis, index, 0, start))
                             : nullptr;
  uint16_t* lh = reinterpret_cast<uint16_t*>(leaf_hashes + (size_t)g * CDA_NODE_SIZE);
  for (uint32_t hw = lane; hw < CDA_NODE_SIZE / 2; hw += 32) lh[hw] = leaf ? leaf[hw] : (uint16_t)0;
  if (lane == 0) {
    cda_namespace_result r;
    r.kind = kind;
    r.start = start;
    r.end = end;
    r.nnodes = cnt;
    r.share_off = 0;  // namespace_share_offsets_kernel's
    r.nshares = kind == CDA_NSP_INCLUSION ? end - start : 0;
    results[g] = r;
  }
}

// square_share_offsets_kernel's twin over the results' share counts, which only the device knows:
// results[q].share_off = the shares of the results before q, *total = the shares of all.
__global__ void __launch_bounds__(1024) namespace_share_offsets_kernel(cda_namespace_result* __restrict__ r,
                                                                       uint32_t nq,
                                                                       unsigned long long* __restrict__ total) {
  __shared__ uint32_t part[1024];
  const uint32_t t = threadIdx.x, run = (nq + 1023) / 1024;
  const uint32_t lo = min(nq, t * run), hi = min(nq, lo + run);
  uint32_t sum = 0;
#pragma unroll 8
  for (uint32_t i = lo; i < hi; i++) sum += r[i].nshares;
  part[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint32_t x = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += x;
    __syncthreads();
  }
  uint32_t off = part[t] - sum;
#pragma unroll 8
  for (uint32_t i = lo; i < hi; i++) {
    r[i].share_off = off;
    off += r[i].nshares;
  }
  if (t == 1023) *total = part[t];
}

// The cells of every INCLUSION result, one query per 32 lanes, 16 bytes per lane and cell
__global__ void __launch_bounds__(256) namespace_shares_kernel(SquareView v, const cda_namespace_query* __restrict__ q,
                                                               uint32_t nq, const cda_namespace_result* __restrict__ r,
                                                               uint8_t* __restrict__ shares_out) {
  const uint32_t g = (blockIdx.x * blockDim.x + threadIdx.x) >> 5, lane = threadIdx.x & 31;
  if (g >= nq) return;
  const cda_namespace_result rr = r[g];
  const uint32_t axis = q[g].axis, index = q[g].index, w = 1u << v.log2w;
  if (rr.nshares == 0 || rr.start + rr.nshares > w) return;
  const uint4* eds = reinterpret_cast<const uint4*>(v.eds);
  uint4* out = reinterpret_cast<uint4*>(shares_out) + (size_t)rr.share_off * (CDA_SHARE / 16);
  for (uint32_t c = 0; c < rr.nshares; c++) {
    const size_t cell = axis ? (size_t)(rr.start + c) * w + index : (size_t)index * w + rr.start + c;
    out[(size_t)c * (CDA_SHARE / 16) + lane] = eds[cell * (CDA_SHARE / 16) + lane];
  }
}

int launch_square_prove_namespace(const SquareView& v, const cda_namespace_query* d_q, uint32_t nq, uint32_t max_nodes,
                                  cda_namespace_result* d_results, uint8_t* d_nodes, uint8_t* d_leaf_hashes,
                                  unsigned long long* d_total, hipStream_t s) {
  if (nq == 0) return 0;
  const uint32_t grid = (uint32_t)(((size_t)nq * 32 + 255) / 256);
  hipLaunchKernelGGL(square_prove_namespace_kernel, dim3(grid), dim3(256), 0, s, v, d_q, nq, max_nodes, d_results,
                     d_nodes, d_leaf_hashes);
  hipLaunchKernelGGL(namespace_share_offsets_kernel, dim3(1), dim3(1024), 0, s, d_results, nq, d_total);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_namespace_shares(const SquareView& v, const cda_namespace_query* d_q, uint32_t nq,
                            const cda_namespace_result* d_results, uint8_t* d_shares, hipStream_t s) {
  if (nq == 0) return 0;
  const uint32_t grid = (uint32_t)(((size_t)nq * 32 + 255) / 256);
  hipLaunchKernelGGL(namespace_shares_kernel, dim3(grid), dim3(256), 0, s, v, d_q, nq, d_results, d_shares);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------
// cda_nmt_verify_namespace
// ---------------------------------------------------------------------------
// nmt Proof.VerifyNamespace of a batch in the shape of cda_share_proofs_validate:
//   prep     a lane per proof: the descriptor against the totals, then V1-V5 (nmt_namespace_rule.h: namespace compares
//            over the proof's nodes, no hash); an inclusion proof that passes gets a cda_nmt_proof_desc;
//   NMT      launch_nmt_verify over those descriptors (an empty descriptor is rejected without a read);
//   absence  a lane per absence proof: the chain of nmt_verify_cells_kernel, started from the supplied leaf node;
//   combine  a lane per proof.
__global__ void __launch_bounds__(256) ns_verify_prep_kernel(NsVerifyArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nproofs) return;
  const cda_nmt_ns_proof_desc d = a.descs[p];
  const bool has_leaf = d.leaf_hash != kNoLeafHash;
  cda_nmt_proof_desc nd;
  nd.start = nd.end = nd.node_off = nd.nnodes = nd.leaf_off = nd.root = 0;
  int pre = kNsReject;
  if (d.end <= kVerifyMaxEnd && d.root < a.nroots && (unsigned long long)d.node_off + d.nnodes <= a.nnodes_total &&
      (unsigned long long)d.leaf_off + d.nleaves <= a.nleaves_total && (!has_leaf || d.leaf_hash < a.nleaf_hashes)) {
    pre = ns_precheck(a.namespaces + (size_t)p * CDA_NAMESPACE_SIZE, d.start, d.end,
                      a.nodes + (size_t)d.node_off * CDA_NODE_SIZE, d.nnodes,
                      has_leaf ? a.leaf_hashes + (size_t)d.leaf_hash * CDA_NODE_SIZE : nullptr, d.nleaves,
                      a.roots + (size_t)d.root * CDA_NODE_SIZE);
    if (pre == kNsInclusion) {  // nleaves == end - start: its leaves lie inside the total
      nd.start = d.start;
      nd.end = d.end;
      nd.node_off = d.node_off;
      nd.nnodes = d.nnodes;
      nd.leaf_off = d.leaf_off;
      nd.root = d.root;
    }
  }
  a.nmt_descs[p] = nd;
  a.pre[p] = (uint8_t)pre;
}

// An absence proof is a proof of one leaf whose node is given: nmt_verify_cells_kernel's chain without the leaf hash.
// The prep kernel has checked the descriptor and that the proof has its left hull's nodes.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) ns_verify_absence_kernel(NsVerifyArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nproofs || a.pre[p] != kNsAbsence) return;
  const cda_nmt_ns_proof_desc d = a.descs[p];
  uint32_t cur[24];
  load_node_regs(a.leaf_hashes, d.leaf_hash, cur);
  VerifyWalk w;
  w.init(d.start, d.end, d.nnodes);
  bool bad = false;
#pragma unroll 1
  for (;;) {
    int left = -1, right = -1;
    if (w.levels > 0) {
      w.step(left, right);
      w.up();
      w.levels--;
      if (left < 0 && right < 0) continue;
    } else if (w.rp < w.nnodes) {
      right = (int)w.rp++;
    } else {
      break;
    }
    bad |= chain_node(cur, a.nodes, d.node_off + (uint32_t)(left >= 0 ? left : right), left >= 0);
  }
  uint32_t root[24];
  load_node_regs(a.roots, d.root, root);
  a.abs_ok[p] = (!bad && node_equal(cur, root)) ? 1 : 0;
}

__global__ void __launch_bounds__(256) ns_verify_combine_kernel(NsVerifyArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nproofs) return;
  const int pre = a.pre[p];
  uint8_t ok = 0;
  if (pre == kNsAcceptEmpty) ok = 1;
  else if (pre == kNsInclusion) ok = a.nmt_ok[p] ? 1 : 0;
  else if (pre == kNsAbsence) ok = a.abs_ok[p] ? 1 : 0;
  a.ok[p] = ok;
}

int launch_nmt_verify_namespace(const NsVerifyArgs& a, hipStream_t s) {
  if (a.nproofs == 0) return 0;
  const dim3 grid((a.nproofs + 255) / 256), block(256);
  hipLaunchKernelGGL(ns_verify_prep_kernel, grid, block, 0, s, a);
  VerifyArgs n{};
  n.descs = a.nmt_descs;
  n.namespaces = a.namespaces;
  n.roots = a.roots;
  n.nodes = a.nodes;
  n.leaves = a.leaves;
  n.ok = a.nmt_ok;
  n.nproofs = a.nproofs;
  n.nroots = a.nroots;
  n.nnodes_total = a.nnodes_total;
  n.nleaves_total = a.nleaves_total;
  if (launch_nmt_verify(n, true, s)) return -1;
  hipLaunchKernelGGL(ns_verify_absence_kernel, grid, block, 0, s, a);
  hipLaunchKernelGGL(ns_verify_combine_kernel, grid, block, 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------
// cda_square_commitment_proofs
// ---------------------------------------------------------------------------
// One row record per 32 lanes, as square_share_proofs_kernel: the group finds its query, the row and its leaf range,
// copies the range's subtree roots out of the retained levels (commitment_rule.h: the tile of size 2^h at c is node
// (h, c >> h) of the row tree), 2 bytes per lane per 90-byte slot, and then, unless only the commitments are wanted,
// the range proof's nodes, the row root, its leaf hash and aunts.  A blob's roots are contiguous: row i's begin after
// those of the first row (which ends at k whenever a row follows it) and of the i - 1 full rows between.  The host has
// checked every query against the square and the rule.
__global__ void __launch_bounds__(256)
square_commitment_proofs_kernel(SquareView v, const cda_blob_range* __restrict__ q, uint32_t nq, uint32_t threshold,
                                const uint32_t* __restrict__ row_off, const uint32_t* __restrict__ root_off,
                                uint32_t nrows, uint32_t max_nodes, CommitProofsOut out) {
  const uint32_t r = (blockIdx.x * blockDim.x + threadIdx.x) >> 5, lane = threadIdx.x & 31;
  if (r >= nrows) return;
  uint32_t lo = 0, hi = nq;  // row_off[lo] <= r < row_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (row_off[mid] <= r) lo = mid;
    else hi = mid;
  }
  const cda_blob_range qq = q[lo];
  const uint32_t w = 1u << v.log2w, k = w >> 1, naunts = (uint32_t)v.log2w + 1;
  const uint32_t W = sub_tree_width(qq.len, threshold);
  const uint32_t i = r - row_off[lo], row = qq.start / k + i, last = qq.start + qq.len - 1, s0 = qq.start % k;
  const uint32_t s = i ? 0 : s0, e = row == last / k ? last % k + 1 : k;
  const uint32_t base = i ? subtree_tile_count(s0, k, W) + (i - 1) * (k / W) : 0;
  const uint32_t nroots = subtree_tile_count(s, e, W), roff = root_off[lo] + base;
  for (uint32_t t = 0, c = s; t < nroots; t++) {
    const uint32_t z = subtree_tile(c, e, W);
    const int h = 31 - __clz(z);
    const uint16_t* from = reinterpret_cast<const uint16_t*>(square_node(v, CDA_AXIS_ROW, row, h, c >> h));
    uint16_t* to = reinterpret_cast<uint16_t*>(out.subtree_roots + (size_t)(roff + t) * CDA_NODE_SIZE);
    for (uint32_t hw = lane; hw < CDA_NODE_SIZE / 2; hw += 32) to[hw] = from[hw];
    c += z;
  }
  if (out.nodes)
    gather_range_proof(v, CDA_AXIS_ROW, row, s, e, lane, max_nodes, out.nodes + (size_t)r * max_nodes * CDA_NODE_SIZE);
  if (lane == 0) {
    cda_commitment_row rec;
    rec.nmt_start = (int32_t)s;
    rec.nmt_end = (int32_t)e;
    rec.node_off = r * max_nodes;
    rec.nnodes = range_proof_nodes(s, e, w);
    rec.root_off = roff;
    rec.nroots = nroots;
    rec.total = 2 * (int64_t)w;
    rec.index = row;
    rec.aunt_off = r * naunts;
    rec.naunts = naunts;
    rec.row = row;
    rec.pad_ = 0;
    out.rows[r] = rec;
    out.root_base[r] = base;
  }
  if (out.row_roots) copy_row_root_proof(v, row, r, lane, out.row_roots, out.leaf_hashes, out.aunts);
}

// merkle.HashFromByteSlices over the subtree roots of a set of row records, one workgroup per set, in
// merkle_sets_kernel's tree shape (levels pair (2i, 2i + 1) and promote an odd last node) for any count up to
// kCommitMaxRoots: 512 roots at a time are leaf-hashed into LDS and folded to one digest -- a chunk boundary is a
// multiple of 2^9, so nothing pairs across it below level 9 -- and the chunks' digests (at most 512) fold the same way.
// Root g of the set lies in the row record with root_base <= g (a search: the bases ascend) at root_off + g -
// root_base; a root that is not there (records that two proofs of a batch wrote) is never read and clears ok.
constexpr int kCommitChunkLog2 = 9, kCommitChunk = 1 << kCommitChunkLog2;
static_assert(kCommitMaxRoots == (uint32_t)kCommitChunk * kCommitChunk, "the chunks' digests fold as one chunk");
// cnt <= kCommitChunk digests at buf to one by the whole workgroup, a level at a time between buf and the half array
// behind it; returns where it lies
__device__ __forceinline__ uint32_t* rfc_fold(uint32_t* buf, int cnt) {
  uint32_t* src = buf;
  uint32_t* dst = buf + kCommitChunk * 8;
  for (; cnt > 1; cnt = (cnt + 1) >> 1) {
    rfc_level_wide(src, dst, cnt, nullptr);
    __syncthreads();
    uint32_t* tmp = src;
    src = dst;
    dst = tmp;
  }
  return src;
}
__global__ void __launch_bounds__(256)
commitment_roots_kernel(const CommitSet* __restrict__ sets, const cda_commitment_row* __restrict__ rows,
                        const uint32_t* __restrict__ root_base, const uint8_t* __restrict__ subtree_roots,
                        uint32_t nsubroots, uint32_t* __restrict__ out, uint32_t* __restrict__ ok_or_null) {
  __shared__ uint32_t dig[(kCommitChunk + kCommitChunk / 2) * 8];
  __shared__ uint32_t tops[(kCommitChunk + kCommitChunk / 2) * 8];
  __shared__ int missing;
  const CommitSet set = sets[blockIdx.x];
  if (!set.live || set.nroots == 0 || set.nroots > kCommitMaxRoots) return;
  if (threadIdx.x == 0) missing = 0;
  const uint32_t nchunks = (set.nroots + kCommitChunk - 1) >> kCommitChunkLog2;
  uint32_t* res = dig;
  for (uint32_t c = 0; c < nchunks; c++) {
    const int cnt = (int)min((uint32_t)kCommitChunk, set.nroots - (c << kCommitChunkLog2));
    __syncthreads();  // the chunk before has been read
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
      const uint32_t g = (c << kCommitChunkLog2) + (uint32_t)i;
      uint32_t lo = 0, hi = set.nrows;  // root_base[row0 + lo] <= g < root_base[row0 + hi]
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (root_base[set.row0 + mid] <= g) lo = mid;
        else hi = mid;
      }
      const cda_commitment_row& rec = rows[set.row0 + lo];
      const uint32_t rb = root_base[set.row0 + lo], j = g - rb;
      const bool there = rb <= g && j < rec.nroots && (unsigned long long)rec.root_off + j < nsubroots;
      if (!there) missing = 1;
      uint32_t L[24], st[8];
      load_node_regs(subtree_roots, there ? rec.root_off + j : 0u, L);  // root 0 exists: this set has roots
      dah_leaf_digest(L, st);
#pragma unroll
      for (int t = 0; t < 8; t++) dig[i * 8 + t] = st[t];
    }
    __syncthreads();
    res = rfc_fold(dig, cnt);
    if (nchunks > 1 && threadIdx.x < 8) tops[c * 8 + threadIdx.x] = res[threadIdx.x];
  }
  if (nchunks > 1) {
    __syncthreads();
    res = rfc_fold(tops, (int)nchunks);
  }
  __syncthreads();
  if (threadIdx.x < 8) out[(size_t)blockIdx.x * 8 + threadIdx.x] = bswap(res[threadIdx.x]);
  if (ok_or_null && threadIdx.x == 0) ok_or_null[blockIdx.x] = missing ? 0u : 1u;
}

int launch_square_commitment_proofs(const SquareView& v, const cda_blob_range* d_q, uint32_t nq, uint32_t threshold,
                                    const uint32_t* d_row_off, const uint32_t* d_root_off, const CommitSet* d_sets,
                                    uint32_t nrows, uint32_t nroots, uint32_t max_nodes, const CommitProofsOut& out,
                                    hipStream_t s) {
  if (nq == 0 || nrows == 0) return 0;
  const uint32_t grid = (uint32_t)(((size_t)nrows * 32 + 255) / 256);
  hipLaunchKernelGGL(square_commitment_proofs_kernel, dim3(grid), dim3(256), 0, s, v, d_q, nq, threshold, d_row_off,
                     d_root_off, nrows, max_nodes, out);
  hipLaunchKernelGGL(commitment_roots_kernel, dim3(nq), dim3(256), 0, s, d_sets, out.rows, out.root_base,
                     out.subtree_roots, nroots, reinterpret_cast<uint32_t*>(out.commitments), (uint32_t*)nullptr);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------
// cda_commitment_proofs_verify
// ---------------------------------------------------------------------------
// Rules C0-C8 (include/cda.h) of a batch in the shape of cda_share_proofs_validate:
//   prep     a lane per proof: C0, the claims on its row records, C1-C4 in order; a proof that passes them hands its
//            records to the legs (row_w = W, root_base) and states its subtree roots as one set;
//   ns       32 lanes per row record: C5, the namespaces of its subtree roots;
//   rows     row_proof_verify_kernel over the records as share rows: C6;
//   folds    C7, commitment_rule.h's walk: a lane per record whose span is one node at every level (a chain of at
//            most log2(2k) hashes: chain_node, as the absence proofs), a workgroup per record for the others (the tail
//            below log2 W as a chain in LDS, then fold_chunks over the level-log2 W nodes);
//   roots    commitment_roots_kernel over the sets: C8's digest;
//   combine  a lane per proof: the first rule that fails.
__device__ __forceinline__ bool commit_pow2(int64_t v) { return v > 0 && !(v & (v - 1)); }

__global__ void __launch_bounds__(256) commitment_prep_kernel(CommitVerifyArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nproofs) return;
  const cda_commitment_proof_desc& d = a.descs[p];
  const uint32_t r0 = d.row_off, n = d.nrows;
  bool inside = n && d.subtree_root_threshold && (unsigned long long)r0 + n <= a.nrows && d.data_root < a.nroots &&
                d.commitment < a.ncommitments;
  unsigned long long all_roots = 0;
  for (uint32_t i = 0; i < n && inside; i++) {
    const cda_commitment_row& row = a.rows[r0 + i];
    inside = (unsigned long long)row.node_off + row.nnodes <= a.nnodes &&
             (unsigned long long)row.root_off + row.nroots <= a.nsubroots &&
             (unsigned long long)row.aunt_off + row.naunts <= a.naunts;
    all_roots += row.nroots;
  }
  if (!inside || all_roots > kCommitMaxRoots) {
    a.pre[p] = CDA_CP_MALFORMED;
    return;
  }
  for (uint32_t i = 0; i < n; i++) {
    const cda_commitment_row& row = a.rows[r0 + i];
    atomicAdd(&a.claims[r0 + i], 1u);
    a.owner[r0 + i] = p;
    cda_share_row sr;
    sr.nmt_start = row.nmt_start;
    sr.nmt_end = row.nmt_end;
    sr.node_off = row.node_off;
    sr.nnodes = row.nnodes;
    sr.total = row.total;
    sr.index = row.index;
    sr.aunt_off = row.aunt_off;
    sr.naunts = row.naunts;
    sr.row = row.row;
    sr.pad_ = 0;
    a.sp_rows[r0 + i] = sr;
  }
  a.sp_descs[p].data_root = d.data_root;
  int v = CDA_CP_VALID;
  if ((long long)d.end_row - (long long)d.start_row + 1 != (long long)n) v = CDA_CP_ROW_COUNT;
  const int64_t total = a.rows[r0].total;
  uint32_t k = 0, W = 0;
  unsigned long long len = 0;
  if (!v) {
    if (total <= 0 || (total & 3) || !commit_pow2(total >> 2) || (total >> 2) > (int64_t)kCommitMaxK) v = CDA_CP_RANGE;
    else k = (uint32_t)(total >> 2);
  }
  for (uint32_t i = 0; i < n && !v; i++) {
    const cda_commitment_row& row = a.rows[r0 + i];
    const int32_t s = row.nmt_start, e = row.nmt_end;
    if (row.total != total || row.index != (int64_t)d.start_row + i || s < 0 || s >= e || (uint32_t)e > k ||
        (i && s) || (i + 1 < n && (uint32_t)e != k))
      v = CDA_CP_RANGE;
    len += (unsigned long long)((long long)e - s);
  }
  if (!v) {
    W = sub_tree_width(len, d.subtree_root_threshold);
    if (W > k || ((uint32_t)a.rows[r0].nmt_start & (W - 1))) v = CDA_CP_ALIGNMENT;
  }
  for (uint32_t i = 0; i < n && !v; i++) {
    const cda_commitment_row& row = a.rows[r0 + i];
    if (row.nroots != subtree_tile_count((uint32_t)row.nmt_start, (uint32_t)row.nmt_end, W)) v = CDA_CP_ROOT_COUNT;
  }
  a.pre[p] = v;
  if (v) return;  // its records stay with row_w = 0: the legs read nothing through them
  // Records that two proofs claim get both proofs' writes here, in either order.  That is safe and needs no order: each
  // writer bounded the record's offsets in C0 and its own W passed C4 on it, SubtreeWalk::init checks the counts again
  // under whichever W landed, commitment_roots_kernel reads no root that is not where root_base says, and combine makes
  // both proofs MALFORMED whatever the legs found.  (claims cannot gate the write: the other claim may come later.)
  uint32_t base = 0;
  for (uint32_t i = 0; i < n; i++) {
    a.root_base[r0 + i] = base;
    a.row_w[r0 + i] = W;
    base += a.rows[r0 + i].nroots;
  }
  a.sets[p] = CommitSet{r0, n, base, 1u};
}

// C5 of row record r by 32 lanes: min (bytes 0..28) and max (29..57) of every subtree root against the proof's namespace
__global__ void __launch_bounds__(256) commitment_ns_kernel(CommitVerifyArgs a) {
  const uint32_t r = (blockIdx.x * blockDim.x + threadIdx.x) >> 5, lane = threadIdx.x & 31;
  if (r >= a.nrows || a.row_w[r] == 0) return;
  const uint8_t* ns = a.descs[a.owner[r]].ns;
  const cda_commitment_row& row = a.rows[r];
  uint32_t bad = 0;
  for (uint32_t j = lane; j < row.nroots; j += 32) {
    const uint8_t* node = a.subtree_roots + ((size_t)row.root_off + j) * CDA_NODE_SIZE;
    for (int b = 0; b < CDA_NAMESPACE_SIZE; b++) bad |= (node[b] ^ ns[b]) | (node[CDA_NAMESPACE_SIZE + b] ^ ns[b]);
  }
  for (int d = 16; d; d >>= 1) bad |= __shfl_xor(bad, d, 32);
  if (lane == 0) a.ns_ok[r] = bad ? 0 : 1;
}

// The row records whose span is one node at every level, a lane each: the subtree roots and the proof's nodes join a
// running node one at a time.  The walk's state beside chain_node's 128 registers does not fit the 4 waves per SIMD of
// the other chains without spilling, so the compiler is left its choice (3 waves).
__global__ void __launch_bounds__(256) commitment_chain_kernel(CommitVerifyArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nrows) return;
  const uint32_t W = a.row_w[r];
  if (W == 0) return;
  const cda_commitment_row& rec = a.rows[r];
  SubtreeWalk sw;
  if (!sw.init((uint32_t)rec.nmt_start, (uint32_t)rec.nmt_end, W, (uint32_t)(rec.total >> 2), rec.nroots, rec.nnodes))
    return;                                     // fold_ok stays 0
  if (sw.nfull + (sw.rem ? 1u : 0u) != 1) return;  // commitment_rows_kernel's
  const uint32_t root_off = rec.root_off, node_off = rec.node_off;
  uint32_t cur[24];
  bool bad = false;
#pragma unroll 1
  for (int h = 0; h < sw.top; h++) {
    const bool was = sw.live;
    uint32_t first, count, at;
    sw.enter(h, first, count, at);
    if (count) {
      if (was) bad |= chain_node(cur, a.subtree_roots, root_off + first, true);  // a tile comes in front
      else load_node_regs(a.subtree_roots, root_off + first, cur);
    }
    if (!sw.live) continue;
    int left, right;
    sw.w.step(left, right);
    sw.w.up();
    if (left >= 0 || right >= 0)
      bad |= chain_node(cur, a.nodes, node_off + (uint32_t)(left >= 0 ? left : right), left >= 0);
  }
  uint32_t root[24];
  load_node_regs(a.row_roots, r, root);
  a.fold_ok[r] = (!bad && node_equal(cur, root)) ? 1 : 0;
}

// One row record of two or more level-log2 W nodes by the whole workgroup.  The tail below log2 W is a chain: the
// running node in one of two LDS slots, what joins it (a tile in front, a proof node behind) in the other, hashed by
// one thread.  At log2 W the W-sized roots stand in front of it and fold_chunks takes over: its records are the roots
// as they lie, the running node last.  Uniform over the workgroup.
__device__ __forceinline__ void verify_subtree_row(const CommitVerifyArgs& a, uint32_t r, uint4* recs, uint4* tops,
                                                   uint4* tail, int& bad) {
  const cda_commitment_row rec = a.rows[r];
  SubtreeWalk sw;
  if (!sw.init((uint32_t)rec.nmt_start, (uint32_t)rec.nmt_end, a.row_w[r], (uint32_t)(rec.total >> 2), rec.nroots,
               rec.nnodes))
    return;  // fold_ok stays 0
  VerifyArgs va{};
  va.nodes = a.nodes;
  cda_nmt_proof_desc d{};
  d.node_off = rec.node_off;
  __syncthreads();  // the record before this one is done with the LDS arrays
  if (threadIdx.x == 0) bad = 0;
  uint4* cur = tail;
  uint4* oth = tail + 6;
  for (int h = 0; h < sw.hw; h++) {
    const bool was = sw.live;
    uint32_t first, count, at;
    sw.enter(h, first, count, at);
    if (count) node_to_slot(was ? oth : cur, a.subtree_roots, rec.root_off + first);
    if (!sw.live) continue;
    int left, right;
    sw.w.step(left, right);
    sw.w.up();
    const bool front = (was && count) || left >= 0;
    if (left >= 0) node_to_slot(oth, a.nodes, rec.node_off + (uint32_t)left);
    if (right >= 0) node_to_slot(oth, a.nodes, rec.node_off + (uint32_t)right);
    __syncthreads();
    if (!front && right < 0) continue;  // nothing joined: the node goes up as it is
    uint4* pl = front ? oth : cur;
    uint4* pr = front ? cur : oth;
    if (threadIdx.x == 0) {
      uint32_t L[16], R[16];
      load16(pl, L);
      load16(pr, R);
      if (siblings_out_of_order(L, R)) bad = 1;
      hash_node_mem(pl, pr, pl);
    }
    __syncthreads();
    if (front) {
      oth = cur;
      cur = pl;
    }
  }
  const bool was = sw.live;
  uint32_t first, count, at;
  sw.enter(sw.hw, first, count, at);
  const uint32_t tailpos = was ? sw.w.hi - 1 : ~0u;
  sw.w.levels = sw.top - sw.hw;
  uint4* top = fold_chunks(va, d, sw.w, recs, tops, bad, [&](uint32_t idx, uint4* slot) {
    if (idx == tailpos) {
#pragma unroll
      for (int i = 0; i < 6; i++) slot[i] = cur[i];
    } else {
      uint32_t o[24];
      load_node_regs(a.subtree_roots, rec.root_off + (idx - at), o);
      store_rec(slot, o);
    }
  });
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t got[24], root[24];
    load_rec(top, got);
    load_node_regs(a.row_roots, r, root);
    a.fold_ok[r] = (!bad && node_equal(got, root)) ? 1 : 0;
  }
}

// The row records the chain kernel leaves, on nmt_verify_ranges_kernel's grid: workgroup b looks at records b, b + G,
// ..., 512 at a time, lists its own and verifies them one after the other.
__global__ void __launch_bounds__(kVerifyChunk) __attribute__((amdgpu_waves_per_eu(4)))
commitment_rows_kernel(CommitVerifyArgs a) {
  __shared__ uint4 recs[kVerifyChunk * 6];
  __shared__ uint4 tops[kVerifyTops * 6];
  __shared__ uint4 tail[2 * 6];
  __shared__ uint32_t list[kVerifyChunk];
  __shared__ uint32_t nlist;
  __shared__ int bad;
  for (unsigned long long base = blockIdx.x; base < a.nrows; base += (unsigned long long)gridDim.x * kVerifyChunk) {
    __syncthreads();
    if (threadIdx.x == 0) nlist = 0;
    __syncthreads();
    const unsigned long long r = base + (unsigned long long)gridDim.x * threadIdx.x;
    if (r < a.nrows && a.row_w[r]) {
      const cda_commitment_row& rec = a.rows[r];
      const uint32_t W = a.row_w[r], n = (uint32_t)(rec.nmt_end - rec.nmt_start);
      if (n / W + ((n & (W - 1)) ? 1u : 0u) > 1) list[atomicAdd(&nlist, 1u)] = (uint32_t)r;  // else the chain kernel's
    }
    __syncthreads();
    const uint32_t n = nlist;
    for (uint32_t i = 0; i < n; i++) verify_subtree_row(a, list[i], recs, tops, tail, bad);
  }
}

__global__ void __launch_bounds__(256) commitment_combine_kernel(CommitVerifyArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nproofs) return;
  int v = a.pre[p];
  if (v != CDA_CP_MALFORMED) {
    const cda_commitment_proof_desc& d = a.descs[p];
    bool shared = false, ns_ok = true, rows_ok = true, fold_ok = true;
    for (uint32_t i = 0; i < d.nrows; i++) {
      const uint32_t r = d.row_off + i;
      shared = shared || a.claims[r] != 1;
      ns_ok = ns_ok && a.ns_ok[r];
      rows_ok = rows_ok && a.row_ok[r];
      fold_ok = fold_ok && a.fold_ok[r];
    }
    if (shared) {
      v = CDA_CP_MALFORMED;
    } else if (!v) {
      const uint32_t* want = reinterpret_cast<const uint32_t*>(a.commitments) + (size_t)d.commitment * 8;
      uint32_t diff = a.got_ok[p] ? 0u : 1u;
      for (int t = 0; t < 8; t++) diff |= a.got[(size_t)p * 8 + t] ^ want[t];
      v = !ns_ok ? CDA_CP_NAMESPACE
                 : !rows_ok ? CDA_CP_ROW_PROOF : !fold_ok ? CDA_CP_SUBTREE_ROOTS : diff ? CDA_CP_COMMITMENT : CDA_CP_VALID;
    }
  }
  a.verdicts[p] = v;
}

// prof: the context, for a ProfScope around every leg (cda_profile_*: DESIGN §23's per-launch times)
int launch_commitment_proofs_verify(const CommitVerifyArgs& a, void* prof, hipStream_t s) {
  if (a.nproofs == 0) return 0;
  // everything zero (no claims, W = 0, sets not live, verdicts "fails") but the owners: none
  if (hipMemsetAsync(a.pre, 0, workspace_bytes(a, commit_verify_workspace), s) != hipSuccess) return -1;
  if (a.nrows && hipMemsetAsync(a.owner, 0xFF, (size_t)a.nrows * 4, s) != hipSuccess) return -1;
  const dim3 pgrid((a.nproofs + 255) / 256), rgrid((a.nrows + 255) / 256), block(256);
  {
    ProfScope ps(prof, "commitment_prep", s);
    hipLaunchKernelGGL(commitment_prep_kernel, pgrid, block, 0, s, a);
  }
  if (a.nrows) {
    {
      ProfScope ps(prof, "commitment_ns", s);
      hipLaunchKernelGGL(commitment_ns_kernel, dim3((uint32_t)(((size_t)a.nrows * 32 + 255) / 256)), block, 0, s, a);
    }
    ValidateArgs rp{};  // the records as share rows: the row-proof leg reads nothing else of a share proof
    rp.descs = a.sp_descs;
    rp.rows = a.sp_rows;
    rp.row_roots = a.row_roots;
    rp.leaf_hashes = a.leaf_hashes;
    rp.aunts = a.aunts;
    rp.data_roots = a.data_roots;
    rp.nproofs = a.nproofs;
    rp.nrows = a.nrows;
    rp.naunts = a.naunts;
    rp.nroots = a.nroots;
    rp.owner = a.owner;
    rp.row_ok = a.row_ok;
    {
      ProfScope ps(prof, "commitment_row_proofs", s);
      hipLaunchKernelGGL(row_proof_verify_kernel, rgrid, block, 0, s, rp);
    }
    {
      ProfScope ps(prof, "commitment_chain", s);
      hipLaunchKernelGGL(commitment_chain_kernel, rgrid, block, 0, s, a);
    }
    {
      ProfScope ps(prof, "commitment_rows", s);
      hipLaunchKernelGGL(commitment_rows_kernel, dim3(a.nrows < kVerifyGrid ? a.nrows : kVerifyGrid),
                         dim3(kVerifyChunk), 0, s, a);
    }
    {
      ProfScope ps(prof, "commitment_roots", s);
      hipLaunchKernelGGL(commitment_roots_kernel, dim3(a.nproofs), block, 0, s, a.sets, a.rows, a.root_base,
                         a.subtree_roots, a.nsubroots, a.got, a.got_ok);
    }
  }
  {
    ProfScope ps(prof, "commitment_combine", s);
    hipLaunchKernelGGL(commitment_combine_kernel, pgrid, block, 0, s, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cda
