// sampling_kernels.hip — sample proofs on a retained square (gfx950): the gather of wrapper.ProveRange proofs
// (cda_square_prove) and batched nmt.Proof.VerifyInclusion (cda_nmt_verify, cda_nmt_verify_device).  The share proofs,
// the namespace proofs and the commitment proofs built on them are share_proof_kernels.hip, namespace_kernels.hip and
// commitment_kernels.hip; the device pieces they share with this file are proof_dev.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cda_internal.h"
#include "nmt_dev.h"
#include "nmt_verify_rule.h"
#include "proof_dev.h"
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
// cda_nmt_verify
// ---------------------------------------------------------------------------
// Reference semantics (celestia-app @ 2025-02-13, nmt v0.22):
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
//
// A descriptor the kernels may read through: inside every total, a range, no wider than the widest axis
__device__ __forceinline__ bool desc_valid(const cda_nmt_proof_desc& d, const VerifyArgs& a) {
  return d.start < d.end && d.end <= kVerifyMaxEnd && d.root < a.nroots &&
         (unsigned long long)d.node_off + d.nnodes <= a.nnodes_total &&
         (unsigned long long)d.leaf_off + (d.end - d.start) <= a.nleaves_total;
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

// One proof of two or more leaves (a descriptor that passed desc_valid) by the whole workgroup (the design note above
// has the plan).  512 threads and 512-leaf chunks: recs = the current chunk's leaves and the levels above them, tops =
// the roots of the chunks' subtrees (indices 0..127 of level 9); 62 KiB of LDS per workgroup, two workgroups = 4 waves
// per SIMD.  Uniform over the workgroup.
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

int launch_nmt_verify(const VerifyArgs& a, bool ranges, hipStream_t s) {
  if (a.nproofs == 0) return 0;
  hipLaunchKernelGGL(nmt_verify_cells_kernel, dim3((a.nproofs + 255) / 256), dim3(256), 0, s, a);
  if (ranges)
    hipLaunchKernelGGL(nmt_verify_ranges_kernel, dim3(a.nproofs < kVerifyGrid ? a.nproofs : kVerifyGrid),
                       dim3(kVerifyChunk), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cda
