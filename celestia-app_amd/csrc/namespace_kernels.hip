// namespace_kernels.hip — namespace data with completeness proofs on a retained square (gfx950): nmt ProveNamespace
// of any row or column tree (cda_square_prove_namespace) and batched nmt Proof.VerifyNamespace
// (cda_nmt_verify_namespace, cda_nmt_verify_namespace_device).  The inclusion leg is sampling_kernels.hip's
// launch_nmt_verify.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cda_internal.h"
#include "namespace_proof.h"
#include "nmt_dev.h"
#include "nmt_namespace_rule.h"
#include "nmt_verify_rule.h"
#include "proof_dev.h"
#include "sha256_dev.h"

namespace cda {

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

}  // namespace cda
