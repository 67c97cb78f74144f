// share_proof_kernels.hip — share proofs to the data root on a retained square (gfx950): the gather of
// NewShareInclusionProof's parts (cda_square_share_proofs) and batched ShareProof.Validate (cda_share_proofs_validate,
// cda_share_proofs_validate_device).  The NMT leg is sampling_kernels.hip's launch_nmt_verify; the row-proof kernel
// here is also the commitment verifier's (launch_row_proof_verify).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cda_internal.h"
#include "merkle_walk_rule.h"
#include "nmt_dev.h"
#include "proof_dev.h"
#include "sha256_dev.h"
#include "share_proof.h"

namespace cda {

// ---------------------------------------------------------------------------
// cda_square_share_proofs
// ---------------------------------------------------------------------------
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

int launch_row_proof_verify(const ValidateArgs& a, hipStream_t s) {
  if (a.nrows == 0) return 0;
  hipLaunchKernelGGL(row_proof_verify_kernel, dim3((a.nrows + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
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
    if (launch_row_proof_verify(a, s)) return -1;
  }
  hipLaunchKernelGGL(share_validate_combine_kernel, pgrid, block, 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cda
