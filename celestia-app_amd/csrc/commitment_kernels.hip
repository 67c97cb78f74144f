// commitment_kernels.hip — blob commitment proofs on a retained square (gfx950): cda_square_commitment_proofs and
// cda_commitment_proofs_verify[_device], ADR-011's blob inclusion proof, rules C0-C8 of DESIGN §23.  The row-proof leg
// is share_proof_kernels.hip's launch_row_proof_verify; the chain and the workgroup fold are proof_dev.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cda_internal.h"
#include "commitment.h"
#include "commitment_rule.h"
#include "nmt_dev.h"
#include "nmt_verify_rule.h"
#include "proof_dev.h"
#include "sha256_dev.h"
#include "share_proof.h"

namespace cda {

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
      if (launch_row_proof_verify(rp, s)) return -1;
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
