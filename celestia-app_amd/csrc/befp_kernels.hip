// befp_kernels.hip — the three kernels that tie cda_befp_validate's legs together.  None hashes: they
// check integers, move bytes and compare.  Between them run launch_nmt_verify, launch_rs_decode, the encoder and
// launch_axis_roots as they stand.
//   prep     a workgroup per proof: B1 and B2 (befp_rule.h), then per entry the NMT leg's descriptor and namespace, per
//            proof the decoder's present mask, codeword offset and stride and the tree's axis index;
//   gather   32 lanes per entry: the share into its slot of the proof's axis buffer, 16 bytes per lane;
//   combine  a lane per proof: the prep verdict, the entries' verdicts, the tree's status word and root.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "befp.h"
#include "befp_rule.h"
#include "cda_internal.h"

namespace cda {

namespace {
__device__ __forceinline__ BefpTotals totals_of(const BefpArgs& a) {
  return BefpTotals{a.k, a.nentries, a.nnodes_total, a.nroots};
}
}  // namespace

// The entries of a proof are checked by the workgroup's lanes side by side (entry j against entry j - 1 for the
// order); the verdict is the same in every lane before anything is derived from an entry.  A rejected proof gets
// empty descriptors (the NMT kernels reject them without a read), an all-ones mask (the decoder writes nothing) and
// axis index 0.
__global__ void __launch_bounds__(256) befp_prep_kernel(BefpArgs a) {
  const uint32_t p = blockIdx.x, w = 2 * a.k;
  const BefpTotals t = totals_of(a);
  const cda_befp_desc d = a.descs[p];
  const bool head = befp_head_ok(d, t);
  int bad = 0;
  if (head)
    for (uint32_t j = threadIdx.x; j < d.nshares; j += blockDim.x) bad |= !befp_entry_ok(d, a.entries, j, t);
  bad = __syncthreads_or(bad);
  const int pre = befp_pre_verdict(d, head, !bad, t);
  const bool live = pre == kBefpPending;
  const size_t slot0 = (size_t)p * w;
  for (uint32_t j = threadIdx.x; j < w; j += blockDim.x) {
    a.mask[slot0 + j] = live ? 0 : 1;
    if (!live || j >= d.nshares) a.nmt_descs[slot0 + j] = befp_empty_desc();
  }
  __syncthreads();
  if (live)
    for (uint32_t j = threadIdx.x; j < d.nshares; j += blockDim.x) {
      const uint32_t e = d.entry_off + j;
      const cda_befp_entry en = a.entries[e];
      a.nmt_descs[slot0 + j] = befp_nmt_desc(d, en, e, a.k);
      befp_namespace(a.k, d.index, en.pos, a.shares + (size_t)e * CDA_SHARE,
                     a.nmt_ns + (slot0 + j) * CDA_NAMESPACE_SIZE);
      a.mask[slot0 + en.pos] = 1;
    }
  if (threadIdx.x == 0) {
    a.pre[p] = pre;
    a.cw_off[p] = (long long)(slot0 * CDA_SHARE);
    a.cw_stride[p] = CDA_SHARE;
    a.axis_idx[p] = live ? d.index : 0;
  }
}

// B1 excluded duplicate positions, so no two groups write one slot.  Entries of a rejected proof are not read.
__global__ void __launch_bounds__(256) befp_gather_kernel(BefpArgs a) {
  const uint32_t w = 2 * a.k, lane = threadIdx.x & 31;
  const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 5;
  if (g >= (size_t)a.nproofs * w) return;
  const uint32_t p = (uint32_t)(g / w), j = (uint32_t)(g % w);
  if (a.pre[p] != kBefpPending) return;
  const cda_befp_desc d = a.descs[p];
  if (j >= d.nshares) return;
  const uint32_t e = d.entry_off + j, pos = a.entries[e].pos;
  const uint4* from = reinterpret_cast<const uint4*>(a.shares) + (size_t)e * (CDA_SHARE / 16);
  uint4* to = reinterpret_cast<uint4*>(a.axes) + ((size_t)p * w + pos) * (CDA_SHARE / 16);
  to[lane] = from[lane];
}

// The NMT leg left 1 for every entry that verifies and 0 for the empty descriptors of the unused slots, so all of a
// proof's entries verify iff its slots' bytes add up to nshares.
__global__ void __launch_bounds__(256) befp_combine_kernel(BefpArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nproofs) return;
  const int pre = a.pre[p];
  if (pre != kBefpPending) {
    a.verdicts[p] = pre;
    return;
  }
  const uint32_t w = 2 * a.k;
  const cda_befp_desc d = a.descs[p];
  const uint8_t* ok = a.nmt_ok + (size_t)p * w;
  uint32_t good = 0;
  if (w >= 4) {  // slots of a proof start on a 4-byte boundary
    const uint32_t* ok4 = reinterpret_cast<const uint32_t*>(ok);
#pragma unroll 8
    for (uint32_t i = 0; i < w / 4; i++) good += __popc(ok4[i] & 0x01010101u);
  } else {
    for (uint32_t i = 0; i < w; i++) good += ok[i] & 1;
  }
  if (good != d.nshares) {
    a.verdicts[p] = CDA_BEFP_BAD_SHARE;
    return;
  }
  // B4: the tree could not be built (push order), or its root (the record's min ‖ max ‖ digest) is not the committed one
  const uint8_t* rec = a.recs + (size_t)p * CDA_REC_BYTES;
  const uint8_t* want = a.roots + ((size_t)d.root_off + (d.axis == CDA_AXIS_ROW ? 0 : w) + d.index) * CDA_NODE_SIZE;
  uint32_t diff = a.status[p] != ~0ull;
  for (uint32_t i = 0; i < CDA_NODE_SIZE; i++) diff |= (uint32_t)(rec[i] ^ want[i]);
  a.verdicts[p] = diff ? CDA_BEFP_FRAUD : CDA_BEFP_NO_FRAUD;
}

int launch_befp_prep(const BefpArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(befp_prep_kernel, dim3(a.nproofs), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_befp_gather(const BefpArgs& a, hipStream_t s) {
  const size_t groups = (size_t)a.nproofs * 2 * a.k;
  hipLaunchKernelGGL(befp_gather_kernel, dim3((unsigned)((groups * 32 + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_befp_combine(const BefpArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(befp_combine_kernel, dim3((a.nproofs + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cda
