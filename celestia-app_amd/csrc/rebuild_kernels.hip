// rebuild_kernels.hip — the three kernels that put verified samples into a square (cda_samples_assemble_device,
// cda_square_rebuild).  None hashes: they check integers, claim cells and move bytes.  Between prep and
// claim runs launch_nmt_verify as it stands.
//   prep     a lane per sample: the malformed check (sample_place_rule.h), then the NMT leg's descriptor and namespace;
//   claim    a lane per sample: owner[cell] = min(owner[cell], p) for the verified ones (owner preset to "none");
//   place    32 lanes per sample, 16 bytes per lane: the owner's share into its cell and present = 1; every other
//            verified sample of the cell is compared with the owner's SHARE (input memory no launch writes, not the
//            cell, which the owner's group may be writing in the same launch) and gets DUPLICATE or CONFLICT.
// Ownership is decided in a launch of its own, before any byte moves, and by the lowest index: the outcome is the same
// whatever order the hardware runs the lanes in.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cda_internal.h"
#include "rebuild.h"
#include "sample_place_rule.h"

namespace cda {

// A malformed sample gets an empty descriptor: the verifier rejects it without a read, so ok = 0 for it and neither
// claim nor place derives a cell from it.
__global__ void __launch_bounds__(256) sample_prep_kernel(AssembleArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nsamples) return;
  const cda_sample_desc d = a.descs[p];
  if (!sample_well_formed(d, a.k)) {
    a.nmt_descs[p] = befp_empty_desc();
    a.statuses[p] = CDA_SAMPLE_MALFORMED;
    return;
  }
  a.nmt_descs[p] = sample_nmt_desc(d, p, a.k);
  sample_namespace(d, a.k, a.shares + (size_t)p * CDA_SHARE, a.nmt_ns + (size_t)p * CDA_NAMESPACE_SIZE);
  a.statuses[p] = CDA_SAMPLE_REJECTED;  // until place says otherwise
}

__global__ void __launch_bounds__(256) sample_claim_kernel(AssembleArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nsamples || !a.ok[p]) return;
  const cda_sample_desc d = a.descs[p];
  if (!sample_well_formed(d, a.k)) return;  // ok = 0 already; the cell index below is never out of the square
  atomicMin(a.owner + sample_cell(d, a.k), p);
}

__global__ void __launch_bounds__(256) sample_place_kernel(AssembleArgs a) {
  const uint32_t lane = threadIdx.x & 31;
  const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 5;
  if (g >= a.nsamples) return;
  const uint32_t p = (uint32_t)g;
  if (!a.ok[p]) return;
  const cda_sample_desc d = a.descs[p];
  if (!sample_well_formed(d, a.k)) return;
  const size_t cell = sample_cell(d, a.k);
  const uint32_t o = a.owner[cell];
  const uint4* shares = reinterpret_cast<const uint4*>(a.shares);
  const uint4 mine = shares[(size_t)p * (CDA_SHARE / 16) + lane];
  if (o == p) {
    reinterpret_cast<uint4*>(a.eds)[cell * (CDA_SHARE / 16) + lane] = mine;
    if (lane == 0) {
      a.present[cell] = 1;
      a.statuses[p] = CDA_SAMPLE_PLACED;
    }
    return;
  }
  if (o >= a.nsamples) return;  // unreachable: a verified sample has claimed its cell
  const uint4 theirs = shares[(size_t)o * (CDA_SHARE / 16) + lane];
  const bool diff = (mine.x ^ theirs.x) | (mine.y ^ theirs.y) | (mine.z ^ theirs.z) | (mine.w ^ theirs.w);
  // the two groups of a wave may be in different branches: a group reads its own half of the ballot
  const unsigned long long any = __ballot(diff) >> (threadIdx.x & 32);
  if (lane == 0) a.statuses[p] = sample_settle(p, o, (uint32_t)any == 0);
}

int launch_sample_prep(const AssembleArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(sample_prep_kernel, dim3((a.nsamples + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_sample_claim(const AssembleArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(sample_claim_kernel, dim3((a.nsamples + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_sample_place(const AssembleArgs& a, hipStream_t s) {
  const size_t lanes = (size_t)a.nsamples * 32;
  hipLaunchKernelGGL(sample_place_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cda
