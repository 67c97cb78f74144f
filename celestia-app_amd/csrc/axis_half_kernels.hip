// axis_half_kernels.hip — the kernels that tie the legs of cda_axis_halves_verify together, place verified halves
// into a square (cda_axis_halves_assemble_device, cda_square_rebuild_axes) and serve halves out of a retained one
// (cda_square_axis_halves); DESIGN §26.  None hashes: they check integers, move bytes and compare.  Between scatter
// and combine run launch_rs_decode, the encoder and launch_axis_roots as they stand.
//   prep     a lane per (half, slot): H0 (axis_half_rule.h), then the decoder's present mask and, per half, the
//            codeword offset and stride and the tree's axis index;
//   scatter  32 lanes per (half, slot), 16 bytes per lane: the half's share into its slot of the half's axis buffer,
//            zeros into the slots the codec is to fill and into every slot of a malformed half;
//   combine  a lane per half: the H0 verdict, then the tree's status word and root;
//   claim    a lane per half: axis_owner[axis] = min(axis_owner[axis], p) for the verified ones (preset to "none");
//   place    a workgroup per half, 32 lanes per cell: the cells the half owns from its axis buffer into the square
//            and present = 1; a cell the crossing axis's half owns is compared with THAT half's axis buffer (memory
//            no lane writes in this launch, not the square, which the owner may be writing), the OR of the
//            differences deciding CONFLICT;
//   gather   32 lanes per (query, cell): a cell of the retained square into its place of the packed half.
// Ownership is decided in a launch of its own, before any byte moves, and by the lowest index; the owner of a cell
// is the lower of its row's and its column's half, which needs no per-cell table.  The outcome is the same whatever
// order the hardware runs the lanes in.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "axis_half.h"
#include "axis_half_rule.h"
#include "cda_internal.h"

namespace cda {

namespace {
constexpr uint32_t kWords = CDA_SHARE / 16;  // 16-byte words of a share: one per lane of a 32-lane group

__device__ __forceinline__ AxisHalfShape shape_of(const AxisHalfArgs& a) {
  return AxisHalfShape{a.k, a.nroots, a.assembling};
}
__device__ __forceinline__ const uint4* axis_cell(const AxisHalfArgs& a, uint32_t p, uint32_t j) {
  return reinterpret_cast<const uint4*>(a.axes) + ((size_t)p * 2 * a.k + j) * kWords;
}
}  // namespace

__global__ void __launch_bounds__(256) axis_half_prep_kernel(AxisHalfArgs a) {
  const uint32_t w = 2 * a.k;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)a.nhalves * w) return;
  const uint32_t p = (uint32_t)(g / w), j = (uint32_t)(g % w);
  const cda_axis_half_desc d = a.descs[p];
  const bool ok = axis_half_well_formed(d, shape_of(a));
  a.mask[g] = axis_half_present(d, ok, a.k, j);
  if (j == 0) {
    a.cw_off[p] = (long long)((size_t)p * w * CDA_SHARE);
    a.cw_stride[p] = CDA_SHARE;
    a.axis_idx[p] = axis_half_tree_index(d, ok);
  }
}

// Every slot of every buffer is written here, so the encoder and the tree read nothing uninitialised.
__global__ void __launch_bounds__(256) axis_half_scatter_kernel(AxisHalfArgs a) {
  const uint32_t w = 2 * a.k, lane = threadIdx.x & 31;
  const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 5;
  if (g >= (size_t)a.nhalves * w) return;
  const uint32_t p = (uint32_t)(g / w), j = (uint32_t)(g % w);
  const cda_axis_half_desc d = a.descs[p];
  const int64_t from = axis_half_source(d, axis_half_well_formed(d, shape_of(a)), a.k, j);
  uint4 v = make_uint4(0, 0, 0, 0);
  if (from >= 0) v = reinterpret_cast<const uint4*>(a.shares)[((size_t)p * a.k + (size_t)from) * kWords + lane];
  reinterpret_cast<uint4*>(a.axes)[g * kWords + lane] = v;
}

// H2: the tree could not be built (push order), or its root (the record's min ‖ max ‖ digest) is not the committed one
__global__ void __launch_bounds__(256) axis_half_combine_kernel(AxisHalfArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nhalves) return;
  const cda_axis_half_desc d = a.descs[p];
  const bool ok = axis_half_well_formed(d, shape_of(a));
  uint32_t diff = 0;
  if (ok) {
    const uint8_t* rec = a.recs + (size_t)p * CDA_REC_BYTES;
    const uint8_t* want = a.roots + axis_half_root(d, a.k) * CDA_NODE_SIZE;
    for (uint32_t i = 0; i < CDA_NODE_SIZE; i++) diff |= (uint32_t)(rec[i] ^ want[i]);
  }
  a.statuses[p] = axis_half_verdict(ok, ok && a.status[p] == ~0ull, diff == 0);
}

__global__ void __launch_bounds__(256) axis_half_claim_kernel(AxisHalfArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nhalves || a.statuses[p] != CDA_HALF_PLACED) return;
  const cda_axis_half_desc d = a.descs[p];
  if (!axis_half_well_formed(d, shape_of(a))) return;  // not PLACED already; the key below is never out of the table
  atomicMin(a.axis_owner + axis_half_key(d, a.k), p);
}

// statuses[p] is read by the workgroup of half p alone, before its barrier, and written by it alone, after.
__global__ void __launch_bounds__(256) axis_half_place_kernel(AxisHalfArgs a) {
  const uint32_t p = blockIdx.x, w = 2 * a.k, lane = threadIdx.x & 31, group = threadIdx.x >> 5;
  if (a.statuses[p] != CDA_HALF_PLACED) return;  // the same in every lane of the workgroup
  const cda_axis_half_desc d = a.descs[p];
  if (!axis_half_well_formed(d, shape_of(a))) return;
  const uint32_t mine = a.axis_owner[axis_half_key(d, a.k)];
  int differs = 0;
  if (mine == p)
    for (uint32_t pos = group; pos < w; pos += blockDim.x >> 5) {
      const uint32_t cross = a.axis_owner[axis_half_cross_key(d, a.k, pos)];
      const uint4 v = axis_cell(a, p, pos)[lane];
      if (axis_half_owns(p, cross)) {
        const size_t cell = axis_half_cell(d, a.k, pos);
        reinterpret_cast<uint4*>(a.eds)[cell * kWords + lane] = v;
        if (lane == 0) a.present[cell] = 1;
      } else if (cross < a.nhalves) {  // always: a claimed axis names a half of this call
        // the shared cell lies at position d.index of the crossing axis
        const uint4 t = axis_cell(a, cross, d.index)[lane];
        differs |= ((v.x ^ t.x) | (v.y ^ t.y) | (v.z ^ t.z) | (v.w ^ t.w)) != 0;
      }
    }
  differs = __syncthreads_or(differs);
  if (threadIdx.x == 0) a.statuses[p] = axis_half_settle(p, mine, differs != 0);
}

// A row half is one contiguous run of k cells, a column half k cells a row apart.  A query outside the square (the
// host has refused those) moves nothing.
__global__ void __launch_bounds__(256) axis_half_gather_kernel(SquareView v, const cda_axis_half_desc* q, uint32_t nq,
                                                               uint8_t* out) {
  const uint32_t k = (1u << v.log2w) >> 1, lane = threadIdx.x & 31;
  const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 5;
  if (g >= (size_t)nq * k) return;
  const uint32_t i = (uint32_t)(g / k), j = (uint32_t)(g % k);
  const cda_axis_half_desc d = q[i];
  if (d.axis > 1 || d.index >= 2 * k || d.side > 1) return;
  const size_t cell = axis_half_cell(d, k, d.side * k + j);
  reinterpret_cast<uint4*>(out)[g * kWords + lane] = reinterpret_cast<const uint4*>(v.eds)[cell * kWords + lane];
}

namespace {
unsigned blocks_for(size_t lanes) { return (unsigned)((lanes + 255) / 256); }
int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }
}  // namespace

int launch_axis_half_prep(const AxisHalfArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(axis_half_prep_kernel, dim3(blocks_for((size_t)a.nhalves * 2 * a.k)), dim3(256), 0, s, a);
  return launched();
}

int launch_axis_half_scatter(const AxisHalfArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(axis_half_scatter_kernel, dim3(blocks_for((size_t)a.nhalves * 2 * a.k * 32)), dim3(256), 0, s, a);
  return launched();
}

int launch_axis_half_combine(const AxisHalfArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(axis_half_combine_kernel, dim3(blocks_for(a.nhalves)), dim3(256), 0, s, a);
  return launched();
}

int launch_axis_half_claim(const AxisHalfArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(axis_half_claim_kernel, dim3(blocks_for(a.nhalves)), dim3(256), 0, s, a);
  return launched();
}

int launch_axis_half_place(const AxisHalfArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(axis_half_place_kernel, dim3(a.nhalves), dim3(256), 0, s, a);
  return launched();
}

int launch_axis_half_gather(const SquareView& v, const cda_axis_half_desc* d_q, uint32_t nq, uint8_t* d_shares,
                            hipStream_t s) {
  const size_t k = ((size_t)1 << v.log2w) >> 1;
  hipLaunchKernelGGL(axis_half_gather_kernel, dim3(blocks_for((size_t)nq * k * 32)), dim3(256), 0, s, v, d_q, nq,
                     d_shares);
  return launched();
}

}  // namespace cda
