// sampling.h — what sampling.cpp (the C ABI of cda_square_* and cda_nmt_verify*) and sampling_kernels.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cda.h"

namespace cda {

// The device memory of a retained square (one allocation owned by its cda_square):
//   eds     (2k)^2 cells of 512 B, row-major
//   leaf    (2k)^2 leaf records of 96 B, cell-major (a cell's leaf is the same node in its row and its column tree)
//   levels  the records of tree levels 1 .. log2(2k), each level [tree][node] with trees 0..2k-1 the rows and
//           2k..4k-1 the columns (launch_nmt_level's layout); level h starts square_level_offset(log2w, h) records in
struct SquareView {
  const uint8_t* eds;
  const uint8_t* leaf;
  const uint8_t* levels;
  int log2w;
};
// records of levels 1 .. h - 1 of the 4k trees: 2w (w / 2 + .. + w >> (h - 1))
__host__ __device__ inline size_t square_level_offset(int log2w, int h) {
  const size_t w = (size_t)1 << log2w;
  return 2 * w * (w - (w >> (h - 1)));
}

// cda_nmt_verify's arguments, all device memory (include/cda.h)
struct VerifyArgs {
  const cda_nmt_proof_desc* descs;
  const uint8_t* namespaces;
  const uint8_t* roots;
  const uint8_t* nodes;
  const uint8_t* leaves;
  uint8_t* ok;
  uint32_t nproofs, nroots, nnodes_total, nleaves_total;
};

// d_share_off (nq words of scratch) and d_shares: both null when the cells are not wanted
int launch_square_prove(const SquareView& v, const cda_range_query* d_q, uint32_t nq, uint32_t max_nodes,
                        int32_t* d_counts, uint8_t* d_nodes, uint32_t* d_share_off, uint8_t* d_shares, hipStream_t s);
// ranges = false: no descriptor has more than one leaf (the kernel of the longer proofs is not launched)
int launch_nmt_verify(const VerifyArgs& a, bool ranges, hipStream_t s);

}  // namespace cda
