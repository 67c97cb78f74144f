// sampling.h — the retained square and the NMT verifier, which every proof and rebuild feature builds on: the view of
// a square's device memory, the two steps that build one (sampling.cpp), the verifier's arguments and launch and the
// prover's launch (sampling_kernels.hip), and the sizing of a workspace from its layout function.  Each feature's own
// argument structs, workspace layout and launches are in its header, which includes this one.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cda.h"
#include "arena.h"
#include "cda_internal.h"

namespace cda {

// The device memory of a retained square (one allocation owned by its cda_square):
//   eds     (2k)^2 cells of 512 B, row-major
//   leaf    (2k)^2 leaf records of 96 B, cell-major (a cell's leaf is the same node in its row and its column tree)
//   levels  the records of tree levels 1 .. log2(2k), each level [tree][node] with trees 0..2k-1 the rows and
//           2k..4k-1 the columns (launch_nmt_level's layout); level h starts square_level_offset(log2w, h) records in
//   dah_nodes  the RFC-6962 tree over rowRoots ‖ colRoots, 8k - 1 digests of 32 B: the 4k leaf hashes, then each
//           level, the data root last (cda_extend_commit_nodes' dah_nodes)
struct SquareView {
  const uint8_t* eds;
  const uint8_t* leaf;
  const uint8_t* levels;
  int log2w;
  const uint8_t* dah_nodes;
};
// records of levels 1 .. h - 1 of the 4k trees: 2w (w / 2 + .. + w >> (h - 1))
__host__ __device__ inline size_t square_level_offset(int log2w, int h) {
  const size_t w = (size_t)1 << log2w;
  return 2 * w * (w - (w >> (h - 1)));
}

}  // namespace cda

struct cda_square {
  cda_ctx* c = nullptr;  // null once the context was freed
  uint32_t k = 0;
  void* mem = nullptr;  // eds | leaf records | level records | data-root tree (SquareView)
  cda::SquareView view{};
};

namespace cda {

// A square being built (sampling.cpp): square_alloc makes the handle and its one allocation and sets the order-status
// word to "no error"; the caller puts the EDS into `eds` on `s` (the k x k ODS may pass through `levels`, which the
// extension has read before level 1 is written); square_commit commits what lies there (leaf hash, levels, DAH and
// data-root tree), brings the roots back in its one wait and hands the handle out.  Until then the destructor
// releases the half-built square, on every failure path (an exception included).  Lock held throughout.
struct SquareBuild {
  cda_square* sq = nullptr;
  uint8_t* eds = nullptr;
  uint8_t* leaf = nullptr;
  uint8_t* levels = nullptr;
  uint8_t* meta = nullptr;  // status [0, 8) | dah [256, 288) | data-root tree [512, ..)
  size_t eds_b = 0;
  SquareBuild() = default;
  SquareBuild(const SquareBuild&) = delete;
  SquareBuild& operator=(const SquareBuild&) = delete;
  ~SquareBuild();
};
int square_alloc(cda_ctx* c, uint32_t k, SquareBuild& b, hipStream_t s);
int square_commit(cda_ctx* c, uint32_t k, SquareBuild& b, cda_square** out, uint8_t* row_roots, uint8_t* col_roots,
                  uint8_t* dah, cda_err_info* err, hipStream_t s);

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
// ranges = false: no descriptor has more than one leaf (the kernel of the longer proofs is not launched)
int launch_nmt_verify(const VerifyArgs& a, bool ranges, hipStream_t s);

// d_share_off (nq words of scratch) and d_shares: both null when the cells are not wanted
int launch_square_prove(const SquareView& v, const cda_range_query* d_q, uint32_t nq, uint32_t max_nodes,
                        int32_t* d_counts, uint8_t* d_nodes, uint32_t* d_share_off, uint8_t* d_shares, hipStream_t s);

// Each workspace of a verifier has one statement of its layout, a walk over an Arena (arena.h): on a measuring arena it
// sizes the workspace, on the buffer it points the struct's workspace fields into it.
template <class Args>
size_t workspace_bytes(Args a, void (*layout)(Args&, Arena&)) {  // a: the counts the layout reads
  Arena measure;
  layout(a, measure);
  return measure.used();
}

}  // namespace cda
