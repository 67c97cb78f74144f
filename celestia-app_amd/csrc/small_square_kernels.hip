// small_square_kernels.hip — a whole small square (k = 1, 2, 4, 8) from ODS to DAH in one workgroup.
//
// A k <= 8 block has at most 256 EDS cells.  Through the block pipeline (engine.cpp) it costs the same chain of
// launches as a k = 128 block -- two extension passes, leaf hashing, the tree levels, the DAH -- each of them a handful
// of waves waiting on launch latency.  small_square_kernel runs that chain in one 256-thread workgroup per block, the
// phases separated by workgroup barriers only (no cross-workgroup counter, no scratch in the context), so all small
// blocks of a mixed-size call (mixed.cpp), whatever their sizes, cost one launch.  Each workgroup reads a descriptor
// (mixed_route.h): log2 k, where the block's ODS, EDS and root records start, and its index for the status word and
// the DAH.
//
//  1. rows and columns of the ODS: the k rows (k codewords of k shards) bit-sliced into state A, the k columns into
//     state B, both from one read of the ODS, which also goes out as Q0.  Leopard GF(2^8) IFFT then FFT with the
//     radix-2 layers of rs_encode8_kernel (rs8_lds_dev.h); a state holds its k codewords side by side as 16 k units of
//     one m = k transform, since a layer's matrix depends on the shard index only.  A -> Q1, B -> Q2.
//  2. Q3 = the columns of Q1: A transposed into B in LDS (the top half is never read back from memory), encoded, out.
//  3. leaf records: one cell per thread, the record computed once and kept in LDS for the cell's row tree and its
//     column tree (nmt_dev.h: parity namespace outside Q0, push order against the Q0 neighbours with the block path's
//     key).  Q0 cells are read from the ODS; the parity cells from the EDS this workgroup has just written.
//  4. trees: the 4k trees of 2k leaves level by level between two LDS buffers, the 4k roots out as 96-B records.  The
//     node is hash_node_mem, which reads its children block by block, not trees_lds_kernel's hash_node_regs: with both
//     children in registers that kernel takes 249 VGPRs, and this one is held to 128 with no spill
//     (tests/test_small_square_registers.py).
//  5. DAH: RFC-6962 over the 4k roots (dah_leaf_digest, dah_fold_kw).
//
// LDS (mixed_route.h small_square_lds_bytes): the 256 layer matrices c_col8[c_skew8[i]] staged from a table in global
// memory filled at context creation (this translation unit cannot reach rs_kernels.hip's constant tables), then one
// region used in turn by the codec states, the records and levels, and the DAH fold: 66 KiB at k = 8.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cda_internal.h"
#include "gf_slice.h"
#include "mixed_route.h"
#include "nmt_dev.h"
#include "rs8_lds_dev.h"
#include "small_square.h"

namespace cda {

static_assert(sizeof(SmallSquareDesc) == 32, "descriptor layout");
static_assert(kSmallSquareDahBytes >= (size_t)(48 * 8 + 64 * kKwStride) * 4, "DAH fold: 32 roots, 64 schedule rows");
static_assert(kSmallSquareCbBytes + 1024 * kSmallSquareMaxK * kSmallSquareMaxK <= (size_t)kSmallSquareMaxLds &&
                  kSmallSquareCbBytes + kSmallSquareDahBytes <= (size_t)kSmallSquareMaxLds,
              "LDS budget");

// rs_layer8's table object: every layer here takes its matrix from the LDS copy, so these are never read
struct NoConstTables {
  __device__ __forceinline__ unsigned skew(int) const { return 255u; }
  __device__ __forceinline__ unsigned long long col(unsigned) const { return 0ull; }
};

// One m = k Leopard encode of the state st ([8][k * U] words): IFFT layers D = 1 .. k/2, FFT layers D = k/2 .. 1;
// k = 1 has no layer (one codeword of one shard: the parity is the data).  Every layer ends in a barrier.
__device__ __forceinline__ void small_encode(uint32_t* st, int k, int log2k, int U, int log2U,
                                             const unsigned long long* s_cb) {
  for (int lD = 0; lD < log2k; lD++) rs_layer8<true>(st, k, U, log2U, 1 << lD, lD, s_cb, NoConstTables());
  for (int lD = log2k - 1; lD >= 0; lD--) rs_layer8<false>(st, k, U, log2U, 1 << lD, lD, s_cb, NoConstTables());
}

// The state's element e = s * U + cw * 16 + u un-sliced to 32 bytes of the cell (row0 + (by_cols ? s : cw),
// col0 + (by_cols ? cw : s)) of the EDS, row pitch w shares
__device__ __forceinline__ void small_store_quadrant(const uint32_t* st, int mU, int log2U, uint8_t* eds, int w,
                                                     int row0, int col0, bool by_cols) {
  for (int e = threadIdx.x; e < mU; e += blockDim.x) {
    const int s = e >> log2U, cw = (e >> 4) & ((1 << (log2U - 4)) - 1), u = e & 15;
    uint32_t v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = st[j * mU + lds_sw(e)];
    bitslice8(v);
    const int r = row0 + (by_cols ? s : cw), c = col0 + (by_cols ? cw : s);
    uint4* q = reinterpret_cast<uint4*>(eds + ((size_t)(r * w + c) * CDA_SHARE + u * 32));
    q[0] = make_uint4(v[0], v[1], v[2], v[3]);
    q[1] = make_uint4(v[4], v[5], v[6], v[7]);
  }
}

constexpr int kSmallRec = 7;  // uint4 per LDS record (112-B stride, as trees_lds_kernel)

__device__ __forceinline__ void small_load_rec(const uint4* p, uint32_t (&r)[24]) {
#pragma unroll
  for (int q = 0; q < 6; q++) {
    const uint4 v = p[q];
    r[4 * q] = v.x, r[4 * q + 1] = v.y, r[4 * q + 2] = v.z, r[4 * q + 3] = v.w;
  }
}

__global__ void __launch_bounds__(kSmallSquareThreads) __attribute__((amdgpu_waves_per_eu(4)))
    small_square_kernel(const SmallSquareDesc* __restrict__ descs, const uint8_t* __restrict__ ods_base,
                        uint8_t* eds_base, uint4* __restrict__ roots_base, uint32_t* __restrict__ dah,
                        unsigned long long* __restrict__ status, const unsigned long long* __restrict__ cb_table) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const SmallSquareDesc d = descs[blockIdx.x];
  const int log2k = (int)d.log2k, k = 1 << log2k, w = 2 * k, log2w = log2k + 1;
  const int log2U = 4 + log2k, U = 1 << log2U;  // a state's k codewords x 16 units of 32 B
  const int mU = k << log2U;                    // words per plane: 16 k^2
  const uint8_t* ods = ods_base + d.ods_off;
  uint8_t* eds = eds_base + d.eds_off;

  unsigned long long* s_cb = reinterpret_cast<unsigned long long*>(lds);
  uint32_t* region = lds + kSmallSquareCbBytes / 4;
  uint32_t* stA = region;           // rows: element (x = column, codeword = row)
  uint32_t* stB = region + 8 * mU;  // columns: element (x = row, codeword = column)
  if (log2k > 0)
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_cb[i] = cb_table[i];

  // ---- 1. the ODS once: Q0 out, rows into A, columns into B ----
  for (int e = threadIdx.x; e < mU; e += blockDim.x) {
    const int cell = e >> 4, u = e & 15, r = cell >> log2k, c = cell & (k - 1);
    const uint4* p = reinterpret_cast<const uint4*>(ods + ((size_t)cell * CDA_SHARE + u * 32));
    const uint4 v0 = p[0], v1 = p[1];
    uint4* q = reinterpret_cast<uint4*>(eds + ((size_t)(r * w + c) * CDA_SHARE + u * 32));
    q[0] = v0;
    q[1] = v1;
    uint32_t v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    bitslice8(v);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      stA[j * mU + lds_sw(c * U + r * 16 + u)] = v[j];
      stB[j * mU + lds_sw(r * U + c * 16 + u)] = v[j];
    }
  }
  __syncthreads();
  small_encode(stA, k, log2k, U, log2U, s_cb);
  small_encode(stB, k, log2k, U, log2U, s_cb);
  small_store_quadrant(stA, mU, log2U, eds, w, 0, k, false);  // Q1: row cw, column k + s
  small_store_quadrant(stB, mU, log2U, eds, w, k, 0, true);   // Q2: row k + s, column cw
  __syncthreads();                                            // B has been read

  // ---- 2. Q3: the columns of Q1, A transposed into B ----
  for (int e = threadIdx.x; e < mU; e += blockDim.x) {
    const int x = e >> log2U, cw = (e >> 4) & (k - 1), u = e & 15;
#pragma unroll
    for (int j = 0; j < 8; j++) stB[j * mU + lds_sw(e)] = stA[j * mU + lds_sw(cw * U + x * 16 + u)];
  }
  __syncthreads();
  small_encode(stB, k, log2k, U, log2U, s_cb);
  small_store_quadrant(stB, mU, log2U, eds, w, k, k, true);  // Q3: row k + s, column k + cw
  // The leaf phase reads parity cells that other threads of this workgroup have just stored to the EDS.  What is
  // relied on is __syncthreads() itself: it is a release fence and an acquire fence at workgroup scope around the
  // barrier, and those fences order global memory as well as LDS (the workgroup's waves share one CU's vector L1, which
  // writes through, so a load after the barrier sees a store before it).  It also ends the codec's use of the region.
  __syncthreads();

  // ---- 3. leaf records, one cell per thread ----
  // two buffers of w^2 records.  One generic pointer, made opaque once: hash_node_mem launders the pointers it is
  // given, and with the LDS-to-generic casts left to each of its uses the gfx950 backend failed to select one
  // ("Illegal instruction detected", a compare against the shared aperture base)
  uint4* P0 = reinterpret_cast<uint4*>(region);
  asm volatile("" : "+v"(P0));
  uint4* P1 = P0 + w * w * kSmallRec;
  if ((int)threadIdx.x < w * w) {
    const int r = threadIdx.x >> log2w, c = threadIdx.x & (w - 1);
    const bool q0 = r < k && c < k;
    const uint4* sh = reinterpret_cast<const uint4*>(q0 ? ods + (size_t)(r * k + c) * CDA_SHARE
                                                        : eds + (size_t)(r * w + c) * CDA_SHARE);
    uint32_t A[16];
    load16(sh, A);
    if (q0) {  // push order, as leaf_cell reads it from the ODS (rows k shares apart), with the same key
      if (c + 1 < k && ns_below(sh + CDA_SHARE / 16, A))
        atomicMin(status + d.block,
                  ((unsigned long long)CDA_AXIS_ROW << 40) | ((unsigned long long)r << 20) | (unsigned)(c + 1));
      if (r + 1 < k && ns_below(sh + (size_t)k * (CDA_SHARE / 16), A))
        atomicMin(status + d.block,
                  ((unsigned long long)CDA_AXIS_COL << 40) | ((unsigned long long)c << 20) | (unsigned)(r + 1));
    }
    leaf_record<false>(sh, A, q0, P0 + threadIdx.x * kSmallRec);
  }
  __syncthreads();

  // ---- 4. trees: level 1 from the cells (row trees, then column trees), then every tree alike ----
  if ((int)threadIdx.x < w * w) {
    const int half = w * w / 2, col = (int)threadIdx.x >= half, idx = threadIdx.x & (half - 1);
    const int tree = idx >> (log2w - 1), i = idx & (w / 2 - 1);
    const int cl = col ? (2 * i) * w + tree : tree * w + 2 * i, cr = col ? cl + w : cl + 1;
    hash_node_mem(P0 + cl * kSmallRec, P0 + cr * kSmallRec, P1 + ((col * w + tree) * (w / 2) + i) * kSmallRec);
  }
  __syncthreads();
  for (int l = 2; l <= log2w; l++) {
    const uint4* in = (l & 1) ? P0 : P1;
    uint4* out = (l & 1) ? P1 : P0;
    const int per = w >> l;  // nodes per tree of this level
    if ((int)threadIdx.x < 2 * w * per) {
      const int tree = threadIdx.x >> (log2w - l), i = threadIdx.x & (per - 1);
      hash_node_mem(in + (tree * 2 * per + 2 * i) * kSmallRec, in + (tree * 2 * per + 2 * i + 1) * kSmallRec,
                    out + (tree * per + i) * kSmallRec);
    }
    __syncthreads();
  }
  const uint4* rootbuf = (log2w & 1) ? P1 : P0;  // root of tree t (rows, then columns) at record t
  const int n = 2 * w;
  for (int x = threadIdx.x; x < n * 6; x += blockDim.x) {
    const int t = x / 6, q = x - t * 6;
    roots_base[(d.rec_off + t) * 6 + q] = rootbuf[t * kSmallRec + q];
  }

  // ---- 5. DAH ----
  uint32_t dg[8];
  if ((int)threadIdx.x < n) {
    uint32_t L[24];
    small_load_rec(rootbuf + threadIdx.x * kSmallRec, L);
    dah_leaf_digest(L, dg);
  }
  __syncthreads();  // the roots have been read: the fold takes the region
  uint32_t* sdig = region;
  if ((int)threadIdx.x < n)
#pragma unroll
    for (int t = 0; t < 8; t++) sdig[threadIdx.x * 8 + t] = dg[t];
  __syncthreads();
  dah_fold_kw(sdig, n, dah + (size_t)d.block * 8, sdig + (n + (n + 1) / 2) * 8);
}

// ---- host side ----
static unsigned long long* g_small_cb[64] = {nullptr};

int small_square_init(int device) {
  if (device < 0 || device >= 64) return -1;
  if (hipFuncSetAttribute((const void*)small_square_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          kSmallSquareMaxLds) != hipSuccess)
    return -1;
  if (g_small_cb[device]) return 0;
  const LeoTables& t = leo_tables(8);
  unsigned long long cb[256];
  for (int i = 0; i < 255; i++) cb[i] = leo8_colbits(t.skew[i]);  // c_col8[c_skew8[i]]; 0 = no multiply
  cb[255] = 0;
  void* p = nullptr;
  if (hipMalloc(&p, sizeof cb) != hipSuccess) return -1;
  if (hipMemcpy(p, cb, sizeof cb, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(p);
    return -1;
  }
  g_small_cb[device] = (unsigned long long*)p;
  return 0;
}

int launch_small_squares(const SmallSquareDesc* d_descs, uint32_t n, uint32_t kmax, const uint8_t* d_ods,
                         uint8_t* d_eds, void* d_roots, void* d_dah, unsigned long long* d_status, hipStream_t s) {
  if (n == 0 || n > 0x7FFFFFFFu || kmax < 1 || kmax > kSmallSquareMaxK) return -2;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64 || !g_small_cb[dev]) return -1;
  hipLaunchKernelGGL(small_square_kernel, dim3(n), dim3(kSmallSquareThreads), small_square_lds_bytes(kmax), s,
                     d_descs, d_ods, d_eds, (uint4*)d_roots, (uint32_t*)d_dah, d_status, g_small_cb[dev]);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cda
