// blob_kernels.hip — the device side of cda_square_index and cda_square_read: the ordered scan that finds
// the sequences of a retained square under share_index_rule.h, and the gather that copies their payload bytes out with
// the share headers stripped.  The host side is blob.cpp.
#include <hip/hip_runtime.h>

#include "blob.h"
#include "share_index_rule.h"

namespace cda {

namespace {

constexpr int kScanBlock = 1024, kScanWaves = kScanBlock / 64;

// bytes [0, 34) of ODS share g out of Q0 of the retained EDS (cells are 512-byte aligned)
__device__ __forceinline__ ShareHead load_head(const uint8_t* __restrict__ eds, uint32_t k, uint32_t g) {
  const uint8_t* p = eds + ((size_t)(g / k) * (2 * (size_t)k) + g % k) * CDA_SHARE;
  const uint4 a = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + 16);
  ShareHead h;
  h.w[0] = a.x, h.w[1] = a.y, h.w[2] = a.z, h.w[3] = a.w;
  h.w[4] = b.x, h.w[5] = b.y, h.w[6] = b.z, h.w[7] = b.w;
  h.w[8] = *reinterpret_cast<const uint32_t*>(p + 32) & 0xFFFFu;
  return h;
}

// The two ordered scans inside a workgroup of kScanBlock lanes, lane t for share block * kScanBlock + t.  Marks ascend
// with the share index, so the max over the lanes before t is the mark of the nearest start lane before t: a ballot,
// the highest set bit below the lane and one cross-lane read in the wave, the nearest wave with a start before it
// through LDS.  The count of sequence starts before t is a popcount of the ballot plus the waves' counts before.
struct BlockScan {
  uint32_t prev;   // max mark over the workgroup's lanes before this one (0: none)
  uint32_t count;  // sequence starts among them
  uint32_t block_mark, block_count;  // over the whole workgroup
};
__device__ __forceinline__ BlockScan block_scan(uint32_t mark, bool is_seq, uint32_t* wave_mark,
                                                uint32_t* wave_count) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1;
  const unsigned long long starts = __ballot(mark != 0), seqs = __ballot(is_seq);
  const unsigned long long before = starts & below;
  // every lane takes part in the cross-lane read; lanes with no start before them read their own mark and drop it
  const uint32_t got = (uint32_t)__shfl((int)mark, before ? 63 - __clzll((long long)before) : (int)lane);
  BlockScan r;
  r.prev = before ? got : 0u;
  r.count = (uint32_t)__popcll(seqs & below);
  const uint32_t top = (uint32_t)__shfl((int)mark, starts ? 63 - __clzll((long long)starts) : 0);
  if (lane == 0) {
    wave_mark[wave] = starts ? top : 0u;
    wave_count[wave] = (uint32_t)__popcll(seqs);
  }
  __syncthreads();
  uint32_t pm = 0, pc = 0, bm = 0, bc = 0;
#pragma unroll
  for (int i = 0; i < kScanWaves; i++) {
    const uint32_t m = wave_mark[i], n = wave_count[i];
    if ((uint32_t)i < wave) pm = max(pm, m), pc += n;
    bm = max(bm, m), bc += n;
  }
  r.prev = max(r.prev, pm);
  r.count += pc;
  r.block_mark = bm;
  r.block_count = bc;
  return r;
}

// Pass 1 of a square of more than one workgroup: each workgroup's totals.
__global__ void __launch_bounds__(kScanBlock)
share_scan_totals_kernel(const uint8_t* __restrict__ eds, uint32_t k, uint32_t* __restrict__ blk_mark,
                         uint32_t* __restrict__ blk_count) {
  __shared__ uint32_t wave_mark[kScanWaves], wave_count[kScanWaves];
  const uint32_t g = blockIdx.x * kScanBlock + threadIdx.x, n = k * k;
  uint32_t mark = 0;
  bool is_seq = false;
  if (g < n) {
    const ShareHead h = load_head(eds, k, g);
    mark = h.mark(g);
    is_seq = h.sequence();
  }
  const BlockScan sc = block_scan(mark, is_seq, wave_mark, wave_count);
  if (threadIdx.x == 0) {
    blk_mark[blockIdx.x] = sc.block_mark;
    blk_count[blockIdx.x] = sc.block_count;
  }
}

// Pass 2: the scans again with the totals of the workgroups before this one in front (every workgroup folds those
// itself: at most 256 words, nothing is handed from workgroup to workgroup inside the launch), then every share's
// part under the rule.  A sequence's start share writes its record at the slot the count gives it; the word that holds
// kind, version and status is OR-ed into the zeroed record by the start share and by every share that breaks the
// sequence, so no order of arrival shows.  counters: nseq, npadding, norphans (sums) and first_orphan (a min).
__global__ void __launch_bounds__(kScanBlock)
share_index_kernel(const uint8_t* __restrict__ eds, uint32_t k, uint32_t threshold,
                   const uint32_t* __restrict__ blk_mark, const uint32_t* __restrict__ blk_count,
                   cda_sequence* __restrict__ recs, uint32_t* __restrict__ counters) {
  __shared__ uint32_t wave_mark[kScanWaves], wave_count[kScanWaves];
  __shared__ uint32_t front_mark, front_count, tot_pad, tot_orphans, min_orphan;
  const uint32_t g = blockIdx.x * kScanBlock + threadIdx.x, n = k * k;
  if (threadIdx.x == 0) {
    front_mark = front_count = tot_pad = tot_orphans = 0;
    min_orphan = kNoShare;
  }
  __syncthreads();
  if (threadIdx.x < blockIdx.x) {  // a square has at most kMaxBlobK^2 / kScanBlock = 256 workgroups
    atomicMax(&front_mark, blk_mark[threadIdx.x]);
    atomicAdd(&front_count, blk_count[threadIdx.x]);
  }
  ShareHead h{};
  uint32_t mark = 0;
  bool is_seq = false;
  if (g < n) {
    h = load_head(eds, k, g);
    mark = h.mark(g);
    is_seq = h.sequence();
  }
  const BlockScan sc = block_scan(mark, is_seq, wave_mark, wave_count);  // its barrier covers the front totals too
  const uint32_t prev = max(sc.prev, front_mark), slot = sc.count + front_count;
  bool orphan = false, pad = false;
  if (g < n) {
    ShareHead owner{};
    if (mark_is_sequence(prev)) owner = load_head(eds, k, mark_share(prev));
    const ShareRole role = share_role(g, h, prev, owner);
    orphan = role == kRoleOrphan;
    pad = h.padding();
    uint32_t* words = reinterpret_cast<uint32_t*>(recs);
    if (role == kRoleBreaks) atomicOr(words + (size_t)(slot - 1) * 12 + 3, (uint32_t)CDA_SEQ_BROKEN << 16);
    if (is_seq) {
      uint32_t* r = words + (size_t)slot * 12;
      r[0] = g;
      r[1] = h.nshares();
      r[2] = h.seq_len();
      atomicOr(r + 3, h.kind() | h.version() << 8 | h.own_status(g, k, threshold) << 16);
#pragma unroll
      for (int i = 0; i < 7; i++) r[4 + i] = h.w[i];
      r[11] = h.w[7] & 0xFFu;
    }
  }
  const unsigned long long orphans = __ballot(orphan), pads = __ballot(pad);
  if ((threadIdx.x & 63) == 0) {
    if (orphans) {
      atomicAdd(&tot_orphans, (uint32_t)__popcll(orphans));
      atomicMin(&min_orphan, g + (uint32_t)__ffsll((long long)orphans) - 1);
    }
    if (pads) atomicAdd(&tot_pad, (uint32_t)__popcll(pads));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (sc.block_count) atomicAdd(counters + 0, sc.block_count);
    if (tot_pad) atomicAdd(counters + 1, tot_pad);
    if (tot_orphans) {
      atomicAdd(counters + 2, tot_orphans);
      atomicMin(counters + 3, min_orphan);
    }
  }
}

// ---- cda_square_read ----
// One wave per share of a query ("unit"): the payload bytes of that share, a run that starts at byte 2 mod 4 of the
// share, to a destination of any phase.  The destination is cut at its dword boundaries: the head and the tail of
// fewer than 4 bytes go bytewise, every dword between is one aligned store of two aligned loads realigned in registers
// (v_alignbyte_b32).  The second load is left out where the source is in phase with the destination, so no load goes
// past the share.  -DCDA_BLOB_GATHER_BYTEWISE=1 builds the form this one was measured against: a byte per
// lane per access, build_ods_kernel's inner loop the other way round.  Neither form writes a byte outside
// [dst, dst + len).
#ifndef CDA_BLOB_GATHER_BYTEWISE
#define CDA_BLOB_GATHER_BYTEWISE 0
#endif
__device__ __forceinline__ void copy_run(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t len,
                                         uint32_t lane) {
#if CDA_BLOB_GATHER_BYTEWISE
  for (uint32_t i = lane; i < len; i += 64) dst[i] = src[i];
#else
  const uint32_t head = min(len, (uint32_t)(-(uintptr_t)dst & 3)), ndw = (len - head) >> 2;
  const uint32_t tail = head + 4 * ndw;
  if (lane < head) dst[lane] = src[lane];
  if (lane >= 60 && tail + (lane - 60) < len) dst[tail + (lane - 60)] = src[tail + (lane - 60)];
  const uintptr_t sp = (uintptr_t)(src + head);
  const uint32_t sh = (uint32_t)(sp & 3);
  const uint32_t* from = reinterpret_cast<const uint32_t*>(sp - sh);
  uint32_t* to = reinterpret_cast<uint32_t*>(dst + head);
  for (uint32_t i = lane; i < ndw; i += 64) {
    const uint32_t lo = from[i], hi = sh ? from[i + 1] : 0u;
    to[i] = __builtin_amdgcn_alignbyte(hi, lo, sh);
  }
#endif
}

__global__ void __launch_bounds__(256)
sequence_read_kernel(const uint8_t* __restrict__ eds, uint32_t k, const cda_sequence_range* __restrict__ q, uint32_t nq,
                     const uint32_t* __restrict__ unit_off, const unsigned long long* __restrict__ dst_off,
                     uint32_t nunits, uint8_t* __restrict__ out) {
  const uint32_t u = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (u >= nunits) return;
  uint32_t lo = 0, hi = nq;  // unit_off[lo] <= u < unit_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (unit_off[mid] <= u) lo = mid;
    else hi = mid;
  }
  const cda_sequence_range qq = q[lo];
  const bool compact = qq.compact != 0;
  const uint32_t j = u - unit_off[lo], g = qq.start + j, strip = seq_share_strip(compact, j);
  const uint64_t off = seq_share_off(compact, j);
  const uint32_t len = (uint32_t)min((uint64_t)(CDA_SHARE - strip), (uint64_t)qq.seq_len - off);
  const uint8_t* src = eds + ((size_t)(g / k) * (2 * (size_t)k) + g % k) * CDA_SHARE + strip;
  copy_run(out + dst_off[lo] + off, src, len, lane);
}

}  // namespace

int launch_share_index(const SquareView& v, uint32_t k, uint32_t threshold, uint32_t* d_blk_mark,
                       uint32_t* d_blk_count, cda_sequence* d_recs, uint32_t* d_counters, hipStream_t s) {
  const uint32_t nblk = (k * k + kScanBlock - 1) / kScanBlock;
  if (nblk > 1)
    hipLaunchKernelGGL(share_scan_totals_kernel, dim3(nblk), dim3(kScanBlock), 0, s, v.eds, k, d_blk_mark, d_blk_count);
  hipLaunchKernelGGL(share_index_kernel, dim3(nblk), dim3(kScanBlock), 0, s, v.eds, k, threshold, d_blk_mark,
                     d_blk_count, d_recs, d_counters);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_sequence_read(const SquareView& v, uint32_t k, const cda_sequence_range* d_q, uint32_t nq,
                         const uint32_t* d_unit_off, const unsigned long long* d_dst_off, uint32_t nunits,
                         uint8_t* d_out, hipStream_t s) {
  if (nunits == 0) return 0;
  const uint32_t grid = (uint32_t)(((size_t)nunits * 64 + 255) / 256);
  hipLaunchKernelGGL(sequence_read_kernel, dim3(grid), dim3(256), 0, s, v.eds, k, d_q, nq, d_unit_off, d_dst_off, nunits,
                     d_out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cda
