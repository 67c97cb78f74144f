// blob.h — what blob.cpp (the C ABI of cda_square_index and cda_square_read) and blob_kernels.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sampling.h"

namespace cda {

// the widest ODS the scan takes: k * k lanes in at most 256 workgroups of 1,024 (the widest the device path extends)
constexpr uint32_t kMaxBlobK = 512;
// shares one cda_square_read call may copy (one wave each)
constexpr uint64_t kMaxReadUnits = 1ull << 25;

// The sequences of the square under share_index_rule.h.  d_recs: k * k records, zeroed; d_counters: nseq, npadding,
// norphans = 0 and first_orphan = 0xFFFFFFFF; d_blk_mark / d_blk_count: ceil(k * k / 1024) words each.
int launch_share_index(const SquareView& v, uint32_t k, uint32_t threshold, uint32_t* d_blk_mark,
                       uint32_t* d_blk_count, cda_sequence* d_recs, uint32_t* d_counters, hipStream_t s);
// Payload bytes of nq checked queries to d_out + d_dst_off[q]; d_unit_off: nq + 1 words, the shares the queries
// before q take (seq_shares_needed); nunits = d_unit_off[nq].
int launch_sequence_read(const SquareView& v, uint32_t k, const cda_sequence_range* d_q, uint32_t nq,
                         const uint32_t* d_unit_off, const unsigned long long* d_dst_off, uint32_t nunits,
                         uint8_t* d_out, hipStream_t s);

}  // namespace cda
