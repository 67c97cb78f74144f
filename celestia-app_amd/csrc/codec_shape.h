// codec_shape.h — the launch shapes of the Leopard erasure decoder (rs_decode.hip) and of the GF(2^8) encoders
// (rs_kernels.hip) as pure functions of (k, shard length, number of codewords): plain C++ with no HIP include, shared
// by the launchers and by host code that builds with a plain C++ compiler (tests/san/codec_shape_dump.cpp, which
// tests/test_codec_shapes.py runs to pin which shapes the suite reaches).
//
// Both LDS kernels work on U units per workgroup (a unit is one lane's 32 bytes at GF(2^8), 64 at GF(2^16)) with the
// state [plane][n or m][U] in LDS; every index in them depends on U, so U is what a test has to vary.
#pragma once
#include <stddef.h>

namespace cda {

constexpr int kRsDecodeMaxLds = 144 * 1024;   // rs_decode_kernel's dynamic LDS cap (hipFuncSetAttribute)
constexpr int kRsEncode8MaxLds = 128 * 1024;  // rs_encode8_kernel's

inline int codec_ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) l++;
  return l;
}

// ---- decoder ----
struct RsDecodeShape {
  bool ok;  // false: not on the device path (the launcher's -2); nothing else is meaningful then
  int PL;   // bit planes: 8 (2k <= 256) or 16
  int m, log2m, n, log2n;
  int U, log2U, slices;  // units per workgroup, workgroups per codeword
  size_t lds_bytes;
  long long grid;
};

inline RsDecodeShape rs_decode_shape(int k, int shard_len, int ncw) {
  RsDecodeShape r{};
  if (k < 1 || k > 32768 || shard_len % 64 != 0 || ncw <= 0) return r;
  const bool ff16 = 2 * k > 256;
  r.log2m = codec_ilog2(k);
  r.m = 1 << r.log2m;
  r.n = 2 * r.m;
  r.log2n = r.log2m + 1;
  r.PL = ff16 ? 16 : 8;
  const int unit = r.PL * 4;  // bytes per lane unit
  const int units = shard_len / unit;
  int U = 16;
  while (U > 1 && (units % U || r.n * U > 1024)) U >>= 1;  // <= 4 derivative items per thread
  if (r.n * U > 1024) return r;                           // n > 1024 (k > 512): not on the device path yet
  // A few codewords (the per-axis Decode, a short crossword batch) leave most CUs idle: split each codeword's bytes
  // over more workgroups (fewer units each) until the launch has 512 of them -- a workgroup's latency falls with its
  // items per thread, and the error locator it recomputes is cheap next to that.
  while (U > 1 && (long long)ncw * (units / U) < 512) U >>= 1;
  r.U = U;
  r.log2U = codec_ilog2(U);
  r.slices = units / U;
  r.lds_bytes = (size_t)r.n * r.PL * U * 4 + (size_t)r.n * 8;
  if (r.lds_bytes > (size_t)kRsDecodeMaxLds) return r;
  r.grid = (long long)ncw * r.slices;
  if (r.grid > 0x7FFFFFFF) return r;
  r.ok = true;
  return r;
}

// ---- GF(2^8) encoder ----
// Latency launches: when the register encoder's grid would leave most CUs idle (one block: 64 / 128 workgroups
// for rows / columns at k = 128, a consensus band 16), the LDS encoder splits each codeword's bytes over
// workgroups of U = lat_u units (32 B each) instead, so the pass spreads over the chip.  lat_u: 0 = off; the
// release value is kRs8LatU (the test-hooks build reads it from the environment, rs_kernels.hip).
constexpr int kRs8LatU = 4;

inline bool rs8_lat_shape(int k, int shard_len, int cw_per_blk, int nblk, int lat_u) {
  const long long g2_grid = (long long)nblk * (cw_per_blk / 2) * (shard_len / 512);
  return lat_u && codec_ilog2(k) >= 4 && shard_len % (32 * lat_u) == 0 && g2_grid < 32;
}

// the register-resident encoder, 2 codewords per workgroup (rs_encode8_g2_kernel), takes the job
inline bool rs8_reg_batched_shape(int k, int shard_len, int cw_per_blk, int nblk, int lat_u) {
  return k >= 1 && k <= 128 && codec_ilog2(k) >= 4 && !rs8_lat_shape(k, shard_len, cw_per_blk, nblk, lat_u) &&
         k % 2 == 0 && cw_per_blk % 2 == 0 && shard_len > 0 && shard_len % 512 == 0;
}

// rs_encode8_g2_kernel's dynamic LDS for m = 2^L
inline size_t rs8_reg_lds_bytes(int L) { return L > 4 ? (size_t)(1 << L) * 32 * 16 : 0; }

struct RsEncode8Shape {
  bool ok;   // false: not this encoder's (the launcher's -2)
  bool reg;  // the register path (slices of 512 bytes, U and lat unused); otherwise the LDS path
  int log2m, m;
  int U, log2U, slices;
  int lat;  // LDS path: layer matrices staged in LDS, U = lat_u
  size_t lds_bytes;
  long long grid;
};

inline RsEncode8Shape rs_encode8_shape(int k, int shard_len, int cw_per_blk, int nblk, int lat_u) {
  RsEncode8Shape r{};
  if (k < 1 || k > 128 || shard_len % 64 != 0) return r;
  const int L = codec_ilog2(k);
  r.log2m = L;
  r.m = 1 << L;
  const bool lat = rs8_lat_shape(k, shard_len, cw_per_blk, nblk, lat_u);
  // Batched path: 2 codewords per workgroup, register-resident (k >= 16).
  if (rs8_reg_batched_shape(k, shard_len, cw_per_blk, nblk, lat_u)) {
    r.reg = true;
    r.slices = shard_len / 512;
    r.lds_bytes = rs8_reg_lds_bytes(L);
    r.grid = (long long)nblk * (cw_per_blk / 2) * r.slices;
    r.ok = r.grid > 0 && r.grid <= 0x7FFFFFFF;
    return r;
  }
  // General path (any k <= 128, any shard length, single codewords): LDS-resident.
  const int units = shard_len / 32;  // even
  int U = lat ? lat_u : 16;
  while (units % U) U >>= 1;
  r.U = U;
  r.log2U = codec_ilog2(U);
  r.slices = units / U;
  r.lat = lat ? 1 : 0;
  r.lds_bytes = (size_t)r.m * 8 * U * 4 + (lat ? 256 * 8 : 0);
  r.grid = (long long)nblk * cw_per_blk * r.slices;
  r.ok = r.grid > 0 && r.grid <= 0x7FFFFFFF;
  return r;
}

}  // namespace cda
