// rs8_lds_dev.h — device pieces of the LDS-resident Leopard GF(2^8) encoders: the bank swizzle of the plane-major
// state, the multiply-add by a layer matrix, one radix-2 butterfly and one layer by the whole workgroup.  Shared by
// rs_kernels.hip (rs_encode8_kernel; the GF(2^16) LDS encoder uses the swizzle) and small_square_kernels.hip.
//
// Translation units carry no relocatable device code, so each one reaches the 256 layer matrices c_col8[c_skew8[i]] its
// own way: rs_layer8 takes them from s_cb (an LDS copy indexed by skew index, 0 = no multiply) when that is given, and
// otherwise from `tab`, an empty object of the including file whose skew(i) and col(log_m) read that file's tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cda {

// LDS bank swizzle of the plane-major state of the LDS encoders ([plane][m*U] words, element e = x*U + u).  In a
// layer D the 32 lanes of a half-wave touch e with one bit fixed (bit log2(D*U)) and bits 0..5 otherwise free, so for
// D*U < 32 two lanes whose e differ in bit 5 only land in the same bank (2-way conflicts in every low layer).
// Flipping bits 0..4 when bit 5 is set separates them for any fixed bit, and keeps contiguous runs conflict-free.
__device__ __forceinline__ int lds_sw(int e) { return e ^ (((e >> 5) & 1) * 31); }

// x ^= M * y, M(j,b) = bit (8b+j) of cb
__device__ __forceinline__ void gf8_muladd(uint32_t x[8], const uint32_t y[8], unsigned long long cb) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    uint32_t acc = x[j];
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const uint32_t mask = 0u - (uint32_t)((cb >> (8 * b + j)) & 1ull);
      acc = __builtin_amdgcn_bitop3_b32(acc, y[b], mask, 0x78);  // acc ^ (y & mask)
    }
    x[j] = acc;
  }
}

template <bool INVERSE>
__device__ __forceinline__ void butterfly8(uint32_t* st, int mU, int U, int x, int y, int u, unsigned log_m,
                                           unsigned long long cb) {
  uint32_t X[8], Y[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    X[j] = st[j * mU + lds_sw(x * U + u)];
    Y[j] = st[j * mU + lds_sw(y * U + u)];
  }
  if (INVERSE) {  // IFFT2
#pragma unroll
    for (int j = 0; j < 8; j++) Y[j] ^= X[j];
    if (log_m != 255u) gf8_muladd(X, Y, cb);
  } else {  // FFT2
    if (log_m != 255u) gf8_muladd(X, Y, cb);
#pragma unroll
    for (int j = 0; j < 8; j++) Y[j] ^= X[j];
  }
#pragma unroll
  for (int j = 0; j < 8; j++) {
    st[j * mU + lds_sw(x * U + u)] = X[j];
    st[j * mU + lds_sw(y * U + u)] = Y[j];
  }
}

template <bool INVERSE, class Tables>
__device__ __forceinline__ void rs_layer8(uint32_t* st, int m, int U, int log2U, int D, int log2D,
                                          const unsigned long long* s_cb, Tables tab) {
  const int nbu = (m >> 1) << log2U;
  for (int bu = threadIdx.x; bu < nbu; bu += blockDim.x) {
    const int p = bu >> log2U, u = bu & (U - 1);
    const int s0 = (p >> log2D) << (log2D + 1);
    const int x = s0 | (p & (D - 1));
    const int y = x + D;
    const int idx = INVERSE ? (m - 1 + s0 + D) : (s0 + D - 1);
    if (s_cb) {  // latency launches: the layer's matrix from the LDS copy (0 = no multiply)
      unsigned long long cb = s_cb[idx];
      if ((D << log2U) >= 64) {
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)cb);
        const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(cb >> 32));
        cb = (unsigned long long)hi << 32 | lo;
      }
      butterfly8<INVERSE>(st, m << log2U, U, x, y, u, cb ? 0u : 255u, cb);
    } else if ((D << log2U) >= 64) {  // constant is wave-uniform: masks in SGPRs
      const int sidx = __builtin_amdgcn_readfirstlane(idx);
      const unsigned lm = tab.skew(sidx);
      butterfly8<INVERSE>(st, m << log2U, U, x, y, u, lm, tab.col(lm));
    } else {
      const unsigned lm = tab.skew(idx);
      butterfly8<INVERSE>(st, m << log2U, U, x, y, u, lm, tab.col(lm));
    }
  }
  __syncthreads();
}

}  // namespace cda
