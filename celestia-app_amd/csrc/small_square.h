// small_square.h — launcher of small_square_kernel (small_square_kernels.hip) for the mixed-size batch (mixed.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mixed_route.h"

namespace cda {

// the layer-matrix table of `device` and the kernel's LDS limit (cda_init); 0, or -1
int small_square_init(int device);
// One workgroup per descriptor (kmax: the largest k among them, which sizes the LDS).  Offsets are relative to d_ods /
// d_eds (bytes) and d_roots (96-B records); descriptor `block` indexes d_dah (32 B) and d_status, whose words the
// caller has set to all-ones.  The ODS must not overlap the EDS.  0, -1 (launch error) or -2 (not this kernel's shape).
int launch_small_squares(const SmallSquareDesc* d_descs, uint32_t n, uint32_t kmax, const uint8_t* d_ods,
                         uint8_t* d_eds, void* d_roots, void* d_dah, unsigned long long* d_status, hipStream_t s);

}  // namespace cda
