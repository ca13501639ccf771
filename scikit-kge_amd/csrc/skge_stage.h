// Staging loads and the accumulator type of the fp32 MFMA kernels
// (skge_neighbours.hip, skge_rescal_tile.h).
#pragma once
#include <hip/hip_runtime.h>

namespace skge {

// the 16 accumulators a lane holds of a v_mfma_f32_32x32x2_f32 tile
typedef float f32x16 __attribute__((ext_vector_type(16)));

// four dims kk .. kk + 3 of a row, zeros past d and for a row past the end
// (ok false; row is then any readable row).  Every load is issued, from a
// clamped address, and masked afterwards: a branch around a load would make
// the loads wait for one another.  VEC: d % 4 == 0, one 16-byte load.
template <bool VEC>
__device__ __forceinline__ float4 stage_load4(const float* row, bool ok, int kk, int d) {
  float4 x;
  if (VEC) {
    x = *reinterpret_cast<const float4*>(row + (kk < d ? kk : 0));
  } else {
    x.x = row[kk < d ? kk : 0];
    x.y = row[kk + 1 < d ? kk + 1 : 0];
    x.z = row[kk + 2 < d ? kk + 2 : 0];
    x.w = row[kk + 3 < d ? kk + 3 : 0];
  }
  x.x = ok && kk < d ? x.x : 0.0f;
  x.y = ok && kk + 1 < d ? x.y : 0.0f;
  x.z = ok && kk + 2 < d ? x.z : 0.0f;
  x.w = ok && kk + 3 < d ? x.w : 0.0f;
  return x;
}

}  // namespace skge
