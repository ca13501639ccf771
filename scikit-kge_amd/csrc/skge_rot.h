// RotatE: the relational rotation on rows in the lane-strided layout
// (skge_device.h: lane l holds elements l + 64k), stated once for the step
// kernels (skge_grad.hip) and the score kernel (skge_score.hip).
//
//   phi(s, p, o) = - sum_{j < d/2} | E_s[j] * R_p[j] - E_o[j] |
//
// over ComplEx's rows (skge_diag.h): d/2 complex components interleaved,
// (re, im) = (x[2j], x[2j + 1]), d even; * the complex product, | | the complex
// modulus sqrtf(re^2 + im^2) with the correctly rounded sqrtf.  The products
// are skge_diag.h's (diag_mul: x * y, diag_cmul: conj(x) * y).  With
// u = s * r - o, m = |u| and w = u / m per component (w = 0 where m == 0, as
// sign(0)):
//   d phi / d s = -conj(r) * w     d phi / d o = +w     d phi / d r = -conj(s) * w
// A component's other half is in lane l ^ 1 of the same register (one DPP quad
// permutation), so both lanes of a component form the same modulus bits: re is
// squared into the fma, im is the single multiply.  The zero fill past the row
// (load_row) gives u = 0, m = 0, w = 0 there: padding contributes nothing.
//
// Every product and sum is written with explicit fmaf / single multiplies, so
// the explicit-pair kernel (rot_pair) and the per-positive kernel (k_rot_pos),
// which share these functions, produce the same bits from the same rows.
#pragma once
#include "skge_diag.h"

namespace skge {

// u = x - y
template <int KM>
__device__ __forceinline__ void rot_sub(const float (&x)[KM], const float (&y)[KM],
                                        float (&u)[KM]) {
#pragma unroll
  for (int k = 0; k < KM; ++k) u[k] = x[k] - y[k];
}

// u <- u / |u| per complex component (0 where |u| == 0); returns sum_j |u_j|
// over the row: the moduli of a lane's components added in ascending k on the
// lane holding the real half, then wave_sum
template <int KM>
__device__ __forceinline__ float rot_unit(float (&u)[KM]) {
  const bool im = lane_id() & 1;
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    const float o = dpp_f<0xb1>(u[k]);
    const float re = im ? o : u[k], iv = im ? u[k] : o;
    const float m = sqrtf(fmaf(re, re, iv * iv));
    acc += im ? 0.0f : m;
    u[k] = m > 0.0f ? u[k] / m : 0.0f;
  }
  return wave_sum(acc);
}

// t = -x
template <int KM>
__device__ __forceinline__ void rot_neg(float (&t)[KM], const float (&x)[KM]) {
#pragma unroll
  for (int k = 0; k < KM; ++k) t[k] = -x[k];
}

// t = x - y: the row a pair adds where its positive's contribution x and its
// negative's -y land on the same id (acc_two's float sum of the two)
template <int KM>
__device__ __forceinline__ void rot_diff(float (&t)[KM], const float (&x)[KM],
                                         const float (&y)[KM]) {
#pragma unroll
  for (int k = 0; k < KM; ++k) t[k] = x[k] - y[k];
}

}  // namespace skge
