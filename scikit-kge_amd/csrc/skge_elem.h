// Small per-element pieces of the scores, stated once for the kernels that
// score without a gradient: skge_score.hip (every TransE form but the L1 quad
// layout, which goes through skge_transe_l1.h; HolE outside the quad kernels)
// and the query-vector kernels of the evaluation entry points (k_rank_query,
// skge_eval.hip; k_topk_query, skge_topk.hip; k_rel_query, skge_relation.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/skge_hip.h"

namespace skge {

// one dimension of TransE's score: |E_s + R_p - E_o| or its square
// (transe.py:32; transe_pair's element, skge_grad.hip)
template <bool L1>
__device__ __forceinline__ float transe_elem(float es, float rp, float eo) {
  const float v = (es + rp) - eo;
  return L1 ? fabsf(v) : v * v;
}

// ccorr(a, b)_k = sum_j a[j] b[(j + k) mod d] by the definition, one fma chain
// in ascending j (skge/util.py:30-50); a, b: d floats each, in LDS
__device__ __forceinline__ float ccorr_direct_k(const float* a, const float* b, int d, int k) {
  float c = 0.0f;
  for (int j = 0; j < d; ++j) {
    int ip = j + k;
    ip -= ip >= d ? d : 0;
    c = fmaf(a[j], b[ip], c);
  }
  return c;
}

// cconv(a, b)_k = sum_j a[j] b[(k - j) mod d], the same chain
__device__ __forceinline__ float cconv_direct_k(const float* a, const float* b, int d, int k) {
  float c = 0.0f;
  for (int j = 0; j < d; ++j) {
    int im = k - j;
    im += im < 0 ? d : 0;
    c = fmaf(a[j], b[im], c);
  }
  return c;
}

// Dimension k of the vector q that turns a model's score over every candidate
// row x into one distance or dot product (skge_eval.hip header), for anchor row
// ea and relation row rp (d floats each, in LDS) or RESCAL's W [d][d]:
//            tail = true: x is the object      tail = false: x is the subject
//   TransE   ea + rp                           ea - rp
//   HolE     cconv(rp, ea)                     ccorr(rp, ea)
//   RESCAL   (ea W)_k = sum_j ea[j] W[j][k]    (W ea)_k = sum_j W[k][j] ea[j]
//   DistMult ea[k] rp[k]                       ea[k] rp[k]
//   ComplEx  (ea * rp)_k                       (conj(rp) * ea)_k
//   RotatE   ComplEx's two: |r| = 1 gives |s * r - o| = |s - conj(r) * o|, so
//            every candidate row is compared with the same vector (the score
//            tile's RT_CMOD form, skge_rank_tile.h)
// every sum one fma chain in ascending j.  ComplEx (skge_diag.h): * is the
// complex product over the interleaved components, (re, im) = (x[2j], x[2j+1]),
// d even; the tail form is d phi / d o, the head form d phi / d s.  With E_o
// for the anchor and E_s for the relation row the head form is d phi / d r,
// the relation query (skge_relation.hip).
__device__ __forceinline__ float query_elem(int model, bool tail, const float* ea, const float* rp,
                                            const float* W, int d, int k) {
  if (model == SKGE_TRANSE_L1 || model == SKGE_TRANSE_L2) return tail ? ea[k] + rp[k] : ea[k] - rp[k];
  if (model == SKGE_HOLE) return tail ? cconv_direct_k(rp, ea, d, k) : ccorr_direct_k(rp, ea, d, k);
  if (model == SKGE_DISTMULT) return ea[k] * rp[k];
  if (model == SKGE_COMPLEX || model == SKGE_ROTATE) {
    const int kp = k ^ 1;   // the component's other half
    if (k & 1)   // im: Re a Im r + Im a Re r   |   Re r Im a - Im r Re a
      return tail ? fmaf(ea[kp], rp[k], ea[k] * rp[kp]) : fmaf(rp[kp], ea[k], -(rp[k] * ea[kp]));
    // re: Re a Re r - Im a Im r   |   Re r Re a + Im r Im a
    return tail ? fmaf(ea[k], rp[k], -(ea[kp] * rp[kp])) : fmaf(rp[k], ea[k], rp[kp] * ea[kp]);
  }
  float c = 0.0f;
  for (int j = 0; j < d; ++j)
    c = tail ? fmaf(ea[j], W[(size_t)j * d + k], c) : fmaf(W[(size_t)k * d + j], ea[j], c);
  return c;
}

}  // namespace skge
