// Small per-element pieces of the scores, stated once for the kernels that
// score without a gradient: skge_score.hip (every TransE form but the L1 quad
// layout, which goes through skge_transe_l1.h; HolE outside the quad kernels)
// and k_rel_query (skge_relation.hip).
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace skge
