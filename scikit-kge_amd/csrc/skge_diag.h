// DistMult and ComplEx: the trilinear forms on rows in the lane-strided layout
// (skge_device.h: lane l holds elements l + 64k), stated once for the step
// kernels (skge_grad.hip) and the score kernel (skge_score.hip).
//
//   DistMult  phi = sum_k s_k r_k o_k
//   ComplEx   phi = Re sum_j r_j s_j conj(o_j), a row of width d holding d/2
//             complex components interleaved: (re, im) = (x[2j], x[2j + 1])
//
// With x * y the elementwise product (DistMult) or the complex one (ComplEx):
//   d phi / d s = conj(r) * o     d phi / d o = s * r     d phi / d r = conj(s) * o
// and phi = s . (d phi / d s) = o . (d phi / d o) = r . (d phi / d r) as plain
// dot products over the d floats.  In the lane-strided layout element e sits in
// lane e mod 64, so the other half of a complex component is in lane l ^ 1 of
// the same register: one DPP quad permutation (0xb1, wave_sum's first step),
// no LDS.  d is even, so no component straddles the row's end, and the zero
// fill past the row (load_row) stays zero through every product.
//
// Every product and sum is written with explicit fmaf / single multiplies, so
// the explicit-pair kernel and the per-positive kernel, which share these
// functions, produce the same bits from the same rows.
#pragma once
#include "skge_device.h"

namespace skge {

__host__ __device__ constexpr bool is_diag(int model) { return model == DISTMULT || model == COMPLEX; }

// out = conj(x) * y   (DistMult: x * y)
template <int MODEL, int KM>
__device__ __forceinline__ void diag_cmul(const float (&x)[KM], const float (&y)[KM],
                                          float (&out)[KM]) {
  if constexpr (MODEL == COMPLEX) {
    const bool im = lane_id() & 1;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const float xp = dpp_f<0xb1>(x[k]), yp = dpp_f<0xb1>(y[k]);
      // re: Re x Re y + Im x Im y;   im: Re x Im y - Im x Re y
      out[k] = im ? fmaf(xp, y[k], -(x[k] * yp)) : fmaf(x[k], y[k], xp * yp);
    }
  } else {
#pragma unroll
    for (int k = 0; k < KM; ++k) out[k] = x[k] * y[k];
  }
}

// out = x * y
template <int MODEL, int KM>
__device__ __forceinline__ void diag_mul(const float (&x)[KM], const float (&y)[KM],
                                         float (&out)[KM]) {
  if constexpr (MODEL == COMPLEX) {
    const bool im = lane_id() & 1;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const float xp = dpp_f<0xb1>(x[k]), yp = dpp_f<0xb1>(y[k]);
      // re: Re x Re y - Im x Im y;   im: Re x Im y + Im x Re y
      out[k] = im ? fmaf(xp, y[k], x[k] * yp) : fmaf(x[k], y[k], -(xp * yp));
    }
  } else {
#pragma unroll
    for (int k = 0; k < KM; ++k) out[k] = x[k] * y[k];
  }
}

// x . q over the row: one fma chain per lane in ascending k, then wave_sum
template <int KM>
__device__ __forceinline__ float diag_dot(const float (&x)[KM], const float (&q)[KM]) {
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < KM; ++k) acc = fmaf(x[k], q[k], acc);
  return wave_sum(acc);
}

// the row a pair adds where its positive's and its negative's contribution
// land on the same id: g u + h v, as one rounding sequence
template <int KM>
__device__ __forceinline__ void diag_axpby(float (&t)[KM], float g, const float (&u)[KM], float h,
                                           const float (&v)[KM]) {
#pragma unroll
  for (int k = 0; k < KM; ++k) t[k] = fmaf(h, v[k], g * u[k]);
}

template <int KM>
__device__ __forceinline__ void diag_scale(float (&t)[KM], float g, const float (&u)[KM]) {
#pragma unroll
  for (int k = 0; k < KM; ++k) t[k] = g * u[k];
}

// rows a (g u) and b (h v) of one pair: merged when a == b (acc_two's rule)
template <int KM>
__device__ __forceinline__ void diag_acc_pair(const Accum& acc, int a, float g,
                                              const float (&u)[KM], int b, float h,
                                              const float (&v)[KM], int d) {
  float t[KM];
  if (a == b) {
    diag_axpby<KM>(t, g, u, h, v);
    acc_row<KM>(acc, a, t, d);
  } else {
    diag_scale<KM>(t, g, u);
    acc_row<KM>(acc, a, t, d);
    diag_scale<KM>(t, h, v);
    acc_row<KM>(acc, b, t, d);
  }
}

// One add per element for up to two contributions x (if ux) and y (if uy) to
// one row.  ACC_FX64: each contribution is rounded to fixed point on its own
// and the integers are summed, so the row receives exactly what two acc_row
// calls would add; fp32: the float sum.
template <int KM>
__device__ __forceinline__ void diag_acc_row2(const Accum& a, int row, const float (&x)[KM],
                                              bool ux, const float (&y)[KM], bool uy, int d) {
  const int l = lane_id();
  if (a.mode == ACC_FX64) {
    unsigned long long* base = reinterpret_cast<unsigned long long*>(a.sum) + (size_t)row * a.width;
    bool wrapped = false;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const int e = l + 64 * k;
      const long long add = (ux ? fx_enc(x[k]) : 0ll) + (uy ? fx_enc(y[k]) : 0ll);
      if (e < d && add != 0) {
        const unsigned long long old = atomicAdd(base + e, (unsigned long long)add);
        const long long res = (long long)(old + (unsigned long long)add);
        wrapped = wrapped || ((((long long)old ^ res) & (add ^ res)) < 0);
      }
    }
    if (wrapped && a.err) atomicOr(a.err, 4);
    return;
  }
  float* base = a.sum + (size_t)row * a.width;
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    const int e = l + 64 * k;
    if (e < d) atomicAdd(base + e, (ux ? x[k] : 0.0f) + (uy ? y[k] : 0.0f));
  }
}

}  // namespace skge
