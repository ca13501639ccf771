// One quad-layout row's update -- segment mean, AdaGrad / SGD step and
// projection -- defined once for the two-launch packed apply (i16_finish,
// skge_update.hip), the pipelined and fused TransE runners (skge_pipe.h,
// skge_pipeline.hip) and the pipelined HolE runner (skge_hole_pipe.hip).
#pragma once
#include "skge_device.h"

namespace skge {

struct UpdParams {
  int opt, post;
  float lr, rin, rout, fdiv;   // g = (sum + rin*P)/div + rout*P, div = fdiv > 0 ? fdiv : count
};

// One row's update from its sums (floats, zero past the row) and occurrence
// count c > 0; the reference's arithmetic (skge/param.py:130, 147-155;
// skge/transe.py normalize).  Lanes past the row end with zeros.
// EXACT = false (the packed TransE-L1 sums: exact small integers): the step
// and the projection in the hardware's fast forms (adagrad_step_fast,
// proj_scale_fast).  Every packed apply shares this code, so a row's update
// has the same bits whichever kernel computes it.
// EXACT = true (HolE's fp32 sums): correctly rounded divides and square roots.
template <int KQ, bool EXACT = false>
__device__ __forceinline__ void row_update_s(const UpdParams& t, int c, int d,
                                             const float4 (&sms)[KQ], float4 (&p)[KQ],
                                             float4 (&a)[KQ]) {
  const int l = lane_id(), nq = d >> 2;
  const bool ada = t.opt == OPT_ADAGRAD;
  const float div = t.fdiv > 0.0f ? t.fdiv : (float)c;
  float ss = 0.0f;
#pragma unroll
  for (int m = 0; m < KQ; ++m) {
    const bool in = 64 * m + l < nq;
    const float4 sm = sms[m];
#define SKGE_UP(X)                                                      \
  {                                                                     \
    const float g = (sm.X + t.rin * p[m].X) / div + t.rout * p[m].X;    \
    float pv = p[m].X;                                                  \
    if (ada) {                                                          \
      a[m].X = a[m].X + g * g;                        /* param.py:147 */\
      if (EXACT)                                      /* 152-155 */     \
        pv = pv - (t.lr * g) / fmaxf(sqrtf(a[m].X), 1e-7f);             \
      else                                                              \
        pv = pv - adagrad_step_fast(t.lr, g, a[m].X);                   \
    } else {                                                            \
      pv = pv - t.lr * g;                             /* param.py:130 */\
    }                                                                   \
    p[m].X = in ? pv : 0.0f;                                            \
    ss += p[m].X * p[m].X;                                              \
  }
    SKGE_UP(x)
    SKGE_UP(y)
    SKGE_UP(z)
    SKGE_UP(w)
#undef SKGE_UP
  }
  if (t.post != POST_NONE) {   // param.py:165-166 / 171-173
    ss = wave_sum(ss);
    // EXACT: the norm, divided by; else its fast reciprocal, multiplied by
    const float k = EXACT ? (t.post == POST_NORMALIZE ? sqrtf(ss) : (ss < 1.0f ? 1.0f : ss))
                          : proj_scale_fast(t.post, ss);
    auto proj = [k](float x) { return EXACT ? x / k : x * k; };
#pragma unroll
    for (int m = 0; m < KQ; ++m) {
      p[m].x = proj(p[m].x);
      p[m].y = proj(p[m].y);
      p[m].z = proj(p[m].z);
      p[m].w = proj(p[m].w);
    }
  }
}

// The same from packed sums (W32: int32x2 in sv / sw, else int16x4 in sv)
template <int KQ, bool W32>
__device__ __forceinline__ void row_update(const UpdParams& t, int c, int d,
                                           const unsigned long long (&sv)[KQ],
                                           const unsigned long long (&sw)[KQ], float4 (&p)[KQ],
                                           float4 (&a)[KQ]) {
  const int l = lane_id(), nq = d >> 2;
  float4 sm[KQ];
#pragma unroll
  for (int m = 0; m < KQ; ++m) {
    const bool in = 64 * m + l < nq;
    if (W32) {   // int32x2 sums: quad q in words sv (elements 0, 1) and sw (2, 3)
      const float2 lo = unpack_i32x2(in ? sv[m] : 0ull), hi = unpack_i32x2(in ? sw[m] : 0ull);
      sm[m] = make_float4(lo.x, lo.y, hi.x, hi.y);
    } else {     // int16x4 sums
      sm[m] = unpack_i16x4(in ? sv[m] : 0ull);
    }
  }
  row_update_s<KQ>(t, c, d, sm, p, a);
}

}  // namespace skge
