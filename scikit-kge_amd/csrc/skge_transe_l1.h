// TransE-L1 pair arithmetic in the quad row layout (load_row4: lane l holds
// quads l, l + 64, ...), defined once for every kernel that scores a positive
// and its two corrupted pairs: k_pipe_batch, k_pipe_fused and
// k_pipe_dp_scatter (skge_pipeline.hip), transe_l1_front / transe_l1_commit
// (skge_epoch.hip) and k_shard_score (skge_shard.hip).  They include this
// header, so the two-launch loop, the pipelined and fused runners, the
// data-parallel scatter and the row-sharded step take bitwise the same
// decisions and add bitwise the same contributions.  Loads, pending / hot
// rows, slot commits and entity-sum adds differ per kernel and stay there.
#pragma once
#include "skge_device.h"

namespace skge {

// Per-lane partial L1 sums of the positive (ps) and of pair 0 (s', o, p) and
// pair 1 (s, o', p) (n0, n1), and the sign sub-gradients of the positive (gp)
// and of both negatives (g0, g1), from the rows of s, o, s', o' and p.
template <int KQ>
__device__ __forceinline__ void l1_scores_signs(const float4 (&es)[KQ], const float4 (&eo)[KQ],
                                                const float4 (&fs)[KQ], const float4 (&fo)[KQ],
                                                const float4 (&rp)[KQ], float& ps, float& n0,
                                                float& n1, float4 (&gp)[KQ], float4 (&g0)[KQ],
                                                float4 (&g1)[KQ]) {
  ps = n0 = n1 = 0.0f;
#pragma unroll
  for (int m = 0; m < KQ; ++m) {
#define SKGE_EL(X)                                                                    \
  {                                                                                   \
    const float vp = (es[m].X + rp[m].X) - eo[m].X;   /* transe.py:32 */              \
    const float v0 = (fs[m].X + rp[m].X) - eo[m].X;                                   \
    const float v1 = (es[m].X + rp[m].X) - fo[m].X;                                   \
    ps += fabsf(vp);                                                                  \
    n0 += fabsf(v0);                                                                  \
    n1 += fabsf(v1);                                                                  \
    gp[m].X = signf_np(-((eo[m].X - rp[m].X) - es[m].X)); /* transe.py:103,115 */     \
    g0[m].X = signf_np((eo[m].X - rp[m].X) - fs[m].X);    /* transe.py:104,117 */     \
    g1[m].X = signf_np((fo[m].X - rp[m].X) - es[m].X);                                \
  }
    SKGE_EL(x)
    SKGE_EL(y)
    SKGE_EL(z)
    SKGE_EL(w)
#undef SKGE_EL
  }
}

// The wave's three scores and the margin tests: pair k violates (vk = 1) when
// it has a negative (negk >= 0) and that negative scores within the margin
// of the positive.  Wave-uniform (wave_sum gives every lane the same bits).
__device__ __forceinline__ void l1_decide(float ps, float n0, float n1, int neg0, int neg1,
                                          float margin, int& v0, int& v1) {
  const float pscore = -wave_sum(ps);
  const float ns0 = -wave_sum(n0), ns1 = -wave_sum(n1);
  v0 = (neg0 >= 0 && ns0 + margin > pscore) ? 1 : 0;   // strict >, transe.py:73
  v1 = (neg1 >= 0 && ns1 + margin > pscore) ? 1 : 0;
}

// One quad of the contributions to rows s, o, s', o', p (cs, co, c0, c1, cr)
// from the violation flags as floats (fv0, fv1) and the sign quads:
// pair 0 lists (sp,op,sn,on) = (s,o,s',o): (+gp,-gp,+g0,-g0),
// pair 1 lists (sp,op,sn,on) = (s,o,s,o'): (+gp,-gp,+g1,-g1)
// (skge/transe.py:128-160 before the segment mean); small exact integers.
// Per quad and by value: callers loop over their KQ quads (k_pipe_dp_scatter
// decodes one quad at a time; an array form through one more reference level
// cost k_transe_l1_sample_grad_i16<2> a VGPR and with it a wave per SIMD).
__device__ __forceinline__ void l1_contrib(float fv0, float fv1, const float4 gp, const float4 g0,
                                           const float4 g1, float4& cs, float4& co, float4& c0,
                                           float4& c1, float4& cr) {
#define SKGE_CO(X)                                         \
  cs.X = fv0 * gp.X + fv1 * (gp.X + g1.X);                 \
  co.X = -(fv0 * (gp.X + g0.X) + fv1 * gp.X);              \
  c0.X = g0.X;                                             \
  c1.X = -g1.X;                                            \
  cr.X = fv0 * (gp.X + g0.X) + fv1 * (gp.X + g1.X);
  SKGE_CO(x)
  SKGE_CO(y)
  SKGE_CO(z)
  SKGE_CO(w)
#undef SKGE_CO
}

// cr into the packed relation row rrow: int16x4 sums (word q holds quad q), or
// int32x2 (W32: words 2q, 2q + 1) when a hot relation's batch total could
// pass 16 bits
template <int KQ, bool W32>
__device__ __forceinline__ void l1_add_rel(unsigned long long* rrow, const float4 (&cr)[KQ],
                                           int d) {
  const int l = lane_id(), nq = d >> 2;
#pragma unroll
  for (int m = 0; m < KQ; ++m) {
    const int q = 64 * m + l;
    if (q < nq) {
      if (W32) {
        atomicAdd(rrow + 2 * q, pack_i32x2(cr[m].x, cr[m].y));
        atomicAdd(rrow + 2 * q + 1, pack_i32x2(cr[m].z, cr[m].w));
      } else {
        atomicAdd(rrow + q, pack_i16x4(cr[m]));
      }
    }
  }
}

}  // namespace skge
