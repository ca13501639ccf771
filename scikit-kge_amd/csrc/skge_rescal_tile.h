// The RESCAL fp32-MFMA score tile of the evaluation entry points (DESIGN.md
// 3.8): sum_b (E_S W_j)[q][b] E_o[q][b] for the QB (s, o) rows of a workgroup
// and one relation j.  k_rel_rescal (skge_relation.hip: a block of pairs x a
// group of relations) and k_score_rescal (skge_score.hip: an item of triples
// of one relation) look their rows up, call this and write the sums, so a
// pair's score under relation j has the same bits from both.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "skge_stage.h"

namespace skge {

constexpr int RS_CB = 128;            // columns of W_j per pass: 4 waves x one 32-column MFMA tile
constexpr int RS_KC = 32;             // rows of W_j (dims of E_s) per LDS chunk
constexpr int RS_PADW = RS_CB + 1;    // k-major images with odd strides (k_nb_select's)

// One workgroup of 256 threads, every thread in the call.  s_s / s_o: the
// rows' entities in LDS, written and synchronised by the caller (a row that is
// not there names any entity); eok[u]: staging row (tid >> 3) + 32 u is there.
// Leaves the four waves' sums of row q in s_red[0 .. 3][q] (rescal_row_sum
// adds them) and returns after the barrier that makes them readable; the next
// call's staging barriers come between those reads and its writes.
//
// A = the block's E_s rows, B = W_j: lane l feeds A[q = l & 31][a = l >> 5] and
// B[a = l >> 5][b = l & 31] and holds T[q = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)]
// [b = l & 31] (k_nb_select's layout).  Wave w owns columns b0 + 32 w .. + 31 of
// every 128-column pass and all QB / 32 row tiles.  Per element the chain over
// a = 0 .. d - 1 from 0.0f is the MFMA's; the chunk's zero padding adds +0.
// The reduction over b, fixed: a lane folds its column of every pass into one
// partial (fma, passes ascending), the 32 lanes of a half-wave add by the xor
// butterfly 16, 8, 4, 2, 1, and the four waves' sums are added in wave order.
// A row's sum reads only row q of A, so it does not depend on the row's place
// in the block.  LDS 16.5 (QB 128) + 16.5 KB staging here.
template <int QB>
__device__ __forceinline__ void rescal_score_tile(const float* E, const float* Wj, int d,
                                                  const int* s_s, const int* s_o,
                                                  const bool (&eok)[QB / 32],
                                                  float (*s_red)[QB]) {
  constexpr int MI = QB / 32;
  constexpr int PADQ = QB + 1;
  __shared__ float sA[RS_KC * PADQ];
  __shared__ float sW[RS_KC * RS_PADW];
  const int tid = threadIdx.x;
  const int l = tid & 63, w = tid >> 6, h = l >> 5;
  // staging.  E_s: row (tid >> 3) + 32 u of the block, dims 4 (tid & 7) .. + 3
  // of the chunk.  W_j: row (tid >> 5) + 8 u of the chunk, columns
  // 4 (tid & 31) .. + 3 of the pass (b is the fastest index in memory).
  const int st_r = tid >> 3, st_k = (tid & 7) * 4;
  const int sw_r = tid >> 5, sw_c = (tid & 31) * 4;
  const float* erow[MI];
#pragma unroll
  for (int u = 0; u < MI; ++u) erow[u] = E + (size_t)s_s[st_r + 32 * u] * d;
  const bool vec = (d & 3) == 0;
  const int qi0 = l & 31;              // + 32 mi: this lane's A rows
  const int tj0 = 32 * w + (l & 31);   // this lane's B column of the pass
  float part[MI][16];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) part[mi][r] = 0.0f;
  for (int b0 = 0; b0 < d; b0 += RS_CB) {
    const bool active = b0 + 32 * w < d;   // wave-uniform: the tile has a column of W_j
    f32x16 acc[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][r] = 0.0f;
    for (int k0 = 0; k0 < d; k0 += RS_KC) {
      float4 ea[MI], wa[4];
      auto load = [&](auto v4) {
        constexpr bool VEC = decltype(v4)::value;
#pragma unroll
        for (int u = 0; u < MI; ++u) ea[u] = stage_load4<VEC>(erow[u], eok[u], k0 + st_k, d);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int ar = k0 + sw_r + 8 * u;
          wa[u] = stage_load4<VEC>(Wj + (size_t)(ar < d ? ar : 0) * d, ar < d, b0 + sw_c, d);
        }
      };
      if (vec)
        load(std::true_type());
      else
        load(std::false_type());
      __syncthreads();   // the previous chunk's reads are done
#pragma unroll
      for (int u = 0; u < MI; ++u) {
        float* p = sA + st_k * PADQ + st_r + 32 * u;
        p[0] = ea[u].x;
        p[PADQ] = ea[u].y;
        p[2 * PADQ] = ea[u].z;
        p[3 * PADQ] = ea[u].w;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float* p = sW + (sw_r + 8 * u) * RS_PADW + sw_c;
        p[0] = wa[u].x;
        p[1] = wa[u].y;
        p[2] = wa[u].z;
        p[3] = wa[u].w;
      }
      __syncthreads();
      if (active) {
        // two dims per MFMA; an odd tail's second dim is the chunk's zero
        // padding.  The next step's operands are read while this step's
        // MFMAs run (the last step reads its own again).
        const int steps = (min(RS_KC, d - k0) + 1) >> 1;
        float av[MI], bv;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) av[mi] = sA[h * PADQ + qi0 + 32 * mi];
        bv = sW[h * RS_PADW + tj0];
        for (int s = 0; s < steps; ++s) {
          const int kn = 2 * min(s + 1, steps - 1) + h;
          float an[MI], bn;
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) an[mi] = sA[kn * PADQ + qi0 + 32 * mi];
          bn = sW[kn * RS_PADW + tj0];
#pragma unroll
          for (int mi = 0; mi < MI; ++mi)
            acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mi], bv, acc[mi], 0, 0, 0);
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) av[mi] = an[mi];
          bv = bn;
        }
      }
    }
    if (active) {   // this pass's column of T times E_o[b]
      const int b = b0 + tj0;
      const bool bok = b < d;
      const int bc = bok ? b : 0;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qi = 32 * mi + (r & 3) + 8 * (r >> 2) + 4 * h;
          const float eo = E[(size_t)s_o[qi] * d + bc];
          part[mi][r] = fmaf(acc[mi][r], bok ? eo : 0.0f, part[mi][r]);
        }
    }
  }
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float x = part[mi][r];
#pragma unroll
      for (int off = 16; off >= 1; off >>= 1) x += __shfl_xor(x, off);
      if ((l & 31) == 0) s_red[w][32 * mi + (r & 3) + 8 * (r >> 2) + 4 * h] = x;
    }
  __syncthreads();
}

template <int QB>
__device__ __forceinline__ float rescal_row_sum(const float (*s_red)[QB], int q) {
  return ((s_red[0][q] + s_red[1][q]) + s_red[2][q]) + s_red[3][q];
}

}  // namespace skge
