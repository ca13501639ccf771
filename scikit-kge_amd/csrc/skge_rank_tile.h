// The VALU counting tile of the ranking entry points: for up
// to 64 query vectors and a range of candidates, raw[v] += #{candidates
// scoring strictly above tgt[v] under Q[v]}.  k_rank_count2 (skge_eval.hip:
// every row of a table, the vectors in order) and k_rank_count_pool
// (skge_pools.hip: a pool's rows, the vectors through the order array) are
// this tile with their own mapping.
#pragma once
#include <hip/hip_runtime.h>

namespace skge {

constexpr int RT_QB = 64;    // query vectors per workgroup
constexpr int RT_EB = 128;   // candidates per LDS tile
constexpr int RT_KC = 32;    // dims per LDS chunk
constexpr int RT_PADQ = RT_QB + 4, RT_PADE = RT_EB + 4;   // rows stay 16-B aligned

// dims k .. k + 3 of a row of width d, zeros past d and for a row that is not
// there (ok false: nothing is read)
__device__ __forceinline__ float4 rank_load4(const float* row, bool ok, int k, int d) {
  float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (ok) {
    if ((d & 3) == 0 && k + 3 < d) {
      x = *reinterpret_cast<const float4*>(row + k);
    } else {
      x.x = k < d ? row[k] : 0.0f;
      x.y = k + 1 < d ? row[k + 1] : 0.0f;
      x.z = k + 2 < d ? row[k + 2] : 0.0f;
      x.w = k + 3 < d ? row[k + 3] : 0.0f;
    }
  }
  return x;
}

// The mapping of a workgroup that counts over rows [ebeg, eend) of the table
// itself for the vectors v0 .. v0 + 63.  A mapping gives
//   vec(i)   the vector in slot i < 64, -1 for an empty slot
//   row(e)   the table row of candidate e
//   kept(i)  vec(i) again, for the thread that read it, at the tile's end
struct RankRows {
  int v0, nv;
  __device__ __forceinline__ int vec(int i) const { return v0 + i < nv ? v0 + i : -1; }
  __device__ __forceinline__ int row(int e) const { return e; }
  __device__ __forceinline__ int kept(int i) const { return vec(i); }
};

// One workgroup of 256 threads: the 64 vectors of mapping m x candidates
// [ebeg, eend), ebeg < eend.  Thread = 8 candidates x 4 vectors, every
// accumulator a sequential-k chain from 0.0f (rank_score's arithmetic, so the
// true entity never outranks itself); counts go to LDS and then to raw by
// integer atomics.
template <bool L1, class Map>
__device__ __forceinline__ void rank_count_tile(const float* E, int d, const float* Q,
                                                const float* tgt, int* raw, int ebeg, int eend,
                                                const Map m) {
  __shared__ __attribute__((aligned(16))) float sQ[RT_KC][RT_PADQ];
  __shared__ __attribute__((aligned(16))) float sE[RT_KC][RT_PADE];
  __shared__ int s_raw[RT_QB];
  __shared__ float s_tgt[RT_QB];
  const int tid = threadIdx.x;
  if (tid < RT_QB) {
    const int v = m.vec(tid);
    s_tgt[tid] = v >= 0 ? tgt[v] : INFINITY;
    s_raw[tid] = 0;
  }
  const int te = (tid & 15) * 8, tq = (tid >> 4) * 4;
  int cnt[4] = {0, 0, 0, 0};
  // staging maps: Q chunk = 64 vectors x 8 float4 (2 per thread), candidate
  // chunk = 128 rows x 8 float4 (4 per thread); k fastest in global memory
  const int sq_v = tid >> 2, sq_k = (tid & 3) * 4;          // + 16 for the second float4
  const int se_e = tid >> 1, se_k = (tid & 1) * 4;          // + 8, 16, 24
  const int qv = m.vec(sq_v);
  const float* qrow = Q + (size_t)(qv >= 0 ? qv : 0) * d;
  for (int e0 = ebeg; e0 < eend; e0 += RT_EB) {
    float acc[8][4];
#pragma unroll
    for (int x = 0; x < 8; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y) acc[x][y] = 0.0f;
    const int e = e0 + se_e;
    const float* erow = E + (size_t)(e < eend ? m.row(e) : 0) * d;
    for (int k0 = 0; k0 < d; k0 += RT_KC) {
      float4 qa[2], ea[4];
#pragma unroll
      for (int u = 0; u < 2; ++u) qa[u] = rank_load4(qrow, qv >= 0, k0 + sq_k + 16 * u, d);
#pragma unroll
      for (int u = 0; u < 4; ++u) ea[u] = rank_load4(erow, e < eend, k0 + se_k + 8 * u, d);
      __syncthreads();   // the previous chunk's reads are done
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int k = sq_k + 16 * u;
        sQ[k][sq_v] = qa[u].x;
        sQ[k + 1][sq_v] = qa[u].y;
        sQ[k + 2][sq_v] = qa[u].z;
        sQ[k + 3][sq_v] = qa[u].w;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = se_k + 8 * u;
        sE[k][se_e] = ea[u].x;
        sE[k + 1][se_e] = ea[u].y;
        sE[k + 2][se_e] = ea[u].z;
        sE[k + 3][se_e] = ea[u].w;
      }
      __syncthreads();
      const int kn = min(RT_KC, d - k0);
      for (int k = 0; k < kn; ++k) {
        const float4 e4a = *reinterpret_cast<const float4*>(&sE[k][te]);
        const float4 e4b = *reinterpret_cast<const float4*>(&sE[k][te + 4]);
        const float4 q4 = *reinterpret_cast<const float4*>(&sQ[k][tq]);
        const float ev[8] = {e4a.x, e4a.y, e4a.z, e4a.w, e4b.x, e4b.y, e4b.z, e4b.w};
        const float qf[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int x = 0; x < 8; ++x)
#pragma unroll
          for (int y = 0; y < 4; ++y)
            acc[x][y] = L1 ? acc[x][y] - fabsf(qf[y] - ev[x]) : fmaf(ev[x], qf[y], acc[x][y]);
      }
    }
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const float t = s_tgt[tq + y];
#pragma unroll
      for (int x = 0; x < 8; ++x)
        if (e0 + te + x < eend && acc[x][y] > t) ++cnt[y];
    }
  }
#pragma unroll
  for (int y = 0; y < 4; ++y)
    if (cnt[y]) atomicAdd(&s_raw[tq + y], cnt[y]);
  __syncthreads();
  if (tid < RT_QB) {
    const int v = m.kept(tid);
    if (v >= 0 && s_raw[tid]) atomicAdd(raw + v, s_raw[tid]);
  }
}

}  // namespace skge
