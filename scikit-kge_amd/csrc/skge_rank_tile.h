// The VALU score tile of the ranking and top-k entry points:
// the scores of one block of query vectors against 128 candidate rows, every
// score rank_score's sequential-k fp32 chain from 0.0f.  score_tile is the
// only copy; its callers differ in what they do with a finished tile:
//   rank_count_tile   counts the scores strictly above tgt[v] into raw[v]
//                     (k_rank_count2, skge_eval.hip: every row of a table;
//                     k_rank_count_pool, skge_pools.hip: a pool's rows)
//   k_topk_select     offers them to the queries' sorted lists (skge_topk.hip)
// and in their MAPPING of slots to vectors and of candidates to rows.
#pragma once
#include <hip/hip_runtime.h>

#include "skge_device.h"

namespace skge {

constexpr int RT_QB = 64;    // query vectors per workgroup of the counting pass
constexpr int RT_EB = 128;   // candidates per LDS tile
constexpr int RT_KC = 32;    // dims per LDS chunk
constexpr int RT_PADE = RT_EB + 4;   // rows stay 16-B aligned (the Q image: QB + 4)
enum { RT_L1 = 0, RT_L2SQ = 1, RT_DOT = 2 };   // -sum|q - e|, -sum (q - e)^2, sum e q
// RotatE: -sum_j |q_j - e_j| over the d/2 complex components (x[2j], x[2j + 1])
// of a row, the modulus sqrtf(t0^2 + t1^2) as sqrtf(fmaf(t0, t0, t1 * t1)),
// t = q - e.  d is even and so is RT_KC: a component never straddles a row's
// end or an LDS chunk.
constexpr int RT_CMOD = 3;

// the form a model's ranking entry points score with (both TransE codes as L1)
__host__ __device__ __forceinline__ int rank_form(int model) {
  return model == TRANSE_L1 || model == TRANSE_L2 ? RT_L1 : (model == ROTATE ? RT_CMOD : RT_DOT);
}

// rank_score (skge_device.h) by form; RT_CMOD: the tile's chain, one complex
// component per step in ascending order
template <int FORM>
__device__ __forceinline__ float rank_score_form(const float* __restrict__ q,
                                                 const float* __restrict__ e, int d) {
  if constexpr (FORM == RT_CMOD) {
    float acc = 0.0f;
    for (int k = 0; k + 1 < d; k += 2) {
      const float t0 = q[k] - e[k], t1 = q[k + 1] - e[k + 1];
      acc = acc - sqrtf(fmaf(t0, t0, t1 * t1));
    }
    return acc;
  } else {
    return rank_score<FORM == RT_L1>(q, e, d);
  }
}

// dims k .. k + 3 of a row of width d, zeros past d and for a row that is not
// there (ok false: nothing is read).  stage_load4 (skge_stage.h) is the MFMA
// kernels' form of this load and stays theirs: it reads a clamped address for
// an absent row too, and its caller picks the 16-byte path at compile time,
// which would double every instance of the tile below.
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

// The mapping of a workgroup that scores rows of the table itself for the
// vectors v0 .. v0 + QB - 1 of nv.  A mapping gives
//   vec(i)   the vector in slot i < QB, -1 for an empty slot
//   row(e)   the table row of candidate e
//   kept(i)  vec(i) again, for the thread that read it, at the counting's end
struct RankRows {
  int v0, nv;
  __device__ __forceinline__ int vec(int i) const { return v0 + i < nv ? v0 + i : -1; }
  __device__ __forceinline__ int row(int e) const { return e; }
  __device__ __forceinline__ int kept(int i) const { return vec(i); }
};

// RT_CMOD's pass over one staged chunk of kn dims (kn even): two dims, one
// complex component, per step
template <int QB>
__device__ __forceinline__ void cmod_chunk(float (*sQ)[QB + 4], float (*sE)[RT_PADE],
                                           int te, int tq, int kn, float (&acc)[8][QB / 16]) {
  constexpr int TQ = QB / 16;
  for (int k = 0; k + 1 < kn; k += 2) {
    const float4 ra = *reinterpret_cast<const float4*>(&sE[k][te]);
    const float4 rb = *reinterpret_cast<const float4*>(&sE[k][te + 4]);
    const float4 ia = *reinterpret_cast<const float4*>(&sE[k + 1][te]);
    const float4 ib = *reinterpret_cast<const float4*>(&sE[k + 1][te + 4]);
    const float er[8] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w};
    const float ei[8] = {ia.x, ia.y, ia.z, ia.w, ib.x, ib.y, ib.z, ib.w};
    float qr[TQ], qi[TQ];
    if constexpr (TQ == 4) {
      const float4 a4 = *reinterpret_cast<const float4*>(&sQ[k][tq]);
      const float4 b4 = *reinterpret_cast<const float4*>(&sQ[k + 1][tq]);
      qr[0] = a4.x, qr[1] = a4.y, qr[2] = a4.z, qr[3] = a4.w;
      qi[0] = b4.x, qi[1] = b4.y, qi[2] = b4.z, qi[3] = b4.w;
    } else {
      const float2 a2 = *reinterpret_cast<const float2*>(&sQ[k][tq]);
      const float2 b2 = *reinterpret_cast<const float2*>(&sQ[k + 1][tq]);
      qr[0] = a2.x, qr[1] = a2.y;
      qi[0] = b2.x, qi[1] = b2.y;
    }
#pragma unroll
    for (int x = 0; x < 8; ++x)
#pragma unroll
      for (int y = 0; y < TQ; ++y) {
        const float t0 = qr[y] - er[x], t1 = qi[y] - ei[x];
        acc[x][y] = acc[x][y] - sqrtf(fmaf(t0, t0, t1 * t1));
      }
  }
}

// One tile, by a workgroup of 256 threads: out[x][y] = the score of candidate
// e0 + te + x < eend under vector m.vec(tq + y), te = 8 (tid & 15), tq =
// TQ (tid >> 4), TQ = QB / 16; a candidate past eend and an empty slot score
// as zero rows.  QB: 64 or 32.  The 32-dim chunks of the vectors and the rows
// go k-major through sQ [RT_KC][QB + 4] and sE [RT_KC][RT_PADE], the caller's
// LDS: the first barrier in here orders the caller's earlier reads of them,
// and the caller puts one after the call before it writes them.
template <int FORM, int QB, class Map>
__device__ __forceinline__ void score_tile(const float* E, int d, const float* Q, int e0, int eend,
                                           const Map& m, float (*sQ)[QB + 4],
                                           float (*sE)[RT_PADE], float (&out)[8][QB / 16]) {
  constexpr int TQ = QB / 16;               // vectors per thread
  constexpr int NQ4 = QB / 32;              // float4 of the Q chunk per thread
  constexpr int LPV = 8 / NQ4;              // threads per vector's chunk
  const int tid = threadIdx.x;
  const int te = (tid & 15) * 8, tq = (tid >> 4) * TQ;
  // staging maps: Q chunk = QB vectors x 8 float4 (NQ4 per thread), candidate
  // chunk = 128 rows x 8 float4 (4 per thread); k fastest in global memory
  const int sq_v = tid / LPV, sq_k = (tid % LPV) * 4;       // + 4 LPV for the second float4
  const int se_e = tid >> 1, se_k = (tid & 1) * 4;          // + 8, 16, 24
  const int qv = m.vec(sq_v);
  const float* qrow = Q + (size_t)(qv >= 0 ? qv : 0) * d;
  const int e = e0 + se_e;
  const float* erow = E + (size_t)(e < eend ? m.row(e) : 0) * d;
  // a local accumulator, copied out at the end: with the caller's array in
  // its place the compiler pairs the packed fp32 operations along the vector
  // axis, which costs the k loop two moves and the overlap of its LDS reads
  float acc[8][TQ];
#pragma unroll
  for (int x = 0; x < 8; ++x)
#pragma unroll
    for (int y = 0; y < TQ; ++y) acc[x][y] = 0.0f;
  for (int k0 = 0; k0 < d; k0 += RT_KC) {
    float4 qa[NQ4], ea[4];
#pragma unroll
    for (int u = 0; u < NQ4; ++u) qa[u] = rank_load4(qrow, qv >= 0, k0 + sq_k + 4 * LPV * u, d);
#pragma unroll
    for (int u = 0; u < 4; ++u) ea[u] = rank_load4(erow, e < eend, k0 + se_k + 8 * u, d);
    __syncthreads();   // the previous chunk's (or the caller's) reads are done
#pragma unroll
    for (int u = 0; u < NQ4; ++u) {
      const int k = sq_k + 4 * LPV * u;
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
    if constexpr (FORM == RT_CMOD) {
      cmod_chunk<QB>(sQ, sE, te, tq, kn, acc);
      continue;
    }
    for (int k = 0; k < kn; ++k) {
      const float4 e4a = *reinterpret_cast<const float4*>(&sE[k][te]);
      const float4 e4b = *reinterpret_cast<const float4*>(&sE[k][te + 4]);
      const float ev[8] = {e4a.x, e4a.y, e4a.z, e4a.w, e4b.x, e4b.y, e4b.z, e4b.w};
      float qf[TQ];
      if constexpr (TQ == 4) {
        const float4 q4 = *reinterpret_cast<const float4*>(&sQ[k][tq]);
        qf[0] = q4.x, qf[1] = q4.y, qf[2] = q4.z, qf[3] = q4.w;
      } else {
        const float2 q2 = *reinterpret_cast<const float2*>(&sQ[k][tq]);
        qf[0] = q2.x, qf[1] = q2.y;
      }
#pragma unroll
      for (int x = 0; x < 8; ++x)
#pragma unroll
        for (int y = 0; y < TQ; ++y) {
          if (FORM == RT_L1) {
            acc[x][y] = acc[x][y] - fabsf(qf[y] - ev[x]);
          } else if (FORM == RT_L2SQ) {
            const float t = qf[y] - ev[x];
            acc[x][y] = fmaf(-t, t, acc[x][y]);
          } else {
            acc[x][y] = fmaf(ev[x], qf[y], acc[x][y]);
          }
        }
    }
  }
#pragma unroll
  for (int x = 0; x < 8; ++x)
#pragma unroll
    for (int y = 0; y < TQ; ++y) out[x][y] = acc[x][y];
}

// One workgroup of 256 threads: raw[v] += #{candidates of [ebeg, eend), ebeg <
// eend, scoring strictly above tgt[v]} for the 64 vectors of mapping m.  The
// scores are rank_score's, so the true entity never outranks itself; counts
// go to LDS and then to raw by integer atomics.
template <int FORM, class Map>
__device__ __forceinline__ void rank_count_tile(const float* E, int d, const float* Q,
                                                const float* tgt, int* raw, int ebeg, int eend,
                                                const Map m) {
  __shared__ __attribute__((aligned(16))) float sQ[RT_KC][RT_QB + 4];
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
  for (int e0 = ebeg; e0 < eend; e0 += RT_EB) {
    float acc[8][4];
    score_tile<FORM, RT_QB>(E, d, Q, e0, eend, m, sQ, sE, acc);
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
