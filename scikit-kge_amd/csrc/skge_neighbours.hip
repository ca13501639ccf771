// Nearest neighbours in embedding space: for a batch of query vectors, the k
// rows of a table T [N][d] with the largest cosine (or dot product), the
// query's own row left out when the query is a row of T.
//
// The job is one fp32 GEMM of the queries against T with a selection epilogue:
//   k_nb_norms    r_j = 1 / sqrt(T_j . T_j) (0 for a zero row), one lane per
//                 row: the squared norm is the same sequential fma chain as
//                 the dot products, which lanes cannot share
//   k_nb_select   workgroup = a block of QB queries x one slice of table
//                 rows; 128-row tiles of T and the query block go through LDS
//                 in 32-dim chunks and are contracted with
//                 v_mfma_f32_32x32x2_f32, whose result is bit for bit the
//                 k-ordered fmaf chain from 0.0f (a chunk's zero padding adds
//                 +0 to it); after a tile the scores are scaled, written to
//                 LDS query-major over the dead staging buffers, and each wave
//                 offers them to its queries' sorted key lists
//                 (skge_topk_list.h, as k_topk_select does)
// and k_list_merge (skge_topk.hip) takes the slices' lists into the final k.
// cos(q, j) = (dot * r_q) * r_j; the dot metric multiplies by 1.0f twice,
// which changes no bit.  The self entry becomes key 0, "no candidate".
#include <algorithm>
#include <type_traits>

#include "skge_host.h"
#include "skge_stage.h"
#include "skge_topk_list.h"

namespace skge {

constexpr int NB_TB = 128;            // table rows per LDS tile
constexpr int NB_KC = 32;             // dims per LDS chunk
constexpr int NB_PADT = NB_TB + 1;    // k-major images: a lane reads one dword, lanes along the rows

struct NbArgs {
  const float* T;
  const float* Q;        // [nq][d] or nullptr
  const int* rows;       // [nq] or nullptr
  int N, d, nq, k, cosine;
  const float* rT;       // workspace [N]: 1 / |T_j| (cosine)
  const float* rQ;       // workspace [nq]: 1 / |Q_i| (cosine, external queries)
  tkey_t* lists;         // workspace [nq][ns][k]
  int tslice, ns;        // table rows per slice (multiple of NB_TB), slices
};

// ---- reciprocal norms: one lane per row, the contract's chain ----
__global__ __launch_bounds__(256) void k_nb_norms(const float* __restrict__ X, int n, int d,
                                                  float* __restrict__ r) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const float* x = X + (size_t)j * d;
  float n2 = 0.0f;
  if ((d & 3) == 0) {
    for (int kk = 0; kk < d; kk += 4) {
      const float4 v = *reinterpret_cast<const float4*>(x + kk);
      n2 = fmaf(v.x, v.x, n2);
      n2 = fmaf(v.y, v.y, n2);
      n2 = fmaf(v.z, v.z, n2);
      n2 = fmaf(v.w, v.w, n2);
    }
  } else {
    for (int kk = 0; kk < d; ++kk) n2 = fmaf(x[kk], x[kk], n2);
  }
  r[j] = n2 == 0.0f ? 0.0f : 1.0f / sqrtf(n2);
}

// ---- selection: QB queries x one table slice per workgroup ----
// The four waves tile the QB x 128 score block WQ x WT, each wave MI x NJ
// MFMA tiles of 32 x 32 (QB 128: 2 x 2 waves of 2 x 2 tiles; QB 64: 2 x 2 of
// 1 x 2; QB 32: 1 x 4 of 1 x 1).  A = the queries, B = the table rows: lane l
// feeds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31] and holds
// D[i = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)][j = l & 31].  Staging: a
// thread loads 16 bytes of a row, 8 lanes a row's 128-byte chunk, and stores
// them k-major.  The scores of at most 64 queries at a time go to LDS (QB
// 128: two passes).  LDS: max(staging, scores) + lists = 32.3 + 16 KB (QB
// 128, k <= 16), 32.0 + 16 KB (QB 64, k <= 32), 20.3 + 32 KB (QB 32,
// k <= 128).
template <int QB, int KCAP>
__global__ __launch_bounds__(256, 2) void k_nb_select(NbArgs a) {
  constexpr int WQ = QB >= 64 ? 2 : 1, WT = 4 / WQ;
  constexpr int MI = QB / (32 * WQ), NJ = NB_TB / (32 * WT);
  constexpr int PADQ = QB + 1;
  constexpr int SQ = QB < 64 ? QB : 64;     // queries per score pass
  constexpr int NP = QB / SQ;
  constexpr int STAGE = NB_KC * (PADQ + NB_PADT);
  constexpr int SCORES = SQ * NB_TB;
  __shared__ float s_buf[STAGE > SCORES ? STAGE : SCORES];
  __shared__ tkey_t s_list[QB][KCAP];
  __shared__ int s_self[QB];
  __shared__ float s_rq[QB];
  float* sQ = s_buf;                      // [NB_KC][PADQ]
  float* sT = s_buf + NB_KC * PADQ;       // [NB_KC][NB_PADT]
  float* sS = s_buf;                      // [SQ][NB_TB]
  const int tid = threadIdx.x, d = a.d, k = a.k;
  const int l = tid & 63, w = tid >> 6, h = l >> 5;
  const int wq = w / WT, wt = w % WT;
  const int v0 = blockIdx.x * QB;
  const int tbeg = blockIdx.y * a.tslice;
  const int tend = a.N - tbeg < a.tslice ? a.N : tbeg + a.tslice;
  for (int i = tid; i < QB * KCAP; i += 256) (&s_list[0][0])[i] = 0;
  for (int i = tid; i < QB; i += 256) {
    const int v = v0 + i;
    int self = -1;
    float rq = 1.0f;
    if (v < a.nq) {
      if (!a.Q) self = a.rows ? a.rows[v] : v;
      if (a.cosine) rq = a.Q ? a.rQ[v] : a.rT[self];
    }
    s_self[i] = self;
    s_rq[i] = rq;
  }
  __syncthreads();
  // staging: row (tid >> 3) + 32 u of the block, dims 4 (tid & 7) .. + 3 of the chunk
  const int st_r = tid >> 3, st_k = (tid & 7) * 4;
  const float* qrow[QB / 32];
  bool qok[QB / 32];
#pragma unroll
  for (int u = 0; u < QB / 32; ++u) {
    const int i = st_r + 32 * u;
    const int v = v0 + i;
    qok[u] = v < a.nq;
    qrow[u] = !qok[u] ? a.T : a.Q ? a.Q + (size_t)v * d : a.T + (size_t)s_self[i] * d;
  }
  const bool vec = (d & 3) == 0;
  const int qi0 = wq * 32 * MI + (l & 31);     // + 32 mi: this lane's A rows
  const int tj0 = wt * 32 * NJ + (l & 31);     // + 32 nj: this lane's B columns
  for (int t0 = tbeg; t0 < tend; t0 += NB_TB) {
    f32x16 acc[MI][NJ];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][nj][r] = 0.0f;
    for (int k0 = 0; k0 < d; k0 += NB_KC) {
      float4 qa[QB / 32], ta[NB_TB / 32];
      auto load = [&](auto v4) {
        constexpr bool VEC = decltype(v4)::value;
#pragma unroll
        for (int u = 0; u < QB / 32; ++u) qa[u] = stage_load4<VEC>(qrow[u], qok[u], k0 + st_k, d);
#pragma unroll
        for (int u = 0; u < NB_TB / 32; ++u) {
          const int j = t0 + st_r + 32 * u;
          ta[u] = stage_load4<VEC>(a.T + (size_t)(j < tend ? j : tbeg) * d, j < tend, k0 + st_k, d);
        }
      };
      if (vec)
        load(std::true_type());
      else
        load(std::false_type());
      __syncthreads();   // the previous chunk's (or tile's score) reads are done
#pragma unroll
      for (int u = 0; u < QB / 32; ++u) {
        float* p = sQ + st_k * PADQ + st_r + 32 * u;
        p[0] = qa[u].x;
        p[PADQ] = qa[u].y;
        p[2 * PADQ] = qa[u].z;
        p[3 * PADQ] = qa[u].w;
      }
#pragma unroll
      for (int u = 0; u < NB_TB / 32; ++u) {
        float* p = sT + st_k * NB_PADT + st_r + 32 * u;
        p[0] = ta[u].x;
        p[NB_PADT] = ta[u].y;
        p[2 * NB_PADT] = ta[u].z;
        p[3 * NB_PADT] = ta[u].w;
      }
      __syncthreads();
      // two dims per MFMA; an odd tail's second dim is the chunk's zero padding
      const int steps = (min(NB_KC, d - k0) + 1) >> 1;
      // the next step's operands are read while this step's MFMAs run (the
      // last step reads its own again)
      float av[MI], bv[NJ];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) av[mi] = sQ[h * PADQ + qi0 + 32 * mi];
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj) bv[nj] = sT[h * NB_PADT + tj0 + 32 * nj];
      for (int s = 0; s < steps; ++s) {
        const int kn = 2 * min(s + 1, steps - 1) + h;
        float an[MI], bn[NJ];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) an[mi] = sQ[kn * PADQ + qi0 + 32 * mi];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) bn[nj] = sT[kn * NB_PADT + tj0 + 32 * nj];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int nj = 0; nj < NJ; ++nj)
            acc[mi][nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mi], bv[nj], acc[mi][nj], 0, 0, 0);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) av[mi] = an[mi];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) bv[nj] = bn[nj];
      }
    }
    float rj[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
      const int j = t0 + tj0 + 32 * nj;
      rj[nj] = a.cosine && j < tend ? a.rT[j] : 1.0f;
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      __syncthreads();   // the staging buffers' (the previous pass's score) reads are done
      if (NP == 1 || wq == p) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int qi = qi0 - (l & 31) + 32 * mi + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float rq = s_rq[qi];
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
              sS[(qi - p * SQ) * NB_TB + tj0 + 32 * nj] = (acc[mi][nj][r] * rq) * rj[nj];
          }
      }
      __syncthreads();
      for (int qq = w; qq < SQ; qq += 4) {   // wave-uniform
        const int qi = p * SQ + qq;
        const int v = v0 + qi;
        if (v >= a.nq) break;
        const int self = s_self[qi];
        const int ja = t0 + l, jb = t0 + 64 + l;
        const tkey_t c0 = ja < tend && ja != self ? make_key(sS[qq * NB_TB + l], ja) : 0;
        const tkey_t c1 = jb < tend && jb != self ? make_key(sS[qq * NB_TB + 64 + l], jb) : 0;
        list_offer2(s_list[qi], c0, c1, k, l, nullptr, nullptr, 0);
      }
    }
  }
  // this (query, slice)'s list: each wave writes the queries it owns
  __builtin_amdgcn_wave_barrier();
  for (int qi = w; qi < QB; qi += 4) {
    const int v = v0 + qi;
    if (v >= a.nq) break;
    list_store(a.lists + ((size_t)v * a.ns + blockIdx.y) * k, s_list[qi], k, l);
  }
}

// query block (shrinks as k grows: the lists' LDS), table slices: enough
// workgroups to fill the chip (slice_plan)
struct NbPlan {
  int qb_size, qb, tslice, ns;
};
static NbPlan nb_plan(int nq, int k, int N) {
  NbPlan p;
  p.qb_size = k <= 16 ? 128 : k <= 32 ? 64 : 32;
  p.qb = (nq + p.qb_size - 1) / p.qb_size;
  const SlicePlan sp = slice_plan(p.qb, (N + NB_TB - 1) / NB_TB);
  p.tslice = sp.per * NB_TB;
  p.ns = sp.ns;
  return p;
}
static size_t nb_r_bytes(int n) { return align256((size_t)n * sizeof(float)); }

}  // namespace skge

using namespace skge;

extern "C" size_t skge_neighbours_workspace_bytes(int nq, int N, int d, int k) {
  if (nq <= 0 || N <= 0 || d <= 0 || k < 1 || k > TK_KMAX) return 0;
  const NbPlan p = nb_plan(nq, k, N);
  return nb_r_bytes(N) + nb_r_bytes(nq) + (size_t)nq * p.ns * k * sizeof(tkey_t) + 256;
}

extern "C" int skge_neighbours(void* stream, const float* T, int N, int d, const float* Q,
                               const int* rows, int nq, int metric, int k, void* workspace,
                               size_t ws_bytes, int* ids_out, float* sim_out) {
  SKGE_CHECK_ARG(T && ids_out && sim_out, "NULL argument");
  SKGE_CHECK_ARG(N > 0 && d > 0 && nq >= 0, "bad sizes (N = %d, d = %d, nq = %d)", N, d, nq);
  SKGE_CHECK_ARG(metric == SKGE_SIM_COSINE || metric == SKGE_SIM_DOT, "unknown metric %d", metric);
  SKGE_CHECK_ARG(k >= 1 && k <= TK_KMAX, "k = %d outside 1 .. %d", k, TK_KMAX);
  SKGE_CHECK_ARG(!(Q && rows), "give query vectors or query rows, not both");
  SKGE_CHECK_ARG(Q || rows || nq == N, "no query form given: every row needs nq == N (%d != %d)",
                 nq, N);
  if (nq == 0) return SKGE_OK;
  SKGE_CHECK_ARG(workspace && ws_bytes >= skge_neighbours_workspace_bytes(nq, N, d, k),
                 "neighbours workspace needs %zu bytes",
                 skge_neighbours_workspace_bytes(nq, N, d, k));
  const NbPlan p = nb_plan(nq, k, N);
  float* rT = (float*)workspace;
  float* rQ = (float*)((char*)workspace + nb_r_bytes(N));
  NbArgs a = {};
  a.T = T;
  a.Q = Q;
  a.rows = rows;
  a.N = N;
  a.d = d;
  a.nq = nq;
  a.k = k;
  a.cosine = metric == SKGE_SIM_COSINE;
  a.rT = rT;
  a.rQ = rQ;
  a.lists = (tkey_t*)((char*)workspace + nb_r_bytes(N) + nb_r_bytes(nq));
  a.tslice = p.tslice;
  a.ns = p.ns;
  hipStream_t st = as_stream(stream);
  if (a.cosine) {
    hipLaunchKernelGGL(k_nb_norms, dim3((N + 255) / 256), dim3(256), 0, st, T, N, d, rT);
    if (Q) hipLaunchKernelGGL(k_nb_norms, dim3((nq + 255) / 256), dim3(256), 0, st, Q, nq, d, rQ);
  }
  if (p.qb_size == 128)
    hipLaunchKernelGGL((k_nb_select<128, 16>), dim3(p.qb, p.ns), dim3(256), 0, st, a);
  else if (p.qb_size == 64)
    hipLaunchKernelGGL((k_nb_select<64, 32>), dim3(p.qb, p.ns), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((k_nb_select<32, TK_KMAX>), dim3(p.qb, p.ns), dim3(256), 0, st, a);
  launch_list_merge(st, a.lists, nq, p.ns, k, ids_out, sim_out);
  SKGE_CHECK_LAUNCH("neighbours");
  return SKGE_OK;
}
