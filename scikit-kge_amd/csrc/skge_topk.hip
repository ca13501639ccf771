// Top-k link prediction on the device: the k best tails of (a, p, ?) or heads
// of (?, p, a) for a batch of queries.
//
// Every model's score of entity j under a query is a distance to, or a dot
// product with, one query vector (skge_eval.hip header): the vectors are
// k_rank_query's, the scores k_rank_count2's sequential fp32 chain.  New here
// only: SKGE_TRANSE_L2 scores -sum (q - E_j)^2, the model's training score
// (the ranking entry points score both TransE codes as L1).
//   k_topk_query    one wave per query: the query vector of the asked direction
//   k_topk_select   workgroup = a block of query vectors x one entity slice;
//                   entity tiles through LDS, a register micro-tile of
//                   scores, then each wave offers a tile's scores to its
//                   queries' sorted lists
//   k_topk_merge    one wave per query: the slices' lists into the final k
// The lists are 64-bit keys in one compare order: skge_topk_list.h.
// k_topk_select<.., GATHER> is the same selection over candidate pools: query
// blocks from a grouped work list, rows through an index (skge_pools.h;
// skge_topk_pools, skge_pools.hip).
#include <algorithm>

#include "skge_host.h"
#include "skge_pools.h"
#include "skge_topk_list.h"

namespace skge {

constexpr int TK_EB = 128;   // entities per LDS tile
constexpr int TK_KC = 32;    // dims per LDS chunk
constexpr int TK_PADE = TK_EB + 4;   // rows stay 16-B aligned
enum { TK_L1 = 0, TK_L2SQ = 1, TK_DOT = 2 };

struct TopkArgs {
  const float* E;
  const float* R;        // TransE / HolE: [M][d]; RESCAL: W [M][d][d]
  int N, d, model, nq, direction, k;
  const int* queries;    // [nq][2] (anchor, p)
  const int* excl_off;   // [nq + 1] or nullptr
  const int* excl_ent;
  float* Q;              // workspace [nq][d]
  tkey_t* lists;         // workspace [nq][ns][k]
  int eslice, ns;        // entities per slice (multiple of TK_EB), slices
  int* ent_out;          // [nq][k]
  float* score_out;      // [nq][k]
  PoolWork pw;           // the gathered selection's work list (k_topk_select<.., true>)
};

// ---- query vectors: one wave per query (k_rank_query's arithmetic) ----
__global__ __launch_bounds__(128) void k_topk_query(TopkArgs a) {
  __shared__ float sm[2][2 * 1024];
  const int wpb = blockDim.x >> 6, l = lane_id(), d = a.d;
  float* ea = sm[threadIdx.x >> 6];   // the anchor's row
  float* rp = ea + 1024;
  const bool dist = a.model == SKGE_TRANSE_L1 || a.model == SKGE_TRANSE_L2;
  const bool tail = a.direction == 0;
  for (int i = blockIdx.x * wpb + (threadIdx.x >> 6); i < a.nq; i += gridDim.x * wpb) {
    const int an = __builtin_amdgcn_readfirstlane(a.queries[2 * i]);
    const int p = __builtin_amdgcn_readfirstlane(a.queries[2 * i + 1]);
    for (int k = l; k < d; k += 64) {
      ea[k] = a.E[(size_t)an * d + k];
      if (a.model != SKGE_RESCAL) rp[k] = a.R[(size_t)p * d + k];
    }
    __builtin_amdgcn_wave_barrier();
    float* q = a.Q + (size_t)i * d;
    const float* W = a.R + (size_t)p * d * d;
    for (int k = l; k < d; k += 64) {
      float v;
      if (dist) {
        v = tail ? ea[k] + rp[k] : ea[k] - rp[k];
      } else if (a.model == SKGE_HOLE) {
        // cconv(R, E_a)_k = sum_j R_j E_a[(k-j) mod d]; ccorr(R, E_a)_k = sum_j R_j E_a[(j+k) mod d]
        float c = 0.0f;
        for (int j = 0; j < d; ++j) {
          int ix = tail ? k - j : j + k;
          ix += ix < 0 ? d : 0;
          ix -= ix >= d ? d : 0;
          c = fmaf(rp[j], ea[ix], c);
        }
        v = c;
      } else {   // RESCAL: (E_a W)_k = sum_j E_a[j] W[j][k]; (W E_a)_k = sum_j W[k][j] E_a[j]
        float c = 0.0f;
        for (int j = 0; j < d; ++j)
          c = tail ? fmaf(ea[j], W[(size_t)j * d + k], c) : fmaf(W[(size_t)k * d + j], ea[j], c);
        v = c;
      }
      q[k] = v;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- selection: QB query vectors x one entity slice per workgroup ----
// thread: 8 entities x QB / 16 queries, every accumulator a sequential-k
// chain (k_rank_count2's tiling and arithmetic).  After a tile the scores go
// to LDS (over the staging buffers) query-major, and wave w offers them to
// queries w, w + 4, ...: a query's list sits in LDS between tiles and in the
// wave's registers while one of the tile's scores beats its k-th entry.
// LDS: max(staging, scores) + lists = 33.0 + 16 KB (QB 64, k <= 32),
// 21.0 + 32 KB (QB 32, k <= 128).
// GATHER (skge_pools.h): the workgroup's queries are item blockIdx.x of the
// grouped work list, reached through its order array, and the candidate rows
// are its pool's entries (row pool_ent[base + e] for candidate e, + 0.5 KB of
// LDS for a tile's row ids); blockIdx.y is a slice of that pool.
template <int FORM, int QB, int KCAP, bool GATHER = false>
__global__ __launch_bounds__(256) void k_topk_select(TopkArgs a) {
  constexpr int PADQ = QB + 4;
  constexpr int TQ = QB / 16;               // queries per thread
  constexpr int NQ4 = QB / 32;              // float4 of the Q chunk per thread
  constexpr int LPV = 8 / NQ4;              // threads per query vector's chunk
  constexpr int STAGE = TK_KC * (PADQ + TK_PADE);
  constexpr int SCORES = QB * TK_PADE;
  __shared__ __attribute__((aligned(16))) float s_buf[STAGE > SCORES ? STAGE : SCORES];
  __shared__ tkey_t s_list[QB][KCAP];
  float (*sQ)[PADQ] = reinterpret_cast<float (*)[PADQ]>(s_buf);
  float (*sE)[TK_PADE] = reinterpret_cast<float (*)[TK_PADE]>(s_buf + TK_KC * PADQ);
  float (*sS)[TK_PADE] = reinterpret_cast<float (*)[TK_PADE]>(s_buf);
  const int tid = threadIdx.x, d = a.d, k = a.k;
  const int l = tid & 63, w = tid >> 6;
  __shared__ int s_rid[GATHER ? TK_EB : 1];
  int v0 = blockIdx.x * QB, nvec = a.nq;   // the block's vectors: slots v0 .. of [0, nvec)
  int ebeg = blockIdx.y * a.eslice;
  int eend = a.N - ebeg < a.eslice ? a.N : ebeg + a.eslice;
  int pool = -1;
  int64_t pbase = 0;
  if constexpr (GATHER) {
    if ((int)blockIdx.x >= *a.pw.n_items) return;
    const int4 it = a.pw.items[blockIdx.x];
    pool = it.x;
    v0 = it.y;
    nvec = it.y + it.z;
    pool_slice(pool_size(a.pw, pool, a.N, pbase), a.pw.ns, blockIdx.y, ebeg, eend);
  }
  // slot -> query id, candidate -> row id
  auto vec_of = [&](int slot) { return GATHER ? a.pw.order[slot] : slot; };
  auto row_of = [&](int e) { return GATHER && pool >= 0 ? a.pw.pool_ent[pbase + e] : e; };
  for (int i = tid; i < QB * KCAP; i += 256) (&s_list[0][0])[i] = 0;
  __syncthreads();
  const int te = (tid & 15) * 8, tq = (tid >> 4) * TQ;
  const int sq_v = tid / LPV, sq_k = (tid % LPV) * 4;       // + 4 LPV for the second float4
  const int se_e = tid >> 1, se_k = (tid & 1) * 4;          // + 8, 16, 24
  for (int e0 = ebeg; e0 < eend; e0 += TK_EB) {
    float acc[8][TQ];
#pragma unroll
    for (int x = 0; x < 8; ++x)
#pragma unroll
      for (int y = 0; y < TQ; ++y) acc[x][y] = 0.0f;
    for (int k0 = 0; k0 < d; k0 += TK_KC) {
      float4 qa[NQ4], ea[4];
      {
        const int v = v0 + sq_v;
        const float* qrow = a.Q + (size_t)(v < nvec ? vec_of(v) : 0) * d;
#pragma unroll
        for (int u = 0; u < NQ4; ++u) {
          const int kk = k0 + sq_k + 4 * LPV * u;
          float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          if (v < nvec) {
            if ((d & 3) == 0 && kk + 3 < d) {
              x = *reinterpret_cast<const float4*>(qrow + kk);
            } else {
              x.x = kk < d ? qrow[kk] : 0.0f;
              x.y = kk + 1 < d ? qrow[kk + 1] : 0.0f;
              x.z = kk + 2 < d ? qrow[kk + 2] : 0.0f;
              x.w = kk + 3 < d ? qrow[kk + 3] : 0.0f;
            }
          }
          qa[u] = x;
        }
        const int e = e0 + se_e;
        const float* erow = a.E + (size_t)(e < eend ? row_of(e) : GATHER ? 0 : ebeg) * d;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int kk = k0 + se_k + 8 * u;
          float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          if (e < eend) {
            if ((d & 3) == 0 && kk + 3 < d) {
              x = *reinterpret_cast<const float4*>(erow + kk);
            } else {
              x.x = kk < d ? erow[kk] : 0.0f;
              x.y = kk + 1 < d ? erow[kk + 1] : 0.0f;
              x.z = kk + 2 < d ? erow[kk + 2] : 0.0f;
              x.w = kk + 3 < d ? erow[kk + 3] : 0.0f;
            }
          }
          ea[u] = x;
        }
      }
      __syncthreads();   // the previous chunk's (or tile's score) reads are done
#pragma unroll
      for (int u = 0; u < NQ4; ++u) {
        const int kk = sq_k + 4 * LPV * u;
        sQ[kk][sq_v] = qa[u].x;
        sQ[kk + 1][sq_v] = qa[u].y;
        sQ[kk + 2][sq_v] = qa[u].z;
        sQ[kk + 3][sq_v] = qa[u].w;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int kk = se_k + 8 * u;
        sE[kk][se_e] = ea[u].x;
        sE[kk + 1][se_e] = ea[u].y;
        sE[kk + 2][se_e] = ea[u].z;
        sE[kk + 3][se_e] = ea[u].w;
      }
      __syncthreads();
      const int kn = min(TK_KC, d - k0);
      for (int kk = 0; kk < kn; ++kk) {
        const float4 e4a = *reinterpret_cast<const float4*>(&sE[kk][te]);
        const float4 e4b = *reinterpret_cast<const float4*>(&sE[kk][te + 4]);
        const float ev[8] = {e4a.x, e4a.y, e4a.z, e4a.w, e4b.x, e4b.y, e4b.z, e4b.w};
        float qv[TQ];
        if constexpr (TQ == 4) {
          const float4 q4 = *reinterpret_cast<const float4*>(&sQ[kk][tq]);
          qv[0] = q4.x, qv[1] = q4.y, qv[2] = q4.z, qv[3] = q4.w;
        } else {
          const float2 q2 = *reinterpret_cast<const float2*>(&sQ[kk][tq]);
          qv[0] = q2.x, qv[1] = q2.y;
        }
#pragma unroll
        for (int x = 0; x < 8; ++x)
#pragma unroll
          for (int y = 0; y < TQ; ++y) {
            if (FORM == TK_L1) {
              acc[x][y] = acc[x][y] - fabsf(qv[y] - ev[x]);
            } else if (FORM == TK_L2SQ) {
              const float t = qv[y] - ev[x];
              acc[x][y] = fmaf(-t, t, acc[x][y]);
            } else {
              acc[x][y] = fmaf(ev[x], qv[y], acc[x][y]);
            }
          }
      }
    }
    __syncthreads();   // the staging buffers' reads are done: the scores go over them
#pragma unroll
    for (int y = 0; y < TQ; ++y) {
      *reinterpret_cast<float4*>(&sS[tq + y][te]) =
          make_float4(acc[0][y], acc[1][y], acc[2][y], acc[3][y]);
      *reinterpret_cast<float4*>(&sS[tq + y][te + 4]) =
          make_float4(acc[4][y], acc[5][y], acc[6][y], acc[7][y]);
    }
    if constexpr (GATHER) {
      if (tid < TK_EB) s_rid[tid] = e0 + tid < eend ? row_of(e0 + tid) : -1;
    }
    __syncthreads();
    for (int qq = w; qq < QB; qq += 4) {   // wave-uniform
      if (v0 + qq >= nvec) break;
      const int v = vec_of(v0 + qq);
      const int ea0 = e0 + l, ea1 = e0 + 64 + l;
      const tkey_t c0 = ea0 < eend ? make_key(sS[qq][l], GATHER ? s_rid[l] : ea0) : 0;
      const tkey_t c1 = ea1 < eend ? make_key(sS[qq][64 + l], GATHER ? s_rid[64 + l] : ea1) : 0;
      tkey_t thr = s_list[qq][k - 1];
      if (__ballot(c0 > thr || c1 > thr) == 0) continue;
      tkey_t lo = l < k ? s_list[qq][l] : 0;
      tkey_t hi = 64 + l < k ? s_list[qq][64 + l] : 0;
      if (a.excl_off) {
        const int* xb = a.excl_ent + a.excl_off[v];
        const int* xe = a.excl_ent + a.excl_off[v + 1];
        list_offer<true>(lo, hi, thr, c0, k, l, xb, xe);
        list_offer<true>(lo, hi, thr, c1, k, l, xb, xe);
      } else {
        list_offer<false>(lo, hi, thr, c0, k, l, nullptr, nullptr);
        list_offer<false>(lo, hi, thr, c1, k, l, nullptr, nullptr);
      }
      if (l < k) s_list[qq][l] = lo;
      if (64 + l < k) s_list[qq][64 + l] = hi;
    }
  }
  // this (query, slice)'s list: each wave writes the queries it owns
  __builtin_amdgcn_wave_barrier();
  for (int qq = w; qq < QB; qq += 4) {
    if (v0 + qq >= nvec) break;
    const int v = vec_of(v0 + qq);
    tkey_t* out = a.lists + ((size_t)v * a.ns + blockIdx.y) * k;
    if (l < k) out[l] = s_list[qq][l];
    if (64 + l < k) out[64 + l] = s_list[qq][64 + l];
  }
}

// ---- merge: one wave per query, the slices' lists into the final k ----
__global__ __launch_bounds__(256) void k_topk_merge(TopkArgs a) {
  const int l = lane_id(), k = a.k;
  const int v = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (v >= a.nq) return;
  tkey_t lo = 0, hi = 0, thr = 0;
  for (int s = 0; s < a.ns; ++s) {
    const tkey_t* in = a.lists + ((size_t)v * a.ns + s) * k;
    const tkey_t c0 = l < k ? in[l] : 0;
    const tkey_t c1 = 64 + l < k ? in[64 + l] : 0;
    list_offer<false>(lo, hi, thr, c0, k, l, nullptr, nullptr);
    list_offer<false>(lo, hi, thr, c1, k, l, nullptr, nullptr);
  }
  int* eo = a.ent_out + (size_t)v * k;
  float* so = a.score_out + (size_t)v * k;
  if (l < k) {
    eo[l] = lo ? key_entity(lo) : -1;
    so[l] = lo ? key_score(lo) : -INFINITY;
  }
  if (64 + l < k) {
    eo[64 + l] = hi ? key_entity(hi) : -1;
    so[64 + l] = hi ? key_score(hi) : -INFINITY;
  }
}

// query block, entity slices: enough workgroups to fill the chip (as
// skge_rank_known sizes its counting pass)
struct TopkPlan {
  int qb_size, qb, eslice, ns;
};
int topk_block_size(int k) { return k <= 32 ? 64 : 32; }
// n_pools >= 0: the gathered selection, whose query blocks are the grouped
// work list's items (their bound; a pool has at most N entries)
static TopkPlan topk_plan(int nq, int k, int N, int n_pools = -1) {
  TopkPlan p;
  p.qb_size = topk_block_size(k);
  p.qb = n_pools >= 0 ? pool_items_max(nq, n_pools, p.qb_size) : (nq + p.qb_size - 1) / p.qb_size;
  const int tiles = (N + TK_EB - 1) / TK_EB;
  const int want = std::max(1, std::min(tiles, (2048 + p.qb - 1) / std::max(1, p.qb)));
  const int per = (tiles + want - 1) / want;
  p.eslice = per * TK_EB;
  p.ns = (tiles + per - 1) / per;
  return p;
}
static size_t topk_q_bytes(int nq, int d) {
  return (((size_t)nq * d * sizeof(float)) + 255) & ~(size_t)255;
}

template <int FORM>
static void launch_select(hipStream_t st, const TopkPlan& p, const TopkArgs& a, bool gather) {
  const dim3 grid(p.qb, p.ns);
  if (gather) {
    if (p.qb_size == 64)
      hipLaunchKernelGGL((k_topk_select<FORM, 64, 32, true>), grid, dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL((k_topk_select<FORM, 32, TK_KMAX, true>), grid, dim3(256), 0, st, a);
  } else if (p.qb_size == 64) {
    hipLaunchKernelGGL((k_topk_select<FORM, 64, 32>), grid, dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((k_topk_select<FORM, 32, TK_KMAX>), grid, dim3(256), 0, st, a);
  }
}

// the selection and the merge over any table T [rows][d] for query vectors
// Q [nq][d] (skge_host.h): model picks the score's form as skge_topk does
size_t topk_lists_bytes(int nq, int k, int rows, int n_pools) {
  const TopkPlan p = topk_plan(nq, k, rows, n_pools);
  return (size_t)nq * p.ns * k * sizeof(tkey_t);
}
void launch_topk_select(hipStream_t st, int model, const float* T, int rows, int d, const float* Q,
                        int nq, int k, const int* excl_off, const int* excl_ent, void* lists,
                        int* ent_out, float* score_out, const PoolWork* pools, int n_pools) {
  const bool gather = pools != nullptr;
  const TopkPlan p = topk_plan(nq, k, rows, gather ? n_pools : -1);
  TopkArgs a = {};
  a.E = T;
  a.N = rows;
  a.d = d;
  a.model = model;
  a.nq = nq;
  a.k = k;
  a.excl_off = excl_off;
  a.excl_ent = excl_ent;
  a.Q = const_cast<float*>(Q);
  a.lists = (tkey_t*)lists;
  a.eslice = p.eslice;
  a.ns = p.ns;
  a.ent_out = ent_out;
  a.score_out = score_out;
  if (gather) {
    a.pw = *pools;
    a.pw.ns = p.ns;
  }
  if (model == SKGE_TRANSE_L1)
    launch_select<TK_L1>(st, p, a, gather);
  else if (model == SKGE_TRANSE_L2)
    launch_select<TK_L2SQ>(st, p, a, gather);
  else
    launch_select<TK_DOT>(st, p, a, gather);
  hipLaunchKernelGGL(k_topk_merge, dim3((nq + 3) / 4), dim3(256), 0, st, a);
}

// the query vectors of nq queries (anchor, p) of one direction into Q [nq][d]
void launch_topk_query(hipStream_t st, int model, const float* E, const float* R, int d,
                       const int* queries, int nq, int direction, float* Q) {
  TopkArgs a = {};
  a.E = E;
  a.R = R;
  a.d = d;
  a.model = model;
  a.nq = nq;
  a.direction = direction;
  a.queries = queries;
  a.Q = Q;
  const int qblocks = std::max(1, std::min((nq + 1) / 2, 16384));
  hipLaunchKernelGGL(k_topk_query, dim3(qblocks), dim3(128), 0, st, a);
}

}  // namespace skge

using namespace skge;

extern "C" size_t skge_topk_workspace_bytes(int nq, int d, int k, int N) {
  if (nq <= 0 || d <= 0 || k < 1 || k > TK_KMAX || N <= 0) return 0;
  return topk_q_bytes(nq, d) + topk_lists_bytes(nq, k, N) + 256;
}

extern "C" int skge_topk(void* stream, int model, const float* E, const float* R, int N, int d,
                         const int* queries, int nq, int direction, int k, const int* excl_off,
                         const int* excl_ent, void* workspace, size_t ws_bytes, int* ent_out,
                         float* score_out) {
  SKGE_CHECK_ARG(E && R && queries && ent_out && score_out, "NULL argument");
  SKGE_CHECK_ARG(!excl_off || excl_ent, "NULL argument (excl_ent with excl_off given)");
  SKGE_CHECK_ARG(model >= 0 && model <= 3, "unknown model %d", model);
  SKGE_CHECK_ARG(direction == 0 || direction == 1, "direction must be 0 (tail) or 1 (head)");
  SKGE_CHECK_ARG(N > 0 && d > 0 && d <= 1024 && nq >= 0, "bad sizes (d <= 1024)");
  SKGE_CHECK_ARG(k >= 1 && k <= TK_KMAX, "k = %d outside 1 .. %d", k, TK_KMAX);
  if (nq == 0) return SKGE_OK;
  SKGE_CHECK_ARG(workspace && ws_bytes >= skge_topk_workspace_bytes(nq, d, k, N),
                 "top-k workspace needs %zu bytes", skge_topk_workspace_bytes(nq, d, k, N));
  float* Q = (float*)workspace;
  hipStream_t st = as_stream(stream);
  launch_topk_query(st, model, E, R, d, queries, nq, direction, Q);
  launch_topk_select(st, model, E, N, d, Q, nq, k, excl_off, excl_ent,
                     (char*)workspace + topk_q_bytes(nq, d), ent_out, score_out);
  SKGE_CHECK_LAUNCH("top-k");
  return SKGE_OK;
}
