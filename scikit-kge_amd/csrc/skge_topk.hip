// Top-k link prediction on the device: the k best tails of (a, p, ?) or heads
// of (?, p, a) for a batch of queries.
//
// Every model's score of entity j under a query is a distance to, or a dot
// product with, one query vector (skge_eval.hip header): the vectors are
// query_elem's (skge_elem.h), the scores the score tile's (skge_rank_tile.h),
// the counting pass's own.  New here only: SKGE_TRANSE_L2 scores
// -sum (q - E_j)^2, the model's training score (the ranking entry points score
// both TransE codes as L1).
//   k_topk_query    one wave per query: the query vector of the asked direction
//   k_topk_select   workgroup = a block of query vectors x one entity slice;
//                   after each score tile every wave offers the tile's scores
//                   to its queries' sorted lists
//   k_list_merge    one wave per query: the slices' lists into the final k
//                   (skge_neighbours.hip's merge too)
// The lists are 64-bit keys in one compare order: skge_topk_list.h.
// k_topk_select<.., GATHER> is the same selection over candidate pools: query
// blocks from a grouped work list, rows through an index (skge_pools.h;
// skge_topk_pools, skge_pools.hip).
#include <algorithm>
#include <type_traits>

#include "skge_elem.h"
#include "skge_host.h"
#include "skge_pools.h"
#include "skge_topk_list.h"

namespace skge {

struct TopkArgs {
  const float* E;
  const float* R;        // TransE / HolE: [M][d]; RESCAL: W [M][d][d]
  int N, d, model, nq, direction, k;
  const int* queries;    // [nq][2] (anchor, p)
  const int* excl_off;   // [nq + 1] or nullptr
  const int* excl_ent;
  float* Q;              // workspace [nq][d]
  tkey_t* lists;         // workspace [nq][ns][k]
  int eslice, ns;        // entities per slice (multiple of RT_EB), slices
  PoolWork pw;           // the gathered selection's work list (k_topk_select<.., true>)
};

// ---- query vectors: one wave per query (query_elem, skge_elem.h) ----
__global__ __launch_bounds__(128) void k_topk_query(TopkArgs a) {
  __shared__ float sm[2][2 * 1024];
  const int wpb = blockDim.x >> 6, l = lane_id(), d = a.d;
  float* ea = sm[threadIdx.x >> 6];   // the anchor's row
  float* rp = ea + 1024;
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
    for (int k = l; k < d; k += 64) q[k] = query_elem(a.model, tail, ea, rp, W, d, k);
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- selection: QB query vectors x one entity slice per workgroup ----
// After a score tile (skge_rank_tile.h; thread: 8 entities x QB / 16 queries)
// the scores go to LDS (over the staging buffers) query-major, and wave w
// offers them to queries w, w + 4, ...: a query's list sits in LDS between
// tiles and in the wave's registers while one of the tile's scores beats its
// k-th entry.
// LDS: max(staging, scores) + lists = 33.0 + 16 KB (QB 64, k <= 32),
// 21.0 + 32 KB (QB 32, k <= 128).
// GATHER (skge_pools.h): the workgroup's queries are item blockIdx.x of the
// grouped work list, reached through its order array, and the candidate rows
// are its pool's entries (RankPoolRows; + 0.5 KB of LDS for a tile's row
// ids); blockIdx.y is a slice of that pool.
template <int FORM, int QB, int KCAP, bool GATHER = false>
__global__ __launch_bounds__(256) void k_topk_select(TopkArgs a) {
  constexpr int PADQ = QB + 4;
  constexpr int TQ = QB / 16;               // queries per thread
  constexpr int STAGE = RT_KC * (PADQ + RT_PADE);
  constexpr int SCORES = QB * RT_PADE;
  __shared__ __attribute__((aligned(16))) float s_buf[STAGE > SCORES ? STAGE : SCORES];
  __shared__ tkey_t s_list[QB][KCAP];
  __shared__ int s_rid[GATHER ? RT_EB : 1];
  float (*sQ)[PADQ] = reinterpret_cast<float (*)[PADQ]>(s_buf);
  float (*sE)[RT_PADE] = reinterpret_cast<float (*)[RT_PADE]>(s_buf + RT_KC * PADQ);
  float (*sS)[RT_PADE] = reinterpret_cast<float (*)[RT_PADE]>(s_buf);
  const int tid = threadIdx.x, k = a.k;
  const int l = tid & 63, w = tid >> 6;
  std::conditional_t<GATHER, RankPoolRows, RankRows> m;   // the block's vectors and rows
  int ebeg, eend;
  if constexpr (GATHER) {
    if ((int)blockIdx.x >= *a.pw.n_items) return;
    const int4 it = a.pw.items[blockIdx.x];
    int64_t base;
    pool_slice(pool_size(a.pw, it.x, a.N, base), a.pw.ns, blockIdx.y, ebeg, eend);
    m = {a.pw.order + it.y, it.z, it.x >= 0 ? a.pw.pool_ent + base : nullptr, nullptr};
  } else {
    ebeg = blockIdx.y * a.eslice;
    eend = a.N - ebeg < a.eslice ? a.N : ebeg + a.eslice;
    m = {(int)blockIdx.x * QB, a.nq};
  }
  for (int i = tid; i < QB * KCAP; i += 256) (&s_list[0][0])[i] = 0;
  __syncthreads();
  const int te = (tid & 15) * 8, tq = (tid >> 4) * TQ;
  for (int e0 = ebeg; e0 < eend; e0 += RT_EB) {
    float acc[8][TQ];
    score_tile<FORM, QB>(a.E, a.d, a.Q, e0, eend, m, sQ, sE, acc);
    __syncthreads();   // the staging buffers' reads are done: the scores go over them
#pragma unroll
    for (int y = 0; y < TQ; ++y) {
      *reinterpret_cast<float4*>(&sS[tq + y][te]) =
          make_float4(acc[0][y], acc[1][y], acc[2][y], acc[3][y]);
      *reinterpret_cast<float4*>(&sS[tq + y][te + 4]) =
          make_float4(acc[4][y], acc[5][y], acc[6][y], acc[7][y]);
    }
    if constexpr (GATHER) {
      if (tid < RT_EB) s_rid[tid] = e0 + tid < eend ? m.row(e0 + tid) : -1;
    }
    __syncthreads();
    for (int qq = w; qq < QB; qq += 4) {   // wave-uniform
      const int v = m.vec(qq);
      if (v < 0) break;
      const int ea0 = e0 + l, ea1 = e0 + 64 + l;
      const tkey_t c0 = ea0 < eend ? make_key(sS[qq][l], GATHER ? s_rid[l] : ea0) : 0;
      const tkey_t c1 = ea1 < eend ? make_key(sS[qq][64 + l], GATHER ? s_rid[64 + l] : ea1) : 0;
      list_offer2(s_list[qq], c0, c1, k, l, a.excl_off, a.excl_ent, v);
    }
  }
  // this (query, slice)'s list: each wave writes the queries it owns
  __builtin_amdgcn_wave_barrier();
  for (int qq = w; qq < QB; qq += 4) {
    const int v = m.vec(qq);
    if (v < 0) break;
    list_store(a.lists + ((size_t)v * a.ns + blockIdx.y) * k, s_list[qq], k, l);
  }
}

// ---- merge: one wave per query, the slices' lists into the final k ----
__global__ __launch_bounds__(256) void k_list_merge(const tkey_t* __restrict__ lists, int nq, int ns,
                                                    int k, int* __restrict__ ids_out,
                                                    float* __restrict__ score_out) {
  const int l = lane_id();
  const int v = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (v >= nq) return;
  tkey_t lo = 0, hi = 0, thr = 0;
  for (int s = 0; s < ns; ++s) {
    const tkey_t* in = lists + ((size_t)v * ns + s) * k;
    const tkey_t c0 = l < k ? in[l] : 0;
    const tkey_t c1 = 64 + l < k ? in[64 + l] : 0;
    list_offer<false>(lo, hi, thr, c0, k, l, nullptr, nullptr);
    list_offer<false>(lo, hi, thr, c1, k, l, nullptr, nullptr);
  }
  list_decode_store(lo, hi, k, l, ids_out + (size_t)v * k, score_out + (size_t)v * k);
}
void launch_list_merge(hipStream_t st, const void* lists, int nq, int ns, int k, int* ids_out,
                       float* score_out) {
  hipLaunchKernelGGL(k_list_merge, dim3((nq + 3) / 4), dim3(256), 0, st, (const tkey_t*)lists, nq,
                     ns, k, ids_out, score_out);
}

// query block, entity slices (slice_plan, as skge_rank_known's counting pass)
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
  const SlicePlan sp = slice_plan(p.qb, (N + RT_EB - 1) / RT_EB);
  p.eslice = sp.per * RT_EB;
  p.ns = sp.ns;
  return p;
}
static size_t topk_q_bytes(int nq, int d) { return align256((size_t)nq * d * sizeof(float)); }

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
  if (gather) {
    a.pw = *pools;
    a.pw.ns = p.ns;
  }
  if (model == SKGE_TRANSE_L1)
    launch_select<RT_L1>(st, p, a, gather);
  else if (model == SKGE_TRANSE_L2)
    launch_select<RT_L2SQ>(st, p, a, gather);
  else if (model == SKGE_ROTATE)
    launch_select<RT_CMOD>(st, p, a, gather);
  else
    launch_select<RT_DOT>(st, p, a, gather);
  launch_list_merge(st, lists, nq, p.ns, k, ent_out, score_out);
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
  SKGE_CHECK_MODEL(model, d);
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
