// Type-constrained ranking: filtered ranks and top-k over candidate pools
// (SURVEY.md 8(f) row 9).
//
// skge_rank_known and skge_topk score every entity; here each query vector
// names a POOL of candidates (a CSR of ascending entity ids, DeviceKG.pools'
// layout; -1 = every entity), the protocol that matches training with typed
// negatives.  The query vectors, the true entities' scores and the score
// arithmetic are the all-entity entry points' (launch_rank_query,
// launch_topk_query, rank_score's sequential fp32 chain).  New here:
//   k_pool_hist / k_pool_scan / k_pool_scatter
//                      group the vectors by pool id on the device -- the host
//                      knows only the counts -- into a work list of items,
//                      one block of up to 64 (or 32) vectors of one pool
//                      (skge_pools.h)
//   k_rank_count_pool  the counting tile (skge_rank_tile.h) over one item x one
//                      slice of its pool: Q rows through the order array,
//                      candidate rows through pool_ent
//   k_rank_known_pool  k_rank_known with a membership search: a known answer
//                      outside the vector's pool was never counted, so it is
//                      not subtracted
// and the gathered instantiation of k_topk_select (skge_topk.hip).
#include <algorithm>

#include "skge_host.h"
#include "skge_pools.h"
#include "skge_topk_list.h"

namespace skge {

// ---- grouping ----
// bins[b] for pool b - 1 (bin 0: pool -1), bins[nbins] = the item count
__global__ __launch_bounds__(256) void k_pool_hist(const int* __restrict__ vec_pool, int nv,
                                                   int* __restrict__ bins) {
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += gridDim.x * blockDim.x)
    atomicAdd(&bins[vec_pool[v] + 1], 1);
}

// one workgroup: counts -> each bin's first slot of the order array (left in
// bins as the scatter's cursor) and its items; thread t owns a run of bins
__global__ __launch_bounds__(256) void k_pool_scan(int* __restrict__ bins, long long nbins, int bsz,
                                                   int4* __restrict__ items) {
  __shared__ int s_cnt[256], s_itm[256];
  const int tid = threadIdx.x;
  const long long per = (nbins + 255) / 256;
  const long long b0 = tid * per < nbins ? tid * per : nbins;
  const long long b1 = b0 + per < nbins ? b0 + per : nbins;
  int cnt = 0, itm = 0;
  for (long long b = b0; b < b1; ++b) {
    cnt += bins[b];
    itm += (bins[b] + bsz - 1) / bsz;
  }
  s_cnt[tid] = cnt;
  s_itm[tid] = itm;
  __syncthreads();
  if (tid == 0) {   // exclusive scan of the 256 run totals
    int c = 0, i = 0;
    for (int t = 0; t < 256; ++t) {
      const int tc = s_cnt[t], ti = s_itm[t];
      s_cnt[t] = c;
      s_itm[t] = i;
      c += tc;
      i += ti;
    }
    bins[nbins] = i;
  }
  __syncthreads();
  int slot = s_cnt[tid], it = s_itm[tid];
  for (long long b = b0; b < b1; ++b) {
    const int n = bins[b];
    bins[b] = slot;
    for (int j = 0; j < n; j += bsz)
      items[it++] = make_int4((int)b - 1, slot + j, min(bsz, n - j), 0);
    slot += n;
  }
}

__global__ __launch_bounds__(256) void k_pool_scatter(const int* __restrict__ vec_pool, int nv,
                                                      int* __restrict__ bins,
                                                      int* __restrict__ order) {
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += gridDim.x * blockDim.x)
    order[atomicAdd(&bins[vec_pool[v] + 1], 1)] = v;
}

// every bin with a vector holds at most one partial block
int pool_items_max(int nv, int n_pools, int bsz) {
  return (nv + bsz - 1) / bsz + (int)std::min<long long>(nv, (long long)n_pools + 1);
}
size_t pool_group_bytes(int nv, int n_pools, int bsz) {
  return align256(((size_t)n_pools + 2) * sizeof(int)) + align256((size_t)nv * sizeof(int)) +
         align256((size_t)pool_items_max(nv, n_pools, bsz) * sizeof(int4));
}
int launch_pool_group(hipStream_t st, const int* vec_pool, int nv, int n_pools, int bsz,
                      const int64_t* pool_off, const int* pool_ent, void* ws, PoolWork* w) {
  const long long nbins = (long long)n_pools + 1;
  int* bins = (int*)ws;
  int* order = (int*)((char*)ws + align256((size_t)(nbins + 1) * sizeof(int)));
  int4* items = (int4*)((char*)order + align256((size_t)nv * sizeof(int)));
  SKGE_CHECK_HIP(hipMemsetAsync(bins, 0, (size_t)(nbins + 1) * sizeof(int), st));
  const int blocks = std::max(1, std::min((nv + 255) / 256, 2048));
  hipLaunchKernelGGL(k_pool_hist, dim3(blocks), dim3(256), 0, st, vec_pool, nv, bins);
  hipLaunchKernelGGL(k_pool_scan, dim3(1), dim3(256), 0, st, bins, nbins, bsz, items);
  hipLaunchKernelGGL(k_pool_scatter, dim3(blocks), dim3(256), 0, st, vec_pool, nv, bins, order);
  w->items = items;
  w->n_items = bins + nbins;
  w->order = order;
  w->pool_off = pool_off;
  w->pool_ent = pool_ent;
  w->ns = 1;
  return SKGE_OK;
}

// ---- counting: one item (<= 64 vectors of one pool) x one slice of the pool ----
struct PoolRankArgs {
  const float* E;
  int N, d;
  const float* Q;      // [nv][d]
  const float* tgt;    // [nv]
  int* raw;            // [nv] candidates scoring strictly higher (atomics over the slices)
  PoolWork pw;
};

template <int FORM>
__global__ __launch_bounds__(256) void k_rank_count_pool(PoolRankArgs a) {
  __shared__ int s_vec[RT_QB];
  if ((int)blockIdx.x >= *a.pw.n_items) return;
  const int4 item = a.pw.items[blockIdx.x];
  const int pool = item.x, vbeg = item.y, vcnt = item.z;
  int64_t base;
  int ebeg, eend;
  pool_slice(pool_size(a.pw, pool, a.N, base), a.pw.ns, blockIdx.y, ebeg, eend);
  if (ebeg >= eend) return;
  const RankPoolRows m = {a.pw.order + vbeg, vcnt, pool >= 0 ? a.pw.pool_ent + base : nullptr,
                          s_vec};
  if (threadIdx.x < RT_QB) s_vec[threadIdx.x] = m.vec(threadIdx.x);
  rank_count_tile<FORM>(a.E, a.d, a.Q, a.tgt, a.raw, ebeg, eend, m);
}

// e is an entry of the ascending list p[0 .. n)
__device__ __forceinline__ bool pool_has(const int* __restrict__ p, int n, int e) {
  int lo = 0, hi = n;
  while (lo < hi) {   // lower bound
    const int mid = lo + ((hi - lo) >> 1);
    if (p[mid] < e) lo = mid + 1; else hi = mid;
  }
  return lo < n && p[lo] == e;
}

// filtered correction + the ranks: k_rank_known's form (one thread per query
// vector, its known answers scored with the counting pass's arithmetic); an
// answer counts only when the vector's pool holds it
template <int FORM>
__global__ __launch_bounds__(256) void k_rank_known_pool(
    const float* __restrict__ E, int d, int nq, const float* __restrict__ Q,
    const float* __restrict__ tgt, const int* __restrict__ raw, const int* __restrict__ vec_pool,
    const int64_t* __restrict__ pool_off, const int* __restrict__ pool_ent,
    const int* __restrict__ tail_off, const int* __restrict__ tail_ent,
    const int* __restrict__ head_off, const int* __restrict__ head_ent, int* __restrict__ ranks) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= 2 * nq) return;
  const int qi = v >> 1, dir = v & 1;   // 0: tail (vary o), 1: head (vary s)
  const int* off = dir ? head_off : tail_off;
  const int* ent = dir ? head_ent : tail_ent;
  const float* q = Q + (size_t)v * d;
  const float t = tgt[v];
  const int pool = vec_pool[v];
  const int* mem = nullptr;
  int nmem = 0;
  if (pool >= 0) {
    mem = pool_ent + pool_off[pool];
    nmem = (int)(pool_off[pool + 1] - pool_off[pool]);
  }
  int dec = 0;
  for (int i = off[qi]; i < off[qi + 1]; ++i) {
    const int e = ent[i];
    if (pool >= 0 && !pool_has(mem, nmem, e)) continue;
    if (rank_score_form<FORM>(q, E + (size_t)e * d, d) > t) ++dec;
  }
  ranks[4 * qi + 2 * dir] = 1 + raw[v];
  ranks[4 * qi + 2 * dir + 1] = 1 + raw[v] - dec;
}

}  // namespace skge

using namespace skge;

static bool pool_sizes_ok(int nq, int d, int n_pools) {
  return nq > 0 && d > 0 && n_pools >= 0;
}

extern "C" size_t skge_rank_pools_workspace_bytes(int nq, int d, int n_pools) {
  if (!pool_sizes_ok(nq, d, n_pools)) return 0;
  return align256((size_t)2 * nq * d * sizeof(float)) + 2 * align256((size_t)2 * nq * sizeof(float)) +
         pool_group_bytes(2 * nq, n_pools, RT_QB) + 256;
}

extern "C" int skge_rank_pools(void* stream, int model, const float* E, const float* R, int N,
                               int d, const int* queries, int nq, const int64_t* pool_off,
                               const int* pool_ent, int n_pools, const int* vec_pool,
                               const int* tail_off, const int* tail_ent, const int* head_off,
                               const int* head_ent, void* workspace, size_t ws_bytes,
                               int* ranks_out) {
  SKGE_CHECK_ARG(E && R && queries && ranks_out && vec_pool && tail_off && head_off,
                 "NULL argument");
  SKGE_CHECK_MODEL(model, d);
  SKGE_CHECK_ARG(N > 0 && d > 0 && d <= 1024 && nq >= 0, "bad sizes (d <= 1024)");
  SKGE_CHECK_ARG(n_pools >= 0, "n_pools = %d is negative", n_pools);
  SKGE_CHECK_ARG(n_pools == 0 || (pool_off && pool_ent), "NULL argument (%d pools, no pool arrays)",
                 n_pools);
  if (nq == 0) return SKGE_OK;
  SKGE_CHECK_ARG(workspace && ws_bytes >= skge_rank_pools_workspace_bytes(nq, d, n_pools),
                 "pool rank workspace needs %zu bytes",
                 skge_rank_pools_workspace_bytes(nq, d, n_pools));
  const int nv = 2 * nq;
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  float* Q = (float*)ws;
  float* tgt = (float*)(ws + align256((size_t)nv * d * sizeof(float)));
  int* raw = (int*)((char*)tgt + align256((size_t)nv * sizeof(float)));
  void* gws = (char*)raw + align256((size_t)nv * sizeof(int));
  hipStream_t st = as_stream(stream);
  SKGE_CHECK_HIP(hipMemsetAsync(raw, 0, (size_t)nv * sizeof(int), st));
  PoolRankArgs a;
  a.E = E;
  a.N = N;
  a.d = d;
  a.Q = Q;
  a.tgt = tgt;
  a.raw = raw;
  const int rc = launch_pool_group(st, vec_pool, nv, n_pools, RT_QB, pool_off, pool_ent, gws, &a.pw);
  if (rc != SKGE_OK) return rc;
  launch_rank_query(st, model, E, R, N, d, queries, nq, Q, tgt);
  const int form = rank_form(model);
  const int max_items = pool_items_max(nv, n_pools, RT_QB);
  // a pool has at most N candidates; one with fewer tiles than slices leaves
  // the others empty
  a.pw.ns = slice_plan(max_items, (N + RT_EB - 1) / RT_EB).ns;
  const dim3 grid(max_items, a.pw.ns);
  const int kb = (nv + 255) / 256;
#define SKGE_RP(F)                                                                              \
  do {                                                                                          \
    hipLaunchKernelGGL((k_rank_count_pool<F>), grid, dim3(256), 0, st, a);                      \
    hipLaunchKernelGGL((k_rank_known_pool<F>), dim3(kb), dim3(256), 0, st, E, d, nq, Q, tgt,    \
                       raw, vec_pool, pool_off, pool_ent, tail_off, tail_ent, head_off,         \
                       head_ent, ranks_out);                                                    \
  } while (0)
  if (form == RT_L1)
    SKGE_RP(RT_L1);
  else if (form == RT_CMOD)
    SKGE_RP(RT_CMOD);
  else
    SKGE_RP(RT_DOT);
#undef SKGE_RP
  SKGE_CHECK_LAUNCH("rank (pools)");
  return SKGE_OK;
}

extern "C" size_t skge_topk_pools_workspace_bytes(int nq, int d, int k, int N, int n_pools) {
  if (!pool_sizes_ok(nq, d, n_pools) || k < 1 || k > TK_KMAX || N <= 0) return 0;
  return align256((size_t)nq * d * sizeof(float)) + align256(topk_lists_bytes(nq, k, N, n_pools)) +
         pool_group_bytes(nq, n_pools, topk_block_size(k)) + 256;
}

extern "C" int skge_topk_pools(void* stream, int model, const float* E, const float* R, int N,
                               int d, const int* queries, int nq, int direction, int k,
                               const int64_t* pool_off, const int* pool_ent, int n_pools,
                               const int* query_pool, const int* excl_off, const int* excl_ent,
                               void* workspace, size_t ws_bytes, int* ent_out, float* score_out) {
  SKGE_CHECK_ARG(E && R && queries && query_pool && ent_out && score_out, "NULL argument");
  SKGE_CHECK_ARG(!excl_off || excl_ent, "NULL argument (excl_ent with excl_off given)");
  SKGE_CHECK_MODEL(model, d);
  SKGE_CHECK_ARG(direction == 0 || direction == 1, "direction must be 0 (tail) or 1 (head)");
  SKGE_CHECK_ARG(N > 0 && d > 0 && d <= 1024 && nq >= 0, "bad sizes (d <= 1024)");
  SKGE_CHECK_ARG(k >= 1 && k <= TK_KMAX, "k = %d outside 1 .. %d", k, TK_KMAX);
  SKGE_CHECK_ARG(n_pools >= 0, "n_pools = %d is negative", n_pools);
  SKGE_CHECK_ARG(n_pools == 0 || (pool_off && pool_ent), "NULL argument (%d pools, no pool arrays)",
                 n_pools);
  if (nq == 0) return SKGE_OK;
  SKGE_CHECK_ARG(workspace && ws_bytes >= skge_topk_pools_workspace_bytes(nq, d, k, N, n_pools),
                 "pool top-k workspace needs %zu bytes",
                 skge_topk_pools_workspace_bytes(nq, d, k, N, n_pools));
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  float* Q = (float*)ws;
  void* lists = ws + align256((size_t)nq * d * sizeof(float));
  void* gws = (char*)lists + align256(topk_lists_bytes(nq, k, N, n_pools));
  hipStream_t st = as_stream(stream);
  PoolWork pw;
  const int rc = launch_pool_group(st, query_pool, nq, n_pools, topk_block_size(k), pool_off,
                                   pool_ent, gws, &pw);
  if (rc != SKGE_OK) return rc;
  launch_topk_query(st, model, E, R, d, queries, nq, direction, Q);
  launch_topk_select(st, model, E, N, d, Q, nq, k, excl_off, excl_ent, lists, ent_out, score_out,
                     &pw, n_pools);
  SKGE_CHECK_LAUNCH("top-k (pools)");
  return SKGE_OK;
}
