// Relation prediction on the device: the position of the true relation of
// (s, ?, o) among all M relations (skge_relrank) and the k relations that best
// connect a pair (s, o) (skge_reltopk).  DESIGN.md 3.8.
//
// TransE and HolE score every relation as a distance to, or a dot product with,
// ONE vector per pair, so the relation table takes the entity table's place in
// the evaluator's and the top-k's passes:
//   TransE  -sum|q - R_j|   q = E_o - E_s         (top-k, TRANSE_L2: -sum (q - R_j)^2)
//   HolE    R_j . q         q = ccorr(E_s, E_o)
//   k_rel_query      one wave per pair: q and, for ranks, the true relation's
//                    score by rank_score (the counting pass's chain)
//   then launch_rank_count + k_rel_known, or launch_topk_select, over R.
// RESCAL's E_s W_j E_o has no such vector:
//   k_rel_rescal     workgroup = QB pairs x a few relations: the MFMA score
//                    tile (skge_rescal_tile.h) once per relation; one fp32 per
//                    (pair, relation) into a score matrix [nq][M]
//   k_rel_rank_rows  one wave per pair: relations strictly above sc[q][p], less
//                    the known ones above it
//   k_rel_topk_rows  one wave per pair: the row offered to a register key list
// The true relation's score is read from the matrix like any other, so an
// exact tie is an exact tie.  No float atomics: the same bits on every run.
#include <algorithm>
#include <stdlib.h>

#include "skge_elem.h"
#include "skge_host.h"
#include "skge_rescal_tile.h"
#include "skge_topk_list.h"

namespace skge {

// ---- TransE / HolE: the pair's query vector, one wave per pair ----
struct RelQueryArgs {
  const float* E;
  const float* R;       // [M][d]
  int d, model, nq;
  const int* queries;   // [nq][stride]: (s, o) or (s, o, p)
  int stride;
  float* Q;             // [nq][d]
  float* tgt;           // [nq] the true relation's score, or nullptr (needs stride 3)
};

__global__ __launch_bounds__(128) void k_rel_query(RelQueryArgs a) {
  const int wpb = blockDim.x >> 6, l = lane_id(), d = a.d;
  extern __shared__ float sm[];
  float* es = sm + (threadIdx.x >> 6) * 4 * d;   // E_s, E_o, q, R_p
  float* eo = es + d;
  float* lq = eo + d;
  float* rp = lq + d;
  const bool dist = a.model == SKGE_TRANSE_L1 || a.model == SKGE_TRANSE_L2;
  for (int i = blockIdx.x * wpb + (threadIdx.x >> 6); i < a.nq; i += gridDim.x * wpb) {
    const int s = __builtin_amdgcn_readfirstlane(a.queries[(size_t)a.stride * i]);
    const int o = __builtin_amdgcn_readfirstlane(a.queries[(size_t)a.stride * i + 1]);
    const int p = a.tgt ? __builtin_amdgcn_readfirstlane(a.queries[(size_t)a.stride * i + 2]) : 0;
    for (int k = l; k < d; k += 64) {
      es[k] = a.E[(size_t)s * d + k];
      eo[k] = a.E[(size_t)o * d + k];
      if (a.tgt) rp[k] = a.R[(size_t)p * d + k];
    }
    __builtin_amdgcn_wave_barrier();
    float* q = a.Q + (size_t)i * d;
    for (int k = l; k < d; k += 64) {
      // E_o - E_s or ccorr(E_s, E_o): query_elem's subject-side forms with E_o
      // for the anchor and E_s for the relation row
      const float v = query_elem(a.model, false, eo, es, nullptr, d, k);
      q[k] = v;
      lq[k] = v;
    }
    __builtin_amdgcn_wave_barrier();
    if (a.tgt && l == 0) a.tgt[i] = dist ? rank_score<true>(lq, rp, d) : rank_score<false>(lq, rp, d);
    __builtin_amdgcn_wave_barrier();
  }
}

// filtered correction + the ranks: one thread per pair, its other known
// relations scored with the counting pass's arithmetic (k_rank_known's form)
template <bool L1>
__global__ __launch_bounds__(256) void k_rel_known(const float* __restrict__ R, int d, int nq,
                                                   const float* __restrict__ Q,
                                                   const float* __restrict__ tgt,
                                                   const int* __restrict__ raw,
                                                   const int* __restrict__ known_off,
                                                   const int* __restrict__ known_rel,
                                                   int* __restrict__ ranks) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nq) return;
  int dec = 0;
  if (known_off) {
    const float* q = Q + (size_t)v * d;
    const float t = tgt[v];
    for (int i = known_off[v]; i < known_off[v + 1]; ++i)
      if (rank_score<L1>(q, R + (size_t)known_rel[i] * d, d) > t) ++dec;
  }
  ranks[2 * v] = 1 + raw[v];
  ranks[2 * v + 1] = 1 + raw[v] - dec;
}

// ---- RESCAL: the score matrix ----
struct RelRescalArgs {
  const float* E;
  const float* W;       // [M][d][d]
  int d, M, nq;
  const int* queries;   // [nq][stride]: (s, o, ...)
  int stride;
  int rper;             // relations per workgroup (blockIdx.y)
  float* S;             // [nq][M]
};

// workgroup = QB pairs x relations j0 .. j1 - 1, the score tile
// (skge_rescal_tile.h) once per relation.  LDS: the tile's + 2.5 KB.
template <int QB>
__global__ __launch_bounds__(256, 2) void k_rel_rescal(RelRescalArgs a) {
  constexpr int MI = QB / 32;
  __shared__ int s_s[QB], s_o[QB];
  __shared__ float s_red[4][QB];
  const int tid = threadIdx.x, d = a.d;
  const int v0 = blockIdx.x * QB;
  for (int i = tid; i < QB; i += 256) {
    const int v = v0 + i;
    const bool ok = v < a.nq;   // a row past the end reads entity 0 and is never written
    s_s[i] = ok ? a.queries[(size_t)a.stride * v] : 0;
    s_o[i] = ok ? a.queries[(size_t)a.stride * v + 1] : 0;
  }
  __syncthreads();
  bool eok[MI];
#pragma unroll
  for (int u = 0; u < MI; ++u) eok[u] = v0 + (tid >> 3) + 32 * u < a.nq;
  const int j0 = blockIdx.y * a.rper;
  const int j1 = a.M - j0 < a.rper ? a.M : j0 + a.rper;
  for (int j = j0; j < j1; ++j) {
    rescal_score_tile<QB>(a.E, a.W + (size_t)j * d * d, d, s_s, s_o, eok, s_red);
    if (tid < QB && v0 + tid < a.nq)
      a.S[(size_t)(v0 + tid) * a.M + j] = rescal_row_sum<QB>(s_red, tid);
  }
}

// ranks from the matrix: one wave per pair
__global__ __launch_bounds__(256) void k_rel_rank_rows(const float* __restrict__ S, int M, int nq,
                                                       const int* __restrict__ queries,
                                                       const int* __restrict__ known_off,
                                                       const int* __restrict__ known_rel,
                                                       int* __restrict__ ranks) {
  const int l = lane_id();
  const int v = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (v >= nq) return;
  const float* row = S + (size_t)v * M;
  const float t = row[queries[3 * (size_t)v + 2]];
  int raw = 0, dec = 0;
  for (int j = l; j < M; j += 64) raw += row[j] > t;
  if (known_off)
    for (int i = known_off[v] + l; i < known_off[v + 1]; i += 64) dec += row[known_rel[i]] > t;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    raw += __shfl_xor(raw, off);
    dec += __shfl_xor(dec, off);
  }
  if (l == 0) {
    ranks[2 * v] = 1 + raw;
    ranks[2 * v + 1] = 1 + raw - dec;
  }
}

// top-k from the matrix: one wave per pair, the list in its registers
__global__ __launch_bounds__(256) void k_rel_topk_rows(const float* __restrict__ S, int M, int nq,
                                                       int k, const int* __restrict__ excl_off,
                                                       const int* __restrict__ excl_rel,
                                                       int* __restrict__ rel_out,
                                                       float* __restrict__ score_out) {
  const int l = lane_id();
  const int v = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (v >= nq) return;
  const float* row = S + (size_t)v * M;
  tkey_t lo = 0, hi = 0, thr = 0;
  const int* xb = excl_off ? excl_rel + excl_off[v] : nullptr;
  const int* xe = excl_off ? excl_rel + excl_off[v + 1] : nullptr;
  for (int j0 = 0; j0 < M; j0 += 64) {   // wave-uniform
    const int j = j0 + l;
    const tkey_t c = j < M ? make_key(row[j], j) : 0;
    if (excl_off)
      list_offer<true>(lo, hi, thr, c, k, l, xb, xe);
    else
      list_offer<false>(lo, hi, thr, c, k, l, nullptr, nullptr);
  }
  list_decode_store(lo, hi, k, l, rel_out + (size_t)v * k, score_out + (size_t)v * k);
}

// RESCAL: pairs per pass of the entry points, so that the score matrix stays
// within REL_SCORE_BYTES (SKGE_REL_SCORE_BYTES overrides it: the tests run a
// case in several passes)
constexpr size_t REL_SCORE_BYTES = (size_t)256 << 20;
static int rel_chunk(int nq, int M) {
  size_t cap = REL_SCORE_BYTES;
  if (const char* e = getenv("SKGE_REL_SCORE_BYTES")) {
    const long long v = atoll(e);
    if (v > 0) cap = (size_t)v;
  }
  const size_t per = (size_t)M * sizeof(float);
  const size_t rows = std::max<size_t>(128, (cap / per) & ~(size_t)127);
  return (int)std::min<size_t>((size_t)nq, rows);
}

static void launch_rel_rescal(hipStream_t st, const float* E, const float* W, int M, int d,
                              const int* queries, int stride, int nq, float* S) {
  RelRescalArgs a;
  a.E = E;
  a.W = W;
  a.d = d;
  a.M = M;
  a.nq = nq;
  a.queries = queries;
  a.stride = stride;
  a.S = S;
  // query blocks x relation groups (slice_plan over the M relations)
  const int qb_size = nq <= 32 ? 32 : nq <= 64 ? 64 : 128;
  const int qb = (nq + qb_size - 1) / qb_size;
  const SlicePlan sp = slice_plan(qb, M);
  a.rper = sp.per;
  const int groups = sp.ns;
  if (qb_size == 32)
    hipLaunchKernelGGL((k_rel_rescal<32>), dim3(qb, groups), dim3(256), 0, st, a);
  else if (qb_size == 64)
    hipLaunchKernelGGL((k_rel_rescal<64>), dim3(qb, groups), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((k_rel_rescal<128>), dim3(qb, groups), dim3(256), 0, st, a);
}

static void launch_rel_query(hipStream_t st, int model, const float* E, const float* R, int d,
                             const int* queries, int stride, int nq, float* Q, float* tgt) {
  RelQueryArgs a;
  a.E = E;
  a.R = R;
  a.d = d;
  a.model = model;
  a.nq = nq;
  a.queries = queries;
  a.stride = stride;
  a.Q = Q;
  a.tgt = tgt;
  const int qblocks = std::max(1, std::min((nq + 1) / 2, 16384));
  hipLaunchKernelGGL(k_rel_query, dim3(qblocks), dim3(128), (size_t)2 * 4 * d * sizeof(float), st,
                     a);
}

}  // namespace skge

using namespace skge;

extern "C" size_t skge_relrank_workspace_bytes(int nq, int d, int M, int model) {
  if (nq <= 0 || d <= 0 || M <= 0) return 0;
  if (model == SKGE_RESCAL) return (size_t)rel_chunk(nq, M) * M * sizeof(float) + 256;
  return align256((size_t)nq * d * sizeof(float)) +
         (size_t)nq * (sizeof(float) + sizeof(int)) + 512;
}

extern "C" int skge_relrank(void* stream, int model, const float* E, const float* R, int N, int M,
                            int d, const int* queries, int nq, const int* known_off,
                            const int* known_rel, void* workspace, size_t ws_bytes,
                            int* ranks_out) {
  SKGE_CHECK_ARG(E && R && queries && ranks_out, "NULL argument");
  SKGE_CHECK_ARG(!known_off || known_rel, "NULL argument (known_rel with known_off given)");
  SKGE_CHECK_MODEL(model, d);
  // |s * r_j - o| has no single query vector against the relation table
  SKGE_REFUSE_ROTATE(model, "relation prediction");
  SKGE_CHECK_ARG(N > 0 && M >= 1 && d > 0 && d <= 1024 && nq >= 0,
                 "bad sizes (N = %d, M = %d, d = %d <= 1024, nq = %d)", N, M, d, nq);
  if (nq == 0) return SKGE_OK;
  const size_t need = skge_relrank_workspace_bytes(nq, d, M, model);
  SKGE_CHECK_ARG(workspace && ws_bytes >= need, "relation rank workspace needs %zu bytes", need);
  hipStream_t st = as_stream(stream);
  if (model == SKGE_RESCAL) {
    float* S = (float*)workspace;
    const int chunk = rel_chunk(nq, M);
    for (int q0 = 0; q0 < nq; q0 += chunk) {
      const int n = std::min(chunk, nq - q0);
      const int* q = queries + (size_t)3 * q0;
      launch_rel_rescal(st, E, R, M, d, q, 3, n, S);
      hipLaunchKernelGGL(k_rel_rank_rows, dim3((n + 3) / 4), dim3(256), 0, st, S, M, n, q,
                         known_off ? known_off + q0 : nullptr, known_rel, ranks_out + (size_t)2 * q0);
    }
    SKGE_CHECK_LAUNCH("relation rank (RESCAL)");
    return SKGE_OK;
  }
  float* Q = (float*)workspace;
  float* tgt = (float*)((char*)workspace + align256((size_t)nq * d * sizeof(float)));
  int* raw = (int*)(tgt + nq);
  SKGE_CHECK_HIP(hipMemsetAsync(raw, 0, (size_t)nq * sizeof(int), st));
  launch_rel_query(st, model, E, R, d, queries, 3, nq, Q, tgt);
  const bool l1 = model == SKGE_TRANSE_L1 || model == SKGE_TRANSE_L2;
  launch_rank_count(st, l1, R, M, d, Q, tgt, nq, raw);
  const int kb = (nq + 255) / 256;
  if (l1)
    hipLaunchKernelGGL((k_rel_known<true>), dim3(kb), dim3(256), 0, st, R, d, nq, Q, tgt, raw,
                       known_off, known_rel, ranks_out);
  else
    hipLaunchKernelGGL((k_rel_known<false>), dim3(kb), dim3(256), 0, st, R, d, nq, Q, tgt, raw,
                       known_off, known_rel, ranks_out);
  SKGE_CHECK_LAUNCH("relation rank");
  return SKGE_OK;
}

extern "C" size_t skge_reltopk_workspace_bytes(int nq, int d, int k, int M, int model) {
  if (nq <= 0 || d <= 0 || k < 1 || k > TK_KMAX || M <= 0) return 0;
  if (model == SKGE_RESCAL) return (size_t)rel_chunk(nq, M) * M * sizeof(float) + 256;
  return align256((size_t)nq * d * sizeof(float)) + topk_lists_bytes(nq, k, M) + 256;
}

extern "C" int skge_reltopk(void* stream, int model, const float* E, const float* R, int N, int M,
                            int d, const int* pairs, int nq, int k, const int* excl_off,
                            const int* excl_rel, void* workspace, size_t ws_bytes, int* rel_out,
                            float* score_out) {
  SKGE_CHECK_ARG(E && R && pairs && rel_out && score_out, "NULL argument");
  SKGE_CHECK_ARG(!excl_off || excl_rel, "NULL argument (excl_rel with excl_off given)");
  SKGE_CHECK_MODEL(model, d);
  // |s * r_j - o| has no single query vector against the relation table
  SKGE_REFUSE_ROTATE(model, "relation prediction");
  SKGE_CHECK_ARG(N > 0 && M >= 1 && d > 0 && d <= 1024 && nq >= 0,
                 "bad sizes (N = %d, M = %d, d = %d <= 1024, nq = %d)", N, M, d, nq);
  SKGE_CHECK_ARG(k >= 1 && k <= TK_KMAX, "k = %d outside 1 .. %d", k, TK_KMAX);
  if (nq == 0) return SKGE_OK;
  const size_t need = skge_reltopk_workspace_bytes(nq, d, k, M, model);
  SKGE_CHECK_ARG(workspace && ws_bytes >= need, "relation top-k workspace needs %zu bytes", need);
  hipStream_t st = as_stream(stream);
  if (model == SKGE_RESCAL) {
    float* S = (float*)workspace;
    const int chunk = rel_chunk(nq, M);
    for (int q0 = 0; q0 < nq; q0 += chunk) {
      const int n = std::min(chunk, nq - q0);
      launch_rel_rescal(st, E, R, M, d, pairs + (size_t)2 * q0, 2, n, S);
      hipLaunchKernelGGL(k_rel_topk_rows, dim3((n + 3) / 4), dim3(256), 0, st, S, M, n, k,
                         excl_off ? excl_off + q0 : nullptr, excl_rel, rel_out + (size_t)k * q0,
                         score_out + (size_t)k * q0);
    }
    SKGE_CHECK_LAUNCH("relation top-k (RESCAL)");
    return SKGE_OK;
  }
  float* Q = (float*)workspace;
  launch_rel_query(st, model, E, R, d, pairs, 2, nq, Q, nullptr);
  launch_topk_select(st, model, R, M, d, Q, nq, k, excl_off, excl_rel,
                     (char*)workspace + align256((size_t)nq * d * sizeof(float)), rel_out,
                     score_out);
  SKGE_CHECK_LAUNCH("relation top-k");
  return SKGE_OK;
}
