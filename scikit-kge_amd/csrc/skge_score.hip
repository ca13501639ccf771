// Raw scores of explicit triples (skge_score; DESIGN.md 3.10, SURVEY.md 8(f)
// row 10): what LinkPredictionEval and triple classification read.  Plain
// table pointers, no accumulators, no table structs; every triple's score is
// the model's training score before the activation.
//   k_score_transe4   TransE, d % 4 == 0: one wave per triple, rows in the quad
//                     layout (load_row4, 16 B per lane); L1 through
//                     l1_scores_signs (skge_transe_l1.h, its sign outputs
//                     unused), L2 by transe_elem
//   k_score_transe    TransE, any d: lane-strided rows, transe_elem (skge_elem.h)
//   k_score_hole4     HolE, d % 4 == 0, d <= 256: A = ccorr(R_p, E_o) by
//                     corr_quad, then hole_score_q(E_s, A) (skge_hole.h)
//   k_score_hole      HolE, any d: ccorr_direct_k (skge_elem.h, k_rel_query's),
//                     folded with R_p per lane, then the wave sum
//   k_score_diag      DistMult / ComplEx: E_s . (conj(R_p) * E_o) on rows in
//                     registers (skge_diag.h), the step kernels' expression
//   k_score_rot       RotatE: -sum_j |E_s[j] * R_p[j] - E_o[j]| on rows in
//                     registers (skge_rot.h), the step kernels' expression
//   k_score_rescal    RESCAL: the triples are grouped by relation on the device
//                     (launch_pool_group: histogram, scan, scatter); an item is
//                     up to QB triples of ONE relation, scored by the MFMA
//                     score tile (skge_rescal_tile.h, k_rel_rescal's too).  A
//                     triple's score does not depend on its place in the item,
//                     so the scatter's order does not reach the bits.
// No float atomics anywhere: the same input gives the same bytes.
#include <algorithm>
#include <limits.h>

#include "skge_diag.h"
#include "skge_elem.h"
#include "skge_host.h"
#include "skge_hole.h"
#include "skge_rot.h"
#include "skge_pools.h"
#include "skge_rescal_tile.h"
#include "skge_transe_l1.h"

namespace skge {

struct ScoreArgs {
  const float* E;
  const float* R;
  int d;
  const int* trip;   // [n][3] (s, o, p)
  int n;
  float* out;        // [n]
};

// ---- TransE ----
template <int KQ, bool L1>
__global__ __launch_bounds__(256) void k_score_transe4(ScoreArgs a) {
  const int wpb = blockDim.x >> 6, d = a.d;
  for (int i = blockIdx.x * wpb + (threadIdx.x >> 6); i < a.n; i += gridDim.x * wpb) {
    const int s = uni(a.trip[3 * (size_t)i]), o = uni(a.trip[3 * (size_t)i + 1]);
    const int p = uni(a.trip[3 * (size_t)i + 2]);
    float4 es[KQ], eo[KQ], rp[KQ];
    load_row4<KQ>(a.E, s, d, es);
    load_row4<KQ>(a.R, p, d, rp);
    load_row4<KQ>(a.E, o, d, eo);
    float ps;
    if (L1) {   // the positive's partial of the step kernels; the rest is dead code
      float n0, n1;
      float4 gp[KQ], g0[KQ], g1[KQ];
      l1_scores_signs<KQ>(es, eo, es, eo, rp, ps, n0, n1, gp, g0, g1);
    } else {
      ps = 0.0f;
#pragma unroll
      for (int m = 0; m < KQ; ++m) {
        ps += transe_elem<false>(es[m].x, rp[m].x, eo[m].x);
        ps += transe_elem<false>(es[m].y, rp[m].y, eo[m].y);
        ps += transe_elem<false>(es[m].z, rp[m].z, eo[m].z);
        ps += transe_elem<false>(es[m].w, rp[m].w, eo[m].w);
      }
    }
    const float sc = -wave_sum(ps);
    if (lane_id() == 0) a.out[i] = sc;
  }
}

template <bool L1>
__global__ __launch_bounds__(256) void k_score_transe(ScoreArgs a) {
  const int wpb = blockDim.x >> 6, d = a.d, l = lane_id();
  for (int i = blockIdx.x * wpb + (threadIdx.x >> 6); i < a.n; i += gridDim.x * wpb) {
    const int s = uni(a.trip[3 * (size_t)i]), o = uni(a.trip[3 * (size_t)i + 1]);
    const int p = uni(a.trip[3 * (size_t)i + 2]);
    const float* es = a.E + (size_t)s * d;
    const float* eo = a.E + (size_t)o * d;
    const float* rp = a.R + (size_t)p * d;
    float ps = 0.0f;
    for (int k = l; k < d; k += 64) ps += transe_elem<L1>(es[k], rp[k], eo[k]);
    const float sc = -wave_sum(ps);
    if (l == 0) a.out[i] = sc;
  }
}

// ---- HolE ----
// per wave: R_p as an a operand (d + 4) and E_o doubled (2 d + 4)
__host__ __device__ __forceinline__ int score_hole4_lds_floats(int d) { return 3 * d + 8; }

__global__ __launch_bounds__(256) void k_score_hole4(ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int wpb = blockDim.x >> 6, d = a.d;
  float* sR = smem + (threadIdx.x >> 6) * score_hole4_lds_floats(d);
  float* sO2 = sR + d + 4;
  for (int i = blockIdx.x * wpb + (threadIdx.x >> 6); i < a.n; i += gridDim.x * wpb) {
    const int s = uni(a.trip[3 * (size_t)i]), o = uni(a.trip[3 * (size_t)i + 1]);
    const int p = uni(a.trip[3 * (size_t)i + 2]);
    float4 es[1], eo[1], rp[1];
    load_row4<1>(a.E, s, d, es);
    load_row4<1>(a.R, p, d, rp);
    load_row4<1>(a.E, o, d, eo);
    q_lds(sR, rp[0], d);
    q_lds_dbl(sO2, eo[0], d);
    __builtin_amdgcn_wave_barrier();
    const float* const sa[1] = {sR};
    float4 A[1];
    corr_quad<1>(sa, sO2, d, A);   // ccorr(R_p, E_o): R_p . ccorr(E_s, E_o) = E_s . A
    const float sc = hole_score_q(es[0], A[0]);
    if (lane_id() == 0) a.out[i] = sc;
    __builtin_amdgcn_wave_barrier();   // the next triple's staging
  }
}

__global__ __launch_bounds__(256) void k_score_hole(ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int wpb = blockDim.x >> 6, d = a.d, l = lane_id();
  float* es = smem + (threadIdx.x >> 6) * 2 * d;
  float* eo = es + d;
  for (int i = blockIdx.x * wpb + (threadIdx.x >> 6); i < a.n; i += gridDim.x * wpb) {
    const int s = uni(a.trip[3 * (size_t)i]), o = uni(a.trip[3 * (size_t)i + 1]);
    const int p = uni(a.trip[3 * (size_t)i + 2]);
    for (int k = l; k < d; k += 64) {
      es[k] = a.E[(size_t)s * d + k];
      eo[k] = a.E[(size_t)o * d + k];
    }
    __builtin_amdgcn_wave_barrier();
    const float* rp = a.R + (size_t)p * d;
    float ps = 0.0f;
    for (int k = l; k < d; k += 64) ps = fmaf(rp[k], ccorr_direct_k(es, eo, d, k), ps);
    const float sc = wave_sum(ps);
    if (l == 0) a.out[i] = sc;
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- DistMult / ComplEx: E_s . (conj(R_p) * E_o), the step kernels' score
// (skge_diag.h), one wave per triple, rows in registers ----
template <int MODEL, int KM>
__global__ __launch_bounds__(256) void k_score_diag(ScoreArgs a) {
  const int wpb = blockDim.x >> 6, d = a.d;
  for (int i = blockIdx.x * wpb + (threadIdx.x >> 6); i < a.n; i += gridDim.x * wpb) {
    const int s = uni(a.trip[3 * (size_t)i]), o = uni(a.trip[3 * (size_t)i + 1]);
    const int p = uni(a.trip[3 * (size_t)i + 2]);
    float es[KM], eo[KM], rp[KM], q[KM];
    load_row<KM>(a.E, s, d, es);
    load_row<KM>(a.R, p, d, rp);
    load_row<KM>(a.E, o, d, eo);
    diag_cmul<MODEL, KM>(rp, eo, q);
    const float sc = diag_dot<KM>(es, q);
    if (lane_id() == 0) a.out[i] = sc;
  }
}

template <int MODEL>
static void launch_score_diag(hipStream_t st, int blocks, const ScoreArgs& a) {
#define SKGE_SC_D(K) \
  case K: hipLaunchKernelGGL((k_score_diag<MODEL, K>), dim3(blocks), dim3(256), 0, st, a); break;
  switch (km_for(a.d)) {
    SKGE_SC_D(1)
    SKGE_SC_D(2)
    SKGE_SC_D(3)
    SKGE_SC_D(4)
    SKGE_SC_D(8)
    default:
    SKGE_SC_D(16)
  }
#undef SKGE_SC_D
}

// ---- RotatE: the step kernels' score (skge_rot.h), one wave per triple, rows
// in registers ----
template <int KM>
__global__ __launch_bounds__(256) void k_score_rot(ScoreArgs a) {
  const int wpb = blockDim.x >> 6, d = a.d;
  for (int i = blockIdx.x * wpb + (threadIdx.x >> 6); i < a.n; i += gridDim.x * wpb) {
    const int s = uni(a.trip[3 * (size_t)i]), o = uni(a.trip[3 * (size_t)i + 1]);
    const int p = uni(a.trip[3 * (size_t)i + 2]);
    float es[KM], eo[KM], rp[KM], t[KM], u[KM];
    load_row<KM>(a.E, s, d, es);
    load_row<KM>(a.R, p, d, rp);
    load_row<KM>(a.E, o, d, eo);
    diag_mul<COMPLEX, KM>(es, rp, t);
    rot_sub<KM>(t, eo, u);
    const float sc = -rot_unit<KM>(u);
    if (lane_id() == 0) a.out[i] = sc;
  }
}

static void launch_score_rot(hipStream_t st, int blocks, const ScoreArgs& a) {
#define SKGE_SC_R(K) \
  case K: hipLaunchKernelGGL((k_score_rot<K>), dim3(blocks), dim3(256), 0, st, a); break;
  switch (km_for(a.d)) {
    SKGE_SC_R(1)
    SKGE_SC_R(2)
    SKGE_SC_R(3)
    SKGE_SC_R(4)
    SKGE_SC_R(8)
    default:
    SKGE_SC_R(16)
  }
#undef SKGE_SC_R
}

// ---- RESCAL ----
__global__ __launch_bounds__(256) void k_score_rel(const int* __restrict__ trip, int n,
                                                   int* __restrict__ rel) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    rel[i] = trip[3 * (size_t)i + 2];
}

struct ScoreRescalArgs {
  const float* E;
  const float* W;    // [M][d][d]
  int d;
  const int* trip;
  float* out;
  PoolWork pw;       // items: (relation, first slot of order, triples, 0)
};

// the score tile (skge_rescal_tile.h) over one item: the item's (s, o) rows
// through the order array, W_p of the item's relation.  Rows past the item's
// count read entity 0 and are never written.
template <int QB>
__global__ __launch_bounds__(256, 2) void k_score_rescal(ScoreRescalArgs a) {
  constexpr int MI = QB / 32;
  __shared__ int s_s[QB], s_o[QB], s_v[QB];
  __shared__ float s_red[4][QB];
  if ((int)blockIdx.x >= *a.pw.n_items) return;
  const int4 item = a.pw.items[blockIdx.x];
#ifdef SKGE_MUTANT_RESCAL_IGNORE_REL   // tools/mutants_linkpred.sh: every item reads W_0
  const int rel = 0, vbeg = item.y, vcnt = item.z;
#else
  const int rel = item.x, vbeg = item.y, vcnt = item.z;
#endif
  const int tid = threadIdx.x, d = a.d;
  for (int i = tid; i < QB; i += 256) {
    const int v = i < vcnt ? a.pw.order[vbeg + i] : -1;
    s_v[i] = v;
    s_s[i] = v >= 0 ? a.trip[3 * (size_t)v] : 0;
    s_o[i] = v >= 0 ? a.trip[3 * (size_t)v + 1] : 0;
  }
  __syncthreads();
  bool eok[MI];
#pragma unroll
  for (int u = 0; u < MI; ++u) eok[u] = (tid >> 3) + 32 * u < vcnt;
  rescal_score_tile<QB>(a.E, a.W + (size_t)rel * d * d, d, s_s, s_o, eok, s_red);
  if (tid < QB && s_v[tid] >= 0) a.out[s_v[tid]] = rescal_row_sum<QB>(s_red, tid);
}

// triples per item: wide items when the average relation fills them
static int score_rescal_qb(int n, int M) { return (long long)n >= 64ll * M ? 128 : 32; }

static bool score_sizes_ok(int model, long long n, int M, int d) {
  return model_known(model) && (!model_complex_rows(model) || d % 2 == 0) && n >= 0 && n <= INT_MAX / 4 && M >= 1 && d >= 1 && d <= 1024;
}

}  // namespace skge

using namespace skge;

extern "C" size_t skge_score_workspace_bytes(int model, int n, int M, int d) {
  if (!score_sizes_ok(model, n, M, d)) return 0;
  if (model != SKGE_RESCAL || n == 0) return 256;   // unused; never 0 for good sizes
  return align256((size_t)n * sizeof(int)) + pool_group_bytes(n, M, score_rescal_qb(n, M)) + 512;
}

extern "C" int skge_score(void* stream, int model, const float* E, const float* R, int N, int M,
                          int d, const int* trip, int64_t n, void* workspace, size_t ws_bytes,
                          float* score_out) {
  SKGE_CHECK_MODEL(model, d);
  SKGE_CHECK_ARG(n >= 0 && n <= INT_MAX / 4, "n = %lld outside 0 .. %d", (long long)n, INT_MAX / 4);
  SKGE_CHECK_ARG(N > 0 && M >= 1 && d >= 1 && d <= 1024,
                 "bad sizes (N = %d, M = %d, d = %d, 1 <= d <= 1024)", N, M, d);
  SKGE_CHECK_ARG(E && R, "NULL argument (tables)");
  if (n == 0) return SKGE_OK;
  SKGE_CHECK_ARG(trip && score_out, "NULL argument");
  const size_t need = skge_score_workspace_bytes(model, (int)n, M, d);
  SKGE_CHECK_ARG(workspace && ws_bytes >= need,
                 "score workspace needs %zu bytes", need);
  hipStream_t st = as_stream(stream);
  ScoreArgs a;
  a.E = E;
  a.R = R;
  a.d = d;
  a.trip = trip;
  a.n = (int)n;
  a.out = score_out;
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, 16384));
  const bool quad = (d & 3) == 0;
  if (model == SKGE_TRANSE_L1 || model == SKGE_TRANSE_L2) {
    const bool l1 = model == SKGE_TRANSE_L1;
    const int kq = (d + 255) / 256;
#define SKGE_SC_T4(KQ)                                                                  \
  do {                                                                                  \
    if (l1)                                                                             \
      hipLaunchKernelGGL((k_score_transe4<KQ, true>), dim3(blocks), dim3(256), 0, st, a);  \
    else                                                                                \
      hipLaunchKernelGGL((k_score_transe4<KQ, false>), dim3(blocks), dim3(256), 0, st, a); \
  } while (0)
    if (quad && kq == 1)
      SKGE_SC_T4(1);
    else if (quad && kq == 2)
      SKGE_SC_T4(2);
    else if (quad)
      SKGE_SC_T4(4);
    else if (l1)
      hipLaunchKernelGGL((k_score_transe<true>), dim3(blocks), dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL((k_score_transe<false>), dim3(blocks), dim3(256), 0, st, a);
#undef SKGE_SC_T4
    SKGE_CHECK_LAUNCH("score (TransE)");
    return SKGE_OK;
  }
  if (model == SKGE_HOLE) {
    if (quad && d <= 256)
      hipLaunchKernelGGL(k_score_hole4, dim3(blocks), dim3(256),
                         (size_t)4 * score_hole4_lds_floats(d) * sizeof(float), st, a);
    else
      hipLaunchKernelGGL(k_score_hole, dim3(blocks), dim3(256), (size_t)4 * 2 * d * sizeof(float),
                         st, a);
    SKGE_CHECK_LAUNCH("score (HolE)");
    return SKGE_OK;
  }
  if (model == SKGE_ROTATE) {
    launch_score_rot(st, blocks, a);
    SKGE_CHECK_LAUNCH("score (RotatE)");
    return SKGE_OK;
  }
  if (model_diag(model)) {
    if (model == SKGE_DISTMULT)
      launch_score_diag<DISTMULT>(st, blocks, a);
    else
      launch_score_diag<COMPLEX>(st, blocks, a);
    SKGE_CHECK_LAUNCH("score (DistMult / ComplEx)");
    return SKGE_OK;
  }
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  int* rel = (int*)ws;
  void* gws = ws + align256((size_t)n * sizeof(int));
  const int qb = score_rescal_qb((int)n, M);
  const int eb = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 2048));
  hipLaunchKernelGGL(k_score_rel, dim3(eb), dim3(256), 0, st, trip, (int)n, rel);
  ScoreRescalArgs r;
  r.E = E;
  r.W = R;
  r.d = d;
  r.trip = trip;
  r.out = score_out;
  // bins: relation p sits in launch_pool_group's bin p + 1, so item.x = p
  const int rc = launch_pool_group(st, rel, (int)n, M, qb, nullptr, nullptr, gws, &r.pw);
  if (rc != SKGE_OK) return rc;
  const int max_items = pool_items_max((int)n, M, qb);
  if (qb == 128)
    hipLaunchKernelGGL((k_score_rescal<128>), dim3(max_items), dim3(256), 0, st, r);
  else
    hipLaunchKernelGGL((k_score_rescal<32>), dim3(max_items), dim3(256), 0, st, r);
  SKGE_CHECK_LAUNCH("score (RESCAL)");
  return SKGE_OK;
}
