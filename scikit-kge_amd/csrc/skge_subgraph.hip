// Subgraph embeddings and subgraph ranking on the device.
//
// The reference groups the triples by (relation, subject) and by (relation,
// object), embeds every group with more than `mincard` members as the mean
// (and variance) of its members' entity rows (Experiment.make_subgraphs,
// skge/base.py:122-202) and ranks the groups, not the entities, for a test
// query (FilteredRankingEval.subgraph_positions, skge/base.py:828-911).
//
// Embeddings: a segmented gather-reduce over the members' CSR.
//   k_sub_plan    one workgroup: the groups longer than the split threshold
//                 get ceil(count / split) pieces each, at offsets of an
//                 exclusive scan in group order
//   k_sub_piece   one wave per piece: the piece's partial sum (or partial sum
//                 of squared differences from the mean) into the workspace
//   k_sub_group   one wave per group: a short group start to end (sum, mean,
//                 then the squared differences in a second pass over the
//                 members); a long group's mean from its pieces, added in
//                 piece order
//   k_sub_var     one wave per long group: its variance from its pieces
// A wave owns a row: lanes run across d (16-byte loads when d % 4 == 0), the
// members stream through four rows at a time and are added in member order.
// No float atomics and no order that depends on timing: the same bits on
// every run.
//
// Ranking: the evaluator's query vectors (launch_rank_query) and its all-row
// counting pass over the subgraph table (launch_rank_count); new here only
//   k_sub_target  one wave per (query, direction): the best score among the
//                 subgraphs that contain the answer (the skipped one left
//                 out), by rank_score, the counting pass's own chain
#include <algorithm>
#include <stdlib.h>

#include "skge_host.h"

namespace skge {

constexpr int SG_SPLIT = 256;   // members per piece; groups longer than this are split

// SKGE_SUBGRAPH_SPLIT overrides the threshold (tests split a small group)
static int sg_split() {
  const char* e = getenv("SKGE_SUBGRAPH_SPLIT");
  if (!e || !*e) return SG_SPLIT;
  const long v = strtol(e, nullptr, 10);
  return (int)std::max(2L, std::min(v, 1L << 20));
}

struct EmbedArgs {
  const float* E;
  int d, S;
  const long long* mem_off;   // [S + 1]
  const int* mem_ent;
  float* SA;
  float* SV;                  // or nullptr
  int split, cap;             // members per piece, pieces the workspace holds
  int* grp_base;              // [S] a long group's first piece, -1: not split
  int* piece_grp;             // [cap] the piece's group, -1: unused
  float* parts;               // [cap][d]
};

// a row in registers: K float4 (VEC, d % 4 == 0) or K floats per lane
template <bool VEC, int K>
struct RowRegs {
  static constexpr int NV = VEC ? 4 * K : K;
};

template <bool VEC, int K>
__device__ __forceinline__ void sg_load(const float* __restrict__ T, int row, int d,
                                        float (&v)[RowRegs<VEC, K>::NV]) {
  if constexpr (VEC) {
    float4 t[K];
    load_row4<K>(T, row, d, t);
#pragma unroll
    for (int m = 0; m < K; ++m) {
      v[4 * m] = t[m].x;
      v[4 * m + 1] = t[m].y;
      v[4 * m + 2] = t[m].z;
      v[4 * m + 3] = t[m].w;
    }
  } else {
    load_row<K>(T, row, d, v);
  }
}

template <bool VEC, int K>
__device__ __forceinline__ void sg_store(float* __restrict__ T, long long row, int d,
                                         const float (&v)[RowRegs<VEC, K>::NV]) {
  const int l = lane_id();
  float* base = T + (size_t)row * d;
  if constexpr (VEC) {
    const int nq = d >> 2;
#pragma unroll
    for (int m = 0; m < K; ++m) {
      const int q = 64 * m + l;
      if (q < nq)
        reinterpret_cast<float4*>(base)[q] =
            make_float4(v[4 * m], v[4 * m + 1], v[4 * m + 2], v[4 * m + 3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e = l + 64 * k;
      if (e < d) base[e] = v[k];
    }
  }
}

// acc += x (SQ: += (x - mean)^2), elementwise
template <int NV, bool SQ>
__device__ __forceinline__ void sg_add(float (&acc)[NV], const float (&x)[NV],
                                       const float (&mean)[NV]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    if (SQ) {
      const float t = x[k] - mean[k];
      acc[k] = fmaf(t, t, acc[k]);
    } else {
      acc[k] += x[k];
    }
  }
}

// the members mem_ent[beg .. end) into acc, in member order; four row gathers
// are in flight before the first is added
template <bool VEC, int K, bool SQ>
__device__ __forceinline__ void sg_accum(const float* __restrict__ E, int d,
                                         const int* __restrict__ mem_ent, long long beg,
                                         long long end,
                                         const float (&mean)[RowRegs<VEC, K>::NV],
                                         float (&acc)[RowRegs<VEC, K>::NV]) {
  constexpr int NV = RowRegs<VEC, K>::NV;
  long long i = beg;
  for (; i + 4 <= end; i += 4) {
    const int m0 = __builtin_amdgcn_readfirstlane(mem_ent[i]);
    const int m1 = __builtin_amdgcn_readfirstlane(mem_ent[i + 1]);
    const int m2 = __builtin_amdgcn_readfirstlane(mem_ent[i + 2]);
    const int m3 = __builtin_amdgcn_readfirstlane(mem_ent[i + 3]);
    float x0[NV], x1[NV], x2[NV], x3[NV];
    sg_load<VEC, K>(E, m0, d, x0);
    sg_load<VEC, K>(E, m1, d, x1);
    sg_load<VEC, K>(E, m2, d, x2);
    sg_load<VEC, K>(E, m3, d, x3);
    sg_add<NV, SQ>(acc, x0, mean);
    sg_add<NV, SQ>(acc, x1, mean);
    sg_add<NV, SQ>(acc, x2, mean);
    sg_add<NV, SQ>(acc, x3, mean);
  }
  for (; i < end; ++i) {
    const int m0 = __builtin_amdgcn_readfirstlane(mem_ent[i]);
    float x0[NV];
    sg_load<VEC, K>(E, m0, d, x0);
    sg_add<NV, SQ>(acc, x0, mean);
  }
}

// rows first .. first + n - 1 of the partial table, added in row order
template <bool VEC, int K>
__device__ __forceinline__ void sg_sum_parts(const float* __restrict__ parts, int d, int first,
                                             int n, float (&acc)[RowRegs<VEC, K>::NV]) {
  constexpr int NV = RowRegs<VEC, K>::NV;
  for (int i = 0; i < n; ++i) {
    float x[NV];
    sg_load<VEC, K>(parts, first + i, d, x);
    sg_add<NV, false>(acc, x, x);
  }
}

__device__ __forceinline__ long long sg_pieces(long long cnt, int split) {
  return cnt > split ? (cnt + split - 1) / split : 0;
}

// ---- the long groups' pieces: one workgroup, groups in id order ----
__global__ __launch_bounds__(256) void k_sub_plan(EmbedArgs a) {
  __shared__ long long s_n[256];
  const int t = threadIdx.x;
  const int per = (a.S + 255) / 256;
  const int g0 = min(a.S, t * per), g1 = min(a.S, g0 + per);
  long long n = 0;
  for (int g = g0; g < g1; ++g) n += sg_pieces(a.mem_off[g + 1] - a.mem_off[g], a.split);
  s_n[t] = n;
  __syncthreads();
  if (t == 0) {
    long long run = 0;
    for (int i = 0; i < 256; ++i) {
      const long long x = s_n[i];
      s_n[i] = run;
      run += x;
    }
  }
  __syncthreads();
  long long base = s_n[t];
  for (int g = g0; g < g1; ++g) {
    const long long np = sg_pieces(a.mem_off[g + 1] - a.mem_off[g], a.split);
    // a workspace sized for fewer members than the CSR holds: the groups
    // past its end run unsplit (slower, still exact in order)
    const bool fits = np > 0 && base + np <= (long long)a.cap;
    a.grp_base[g] = fits ? (int)base : -1;
    if (fits)
      for (long long i = 0; i < np; ++i) a.piece_grp[base + i] = g;
    base += np;
  }
}

// ---- one wave per piece ----
template <bool VEC, int K, bool SQ>
__global__ __launch_bounds__(256) void k_sub_piece(EmbedArgs a) {
  constexpr int NV = RowRegs<VEC, K>::NV;
  const int wpb = blockDim.x >> 6;
  for (int w = blockIdx.x * wpb + (threadIdx.x >> 6); w < a.cap; w += gridDim.x * wpb) {
    const int g = __builtin_amdgcn_readfirstlane(a.piece_grp[w]);
    if (g < 0) continue;
    const int pi = w - __builtin_amdgcn_readfirstlane(a.grp_base[g]);
    const long long beg = a.mem_off[g] + (long long)pi * a.split;
    const long long end = min(a.mem_off[g + 1], beg + a.split);
    float acc[NV], mean[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = mean[k] = 0.0f;
    if (SQ) sg_load<VEC, K>(a.SA, g, a.d, mean);
    sg_accum<VEC, K, SQ>(a.E, a.d, a.mem_ent, beg, end, mean, acc);
    sg_store<VEC, K>(a.parts, w, a.d, acc);
  }
}

// ---- one wave per group: SA, and SV of the groups that are not split ----
template <bool VEC, int K>
__global__ __launch_bounds__(256) void k_sub_group(EmbedArgs a) {
  constexpr int NV = RowRegs<VEC, K>::NV;
  const int g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (g >= a.S) return;
  const long long beg = a.mem_off[g], end = a.mem_off[g + 1], cnt = end - beg;
  const int base = __builtin_amdgcn_readfirstlane(a.grp_base[g]);
  float acc[NV], mean[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = mean[k] = 0.0f;
  if (base < 0)
    sg_accum<VEC, K, false>(a.E, a.d, a.mem_ent, beg, end, mean, acc);
  else
    sg_sum_parts<VEC, K>(a.parts, a.d, base, (int)sg_pieces(cnt, a.split), acc);
  const float n = (float)cnt;
#pragma unroll
  for (int k = 0; k < NV; ++k) mean[k] = cnt > 0 ? acc[k] / n : 0.0f;
  sg_store<VEC, K>(a.SA, g, a.d, mean);
  if (!a.SV) return;
  if (cnt <= 2) {   // the reference's quirk (skge/base.py:154-157): the mean
    sg_store<VEC, K>(a.SV, g, a.d, mean);
  } else if (base < 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0f;
    sg_accum<VEC, K, true>(a.E, a.d, a.mem_ent, beg, end, mean, acc);
    const float n1 = (float)(cnt - 1);
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = acc[k] / n1;
    sg_store<VEC, K>(a.SV, g, a.d, acc);
  }
}

// ---- one wave per group: SV of the split groups (count > split >= 2) ----
template <bool VEC, int K>
__global__ __launch_bounds__(256) void k_sub_var(EmbedArgs a) {
  constexpr int NV = RowRegs<VEC, K>::NV;
  const int g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (g >= a.S) return;
  const int base = __builtin_amdgcn_readfirstlane(a.grp_base[g]);
  if (base < 0) return;
  const long long cnt = a.mem_off[g + 1] - a.mem_off[g];
  float acc[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = 0.0f;
  sg_sum_parts<VEC, K>(a.parts, a.d, base, (int)sg_pieces(cnt, a.split), acc);
  const float n1 = (float)(cnt - 1);
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = acc[k] / n1;
  sg_store<VEC, K>(a.SV, g, a.d, acc);
}

template <bool VEC, int K>
static void launch_embed(hipStream_t st, const EmbedArgs& a) {
  const int gblocks = (a.S + 3) / 4;
  const int pblocks = std::min((a.cap + 3) / 4, 1 << 20);
  hipLaunchKernelGGL(k_sub_plan, dim3(1), dim3(256), 0, st, a);
  hipLaunchKernelGGL((k_sub_piece<VEC, K, false>), dim3(pblocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL((k_sub_group<VEC, K>), dim3(gblocks), dim3(256), 0, st, a);
  if (a.SV) {
    hipLaunchKernelGGL((k_sub_piece<VEC, K, true>), dim3(pblocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL((k_sub_var<VEC, K>), dim3(gblocks), dim3(256), 0, st, a);
  }
}

// workspace: [grp_base S ints | parts cap x d floats | piece_grp cap ints]
static size_t sg_head_bytes(int S) { return align256((size_t)S * sizeof(int)); }
static size_t sg_piece_bytes(int d) { return (size_t)d * sizeof(float) + sizeof(int); }

// ---- ranking: the best eligible subgraph that contains the answer ----
struct SubRankArgs {
  const float* X;        // [S][d] SA or SV
  int S, d, nq;
  const int* queries;    // [nq][3] (s, o, p)
  const int* skip_tail;  // [nq] subgraph id or -1
  const int* skip_head;
  const long long* ans_off;   // [N + 1]
  const int* ans_sub;
  const float* Q;        // [2 nq][d]
  float* tgt;            // [2 nq]
  int* ranks;            // [nq][2], here: 1 - (the skipped subgraph beats the target),
                         // or eligible + 1 when no subgraph holds the answer
  int* found;            // [nq][2]
};

template <bool L1>
__global__ __launch_bounds__(256) void k_sub_target(SubRankArgs a) {
  const int l = lane_id();
  const int v = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (v >= 2 * a.nq) return;
  const int i = v >> 1, dir = v & 1;   // 0: tail (the answer is o), 1: head (s)
  const int ans = __builtin_amdgcn_readfirstlane(a.queries[3 * i + (dir ? 0 : 1)]);
  int skip = __builtin_amdgcn_readfirstlane(dir ? a.skip_head[i] : a.skip_tail[i]);
  if (skip < 0 || skip >= a.S) skip = -1;
  const float* q = a.Q + (size_t)v * a.d;
  float best = -INFINITY;
  int any = 0;
  const long long jb = a.ans_off[ans], je = a.ans_off[ans + 1];
  for (long long j = jb + l; j < je; j += 64) {
    const int sub = a.ans_sub[j];
    if (sub == skip) continue;
    const float sc = rank_score<L1>(q, a.X + (size_t)sub * a.d, a.d);
    best = fmaxf(best, sc);
    any = 1;
  }
  const int found = __any(any) ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) best = fmaxf(best, __shfl_xor(best, off));
  // the counting pass counts every row above the target, the skipped one too
  int dec = 0;
  if (found && skip >= 0) dec = rank_score<L1>(q, a.X + (size_t)skip * a.d, a.d) > best ? 1 : 0;
  if (l == 0) {
    a.tgt[v] = found ? best : INFINITY;
    a.ranks[v] = found ? 1 - dec : a.S - (skip >= 0 ? 1 : 0) + 1;
    a.found[v] = found;
  }
}

}  // namespace skge

using namespace skge;

extern "C" size_t skge_subgraph_embed_workspace_bytes(int S, int d, int64_t n_members) {
  if (S <= 0 || d <= 0 || n_members < 0) return 0;
  const size_t cap = 2 * (size_t)(n_members / sg_split()) + 2;
  return sg_head_bytes(S) + cap * sg_piece_bytes(d);
}

extern "C" int skge_subgraph_embed(void* stream, const float* E, int N, int d,
                                   const int64_t* mem_off, const int* mem_ent, int S, float* SA,
                                   float* SV, void* workspace, size_t ws_bytes) {
  SKGE_CHECK_ARG(E && mem_off && mem_ent && SA, "NULL argument");
  SKGE_CHECK_ARG(N > 0 && d > 0 && d <= 1024 && S > 0, "bad sizes (S > 0, d <= 1024)");
  SKGE_CHECK_ARG(workspace && ws_bytes >= sg_head_bytes(S) + 2 * sg_piece_bytes(d),
                 "subgraph embed workspace needs skge_subgraph_embed_workspace_bytes(S, d, "
                 "members) bytes");
  EmbedArgs a = {};
  a.E = E;
  a.d = d;
  a.S = S;
  a.mem_off = (const long long*)mem_off;
  a.mem_ent = mem_ent;
  a.SA = SA;
  a.SV = SV;
  a.split = sg_split();
  a.cap = (int)std::min((ws_bytes - sg_head_bytes(S)) / sg_piece_bytes(d), (size_t)1 << 30);
  a.grp_base = (int*)workspace;
  a.parts = (float*)((char*)workspace + sg_head_bytes(S));
  a.piece_grp = (int*)(a.parts + (size_t)a.cap * d);
  hipStream_t st = as_stream(stream);
  SKGE_CHECK_HIP(hipMemsetAsync(a.piece_grp, 0xff, (size_t)a.cap * sizeof(int), st));
  if (d % 4 == 0) {
    if (d <= 256)
      launch_embed<true, 1>(st, a);
    else if (d <= 512)
      launch_embed<true, 2>(st, a);
    else
      launch_embed<true, 4>(st, a);
  } else {
    if (d <= 64)
      launch_embed<false, 1>(st, a);
    else if (d <= 256)
      launch_embed<false, 4>(st, a);
    else
      launch_embed<false, 16>(st, a);
  }
  SKGE_CHECK_LAUNCH("subgraph embed");
  return SKGE_OK;
}

extern "C" size_t skge_subgraph_rank_workspace_bytes(int nq, int d) {
  if (nq <= 0 || d <= 0) return 0;
  return (size_t)2 * nq * d * sizeof(float) + (size_t)2 * nq * sizeof(float) + 256;
}

extern "C" int skge_subgraph_rank(void* stream, int model, const float* E, const float* R, int N,
                                  int d, const float* X, int S, const int* queries, int nq,
                                  const int* skip_tail, const int* skip_head,
                                  const int64_t* ans_off, const int* ans_sub, void* workspace,
                                  size_t ws_bytes, int* ranks_out, int* found_out) {
  SKGE_CHECK_ARG(E && R && X, "NULL table");
  SKGE_CHECK_ARG(queries && skip_tail && skip_head && ans_off && ans_sub && ranks_out && found_out,
                 "NULL argument");
  SKGE_REFUSE_ROTATE(model, "subgraph ranking");
  SKGE_CHECK_ARG(model >= 0 && model <= 3, "unknown model %d", model);
  SKGE_CHECK_ARG(N > 0 && d > 0 && d <= 1024 && S > 0 && nq >= 0,
                 "bad sizes (S > 0, d <= 1024)");
  if (nq == 0) return SKGE_OK;
  SKGE_CHECK_ARG(workspace && ws_bytes >= skge_subgraph_rank_workspace_bytes(nq, d),
                 "subgraph rank workspace needs %zu bytes",
                 skge_subgraph_rank_workspace_bytes(nq, d));
  SubRankArgs a = {};
  a.X = X;
  a.S = S;
  a.d = d;
  a.nq = nq;
  a.queries = queries;
  a.skip_tail = skip_tail;
  a.skip_head = skip_head;
  a.ans_off = (const long long*)ans_off;
  a.ans_sub = ans_sub;
  float* Q = (float*)workspace;
  a.Q = Q;
  a.tgt = Q + (size_t)2 * nq * d;
  a.ranks = ranks_out;
  a.found = found_out;
  hipStream_t st = as_stream(stream);
  // the true entities' scores land in tgt first; k_sub_target overwrites them
  launch_rank_query(st, model, E, R, N, d, queries, nq, Q, a.tgt);
  const bool l1 = model == SKGE_TRANSE_L1 || model == SKGE_TRANSE_L2;
  const int tb = (2 * nq + 3) / 4;
  if (l1)
    hipLaunchKernelGGL((k_sub_target<true>), dim3(tb), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((k_sub_target<false>), dim3(tb), dim3(256), 0, st, a);
  launch_rank_count(st, l1, X, S, d, Q, a.tgt, 2 * nq, ranks_out);
  SKGE_CHECK_LAUNCH("subgraph rank");
  return SKGE_OK;
}
