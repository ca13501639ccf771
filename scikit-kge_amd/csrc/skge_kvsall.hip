// 1-N training of DistMult and ComplEx: every query (anchor a, relation p,
// direction t) of a batch is scored against EVERY entity row.  With the query
// vector q = query_elem(model, t == 0, E_a, R_p) (skge_elem.h) the score of
// candidate e is the plain dot product z = q . E_e, so one batch is three fp32
// GEMMs around G = d L / d z.  The core both regimes run (kv_open, kv_queries,
// kv_forward, kv_backward, kv_step; one KvPlan lays out the workspace):
//   k_kv_query    Q [B][d], one wave per query
//   k_kv_gemm     forward: Z = Q E^T in 128 x 128 tiles, the regime's epilogue
//                 on the accumulators; G [B][ldg] (and z, when asked for)
//   k_kv_gemm<DQ>   dq = G E, the contraction over the entities cut into
//                 slices: partial tiles [ns][B][d]
//   k_kv_gemm<DE>   gE = G^T Q, every row, plain stores
//   k_kv_chain    one wave per query: dq_b = the slices' partials in slice
//                 order, then the chain rule into gE[a] and gR[p] (float
//                 atomics) and the mark of R row p
//   k_kv_loss     the loss partials, in order, into *loss
// and a _step follows them with the row updates of skge_update.hip
// (launch_update_table: E every row, R the marked rows).  A regime adds:
//   KvsAll (skge_kvsall_grad), binary cross-entropy against the
//   multi-hot vector of a query's known answers: k_kv_labels turns the answers'
//   CSR into a bitmap [B][ceil(N / 32)]; the <FWD> epilogue takes sigma, the
//   smoothed label and the loss term and writes G = (sigma(z) - y') / B and one
//   loss partial per workgroup.
//   1vsAll (skge_onevsall_grad), softmax cross-entropy against
//   one target per query, with N3: the <OVA> epilogue leaves raw z and starts
//   the reduction across a score row, k_ova_combine finishes it, rewrites G and
//   leaves one loss partial per query; k_ova_n3 adds the N3 gradient;
//   k_kv_chain<true> checks the target too and adds the N3 norms; see "1vsAll".
//
// One tile kernel serves the three products.  An operand is read either in ROW
// form (the contraction index runs along its rows: Q and E in FWD, G in DQ) and
// transposed on its way into LDS, as k_nb_select stages its images
// (skge_neighbours.hip), or in K-MAJOR form (the contraction index is its row
// index: E in DQ, G and Q in DE) and stored as loaded.  Either way the LDS
// image is k-major and a lane reads one dword per MFMA operand.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "skge_elem.h"
#include "skge_host.h"
#include "skge_stage.h"

namespace skge {

int launch_update_table(hipStream_t st, const skge_table_t* t, const float* g, const int* mask);

constexpr int KV_T = 128;            // output rows and columns per tile
constexpr int KV_KC = 32;            // contraction indices per LDS chunk
constexpr int KV_PAD_ROW = KV_T + 1; // transposed image: scalar stores, lanes along the rows
constexpr int KV_PAD_KM = KV_T + 4;  // k-major image: 16-byte stores
constexpr int KV_BMAX = 4096;
constexpr int KV_DMAX = 1024;

// KV_OVA: the 1vsAll forward (raw z and each row's softmax partials per tile)
enum { KV_FWD = 0, KV_DQ = 1, KV_DE = 2, KV_OVA = 3 };

struct KvGemm {
  const float* A;        // ROW form [Mr][lda] / K-MAJOR form [K][lda]
  const float* B;        // ROW form [Nc][ldb] / K-MAJOR form [K][ldb]
  size_t lda, ldb;
  int Mr, Nc, K;         // output rows, output columns, contraction length
  int kslice;            // contraction indices per slice (multiple of KV_KC); DQ only
  unsigned nbx;          // tiles along the output rows (the grid is flat)
  float* C;              // DQ: partials [ns][Mr][Nc]; DE: gE [Mr][Nc]
  // FWD
  float* G;              // [Mr][ldg]
  size_t ldg;
  float* scores;         // optional [Mr][Nc]
  const unsigned* bits;  // [Mr][wpr] answer bitmap
  int wpr;
  float eps, eps_n, inv_b;   // smoothing, smoothing / N, 1 / B
  float* lpart;          // [grid] loss partials
  // OVA: per output row and column tile, over the tile's live columns
  float *pm, *ps, *pt;   // [nby][Mr] max z, sum exp(z - max), sum z
};

// ---- softmax partials (1vsAll) ----
// (m, s): s = sum exp(z - m) over some columns, the identity (-inf, 0) over none
__device__ __forceinline__ void kv_ms_merge(float& m, float& s, float m2, float s2) {
  const float mx = fmaxf(m, m2);
  s = (m == mx ? s : (s == 0.0f ? 0.0f : s * expf(m - mx))) +
      (m2 == mx ? s2 : (s2 == 0.0f ? 0.0f : s2 * expf(m2 - mx)));
  m = mx;
}

// max / sum over the 32 lanes of a lane's half-wave, wave_sum's DPP steps: the
// 16-lane rows' values, then the half's two rows
__device__ __forceinline__ float half_max(float v, int h) {
  v = fmaxf(v, dpp_f<0xb1>(v));
  v = fmaxf(v, dpp_f<0x4e>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  v = fmaxf(v, dpp_f<0x140>(v));
  const float lo = fmaxf(lane_f(v, 0), lane_f(v, 16)), hi = fmaxf(lane_f(v, 32), lane_f(v, 48));
  return h ? hi : lo;
}
__device__ __forceinline__ float half_sum(float v, int h) {
  v += dpp_f<0xb1>(v);
  v += dpp_f<0x4e>(v);
  v += dpp_f<0x141>(v);
  v += dpp_f<0x140>(v);
  const float lo = lane_f(v, 0) + lane_f(v, 16), hi = lane_f(v, 32) + lane_f(v, 48);
  return h ? hi : lo;
}

// ---- query vectors: one wave per query ----
// A query naming a row outside its table scores as the zero vector and takes
// no part in the chain rule (k_kv_chain): nothing is read or written out of
// bounds for it.
__device__ __forceinline__ bool kv_query_ok(int a, int p, int t, int N, int M) {
  return a >= 0 && a < N && p >= 0 && p < M && (t == 0 || t == 1);
}

__global__ __launch_bounds__(256) void k_kv_query(int model, const float* __restrict__ E,
                                                  const float* __restrict__ R, int N, int M, int d,
                                                  const int* __restrict__ qa,
                                                  const int* __restrict__ qp,
                                                  const int* __restrict__ qt, int B,
                                                  float* __restrict__ Q) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), l = lane_id();
  if (b >= B) return;
  const int a = qa[b], p = qp[b], t = qt[b];
  const bool ok = kv_query_ok(a, p, t, N, M);
  const float* ea = E + (size_t)(ok ? a : 0) * d;
  const float* rp = R + (size_t)(ok ? p : 0) * d;
  for (int k = l; k < d; k += 64)
    Q[(size_t)b * d + k] = ok ? query_elem(model, t == 0, ea, rp, nullptr, d, k) : 0.0f;
}

// ---- labels: bit e of row b is set when e answers query b ----
__global__ __launch_bounds__(256) void k_kv_labels(const int* __restrict__ off,
                                                   const int* __restrict__ ids, int B, int N,
                                                   int wpr, unsigned* __restrict__ bits) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), l = lane_id();
  if (b >= B) return;
  const int beg = off[b], end = off[b + 1];
  for (int i = beg + l; i < end; i += 64) {
    const int e = ids[i];
    if (e >= 0 && e < N) atomicOr(bits + (size_t)b * wpr + (e >> 5), 1u << (e & 31));
  }
}

// ---- the tile kernel ----
// The four waves tile the 128 x 128 block 2 x 2, each wave 2 x 2 MFMA tiles of
// 32 x 32: lane l feeds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]
// and holds D[i = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)][j = l & 31].  A 32 x 32
// tile that lies wholly past the output's edge is not computed (wave-uniform).
// Staging: ROW form, thread = 16 bytes of a row's 128-byte chunk, 8 lanes a
// row, four rows 32 apart; K-MAJOR form, thread = 16 bytes of one contraction
// index's 512-byte run, four pieces 32 columns apart.  LDS: 2 x 32 x 132
// dwords at most = 33 KB.
template <bool AKM, bool BKM, int EPI>
__global__ __launch_bounds__(256, 2) void k_kv_gemm(KvGemm a) {
  constexpr int PADA = AKM ? KV_PAD_KM : KV_PAD_ROW, PADB = BKM ? KV_PAD_KM : KV_PAD_ROW;
  __shared__ __attribute__((aligned(16))) float sA[KV_KC * PADA];
  __shared__ __attribute__((aligned(16))) float sB[KV_KC * PADB];
  __shared__ float s_loss[4];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, h = l >> 5;
  const int wq = w >> 1, wt = w & 1;
  const unsigned bx = blockIdx.x % a.nbx, by = blockIdx.x / a.nbx;
  int m0, n0, kbeg, kend, slice = 0;
  if (EPI == KV_DQ) {   // by = column tile + column tiles * slice
    const unsigned nty = (unsigned)((a.Nc + KV_T - 1) / KV_T);
    slice = (int)(by / nty);
    m0 = (int)bx * KV_T;
    n0 = (int)(by % nty) * KV_T;
    kbeg = slice * a.kslice;
    kend = a.K - kbeg < a.kslice ? a.K : kbeg + a.kslice;
  } else {
    m0 = (int)bx * KV_T;
    n0 = (int)by * KV_T;
    kbeg = 0;
    kend = a.K;
  }
  const int st_r = tid >> 3, st_c = (tid & 7) * 4;
  // ROW form needs 16-byte rows for the one-load path; K-MAJOR form too
  const bool veca = (a.lda & 3) == 0, vecb = (a.ldb & 3) == 0;
  // this wave's 32 x 32 tiles that hold any output
  bool am[2], bn[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    am[i] = m0 + wq * 64 + 32 * i < a.Mr;
    bn[i] = n0 + wt * 64 + 32 * i < a.Nc;
  }
  const int ai0 = wq * 64 + (l & 31), bj0 = wt * 64 + (l & 31);
  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][nj][r] = 0.0f;
  for (int k0 = kbeg; k0 < kend; k0 += KV_KC) {
    float4 ra[4], rb[4];
    auto load = [&](auto va, auto vb) {
      constexpr bool VA = decltype(va)::value, VB = decltype(vb)::value;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (AKM) {   // contraction index k0 + st_r, output rows m0 + st_c + 32 u ..
          const int k = k0 + st_r;
          ra[u] = stage_load4<VA>(a.A + (size_t)(k < kend ? k : kbeg) * a.lda, k < kend,
                                  m0 + st_c + 32 * u, a.Mr);
        } else {     // output row m0 + st_r + 32 u, contraction indices k0 + st_c ..
          const int m = m0 + st_r + 32 * u;
          ra[u] = stage_load4<VA>(a.A + (size_t)(m < a.Mr ? m : 0) * a.lda, m < a.Mr, k0 + st_c,
                                  kend);
        }
        if (BKM) {
          const int k = k0 + st_r;
          rb[u] = stage_load4<VB>(a.B + (size_t)(k < kend ? k : kbeg) * a.ldb, k < kend,
                                  n0 + st_c + 32 * u, a.Nc);
        } else {
          const int n = n0 + st_r + 32 * u;
          rb[u] = stage_load4<VB>(a.B + (size_t)(n < a.Nc ? n : 0) * a.ldb, n < a.Nc, k0 + st_c,
                                  kend);
        }
      }
    };
    if (veca && vecb)
      load(std::true_type(), std::true_type());
    else if (veca)
      load(std::true_type(), std::false_type());
    else if (vecb)
      load(std::false_type(), std::true_type());
    else
      load(std::false_type(), std::false_type());
    __syncthreads();   // the previous chunk's reads are done
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (AKM) {
        *reinterpret_cast<float4*>(sA + st_r * PADA + st_c + 32 * u) = ra[u];
      } else {
        float* p = sA + st_c * PADA + st_r + 32 * u;
        p[0] = ra[u].x;
        p[PADA] = ra[u].y;
        p[2 * PADA] = ra[u].z;
        p[3 * PADA] = ra[u].w;
      }
      if (BKM) {
        *reinterpret_cast<float4*>(sB + st_r * PADB + st_c + 32 * u) = rb[u];
      } else {
        float* p = sB + st_c * PADB + st_r + 32 * u;
        p[0] = rb[u].x;
        p[PADB] = rb[u].y;
        p[2 * PADB] = rb[u].z;
        p[3 * PADB] = rb[u].w;
      }
    }
    __syncthreads();
    // two contraction indices per MFMA; an odd tail's second is zero padding
    const int steps = (min(KV_KC, kend - k0) + 1) >> 1;
    float av[2], bv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      av[i] = sA[h * PADA + ai0 + 32 * i];
      bv[i] = sB[h * PADB + bj0 + 32 * i];
    }
    for (int s = 0; s < steps; ++s) {
      // the next step's operands are read while this step's MFMAs run
      const int kn = 2 * min(s + 1, steps - 1) + h;
      float an[2], bnx[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        an[i] = sA[kn * PADA + ai0 + 32 * i];
        bnx[i] = sB[kn * PADB + bj0 + 32 * i];
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nj = 0; nj < 2; ++nj)
          if (am[mi] && bn[nj])
            acc[mi][nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mi], bv[nj], acc[mi][nj], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        av[i] = an[i];
        bv[i] = bnx[i];
      }
    }
  }
  // ---- epilogue ----
  if constexpr (EPI == KV_OVA) {
    // Raw z, and per output row the tile's (max z, sum exp(z - max), sum z)
    // over its live columns: the 32 lanes of the row's half-wave, then the two
    // nj tiles, then the two wt waves through LDS (wt = 0 first).  A skipped
    // 32 x 32 tile is the identity (-inf, 0, 0).  Lane rho of a half keeps row
    // rho = 16 mi + r, so the partials leave in one store per lane.
    // The three half_* reductions of one (r, nj) read lanes with v_readlane,
    // so all 64 lanes must be active in them: they sit under the wave-uniform
    // am / bn tests only, never under a per-lane one, and run for rows at or
    // past Mr as well (acc = 0 there; the result is not stored).
    float km = -INFINITY, ks = 0.0f, kt = 0.0f;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      if (!am[mi]) continue;   // wave-uniform
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = m0 + wq * 64 + 32 * mi + (r & 3) + 8 * (r >> 2) + 4 * h;
        float rm = -INFINITY, rs = 0.0f, rt = 0.0f;
#pragma unroll
        for (int nj = 0; nj < 2; ++nj) {
          if (!bn[nj]) continue;   // wave-uniform
          const int j = n0 + bj0 + 32 * nj;
          const bool live = j < a.Nc;
          const float z = acc[mi][nj][r];
          if (live && i < a.Mr) {
            a.G[(size_t)i * a.ldg + j] = z;
            if (a.scores) a.scores[(size_t)i * a.Nc + j] = z;
          }
          const float m = half_max(live ? z : -INFINITY, h);   // finite: column n0 + .. + 32 nj lives
          const float s = half_sum(live ? expf(z - m) : 0.0f, h);
          const float t = half_sum(live ? z : 0.0f, h);
          kv_ms_merge(rm, rs, m, s);
          rt += t;
        }
        if ((l & 31) == 16 * mi + r) {
          km = rm;
          ks = rs;
          kt = rt;
        }
      }
    }
    const int rho = l & 31;
    const int row = wq * 64 + 32 * (rho >> 4) + (rho & 3) + 8 * ((rho & 15) >> 2) + 4 * h;
    __syncthreads();   // the last chunk's operand reads are done: sA is free
    if (wt == 1) {
      sA[3 * row] = km;
      sA[3 * row + 1] = ks;
      sA[3 * row + 2] = kt;
    }
    __syncthreads();
    if (wt == 0 && m0 + row < a.Mr) {
      kv_ms_merge(km, ks, sA[3 * row], sA[3 * row + 1]);
      kt += sA[3 * row + 2];
      const size_t at = (size_t)by * a.Mr + (m0 + row);
      a.pm[at] = km;
      a.ps[at] = ks;
      a.pt[at] = kt;
    }
    return;
  }
  float lsum = 0.0f;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) {
      if (!(am[mi] && bn[nj])) continue;
      const int j = n0 + bj0 + 32 * nj;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = m0 + wq * 64 + 32 * mi + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (i >= a.Mr || j >= a.Nc) continue;
        const float z = acc[mi][nj][r];
        if (EPI == KV_FWD) {
          // j - (l & 31) is a multiple of 32: one bitmap word per row and tile
          const unsigned word = a.bits[(size_t)i * a.wpr + (j >> 5)];
          const float y = (word >> (j & 31)) & 1u ? (1.0f - a.eps) + a.eps_n : a.eps_n;
          // softplus(z) - y z = -(y log sigma(z) + (1 - y) log(1 - sigma(z)))
          const float e = expf(-fabsf(z));
          const float sig = z >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
          lsum += (fmaxf(z, 0.0f) + log1pf(e)) - y * z;
          a.G[(size_t)i * a.ldg + j] = (sig - y) * a.inv_b;
          if (a.scores) a.scores[(size_t)i * a.Nc + j] = z;
        } else if (EPI == KV_DQ) {
          a.C[((size_t)slice * a.Mr + i) * a.Nc + j] = z;
        } else {
          a.C[(size_t)i * a.Nc + j] = z;
        }
      }
    }
  if (EPI == KV_FWD) {   // the workgroup's loss partial: lanes, then waves 0..3
    lsum = wave_sum(lsum);
    if (l == 0) s_loss[w] = lsum;
    __syncthreads();
    if (tid == 0) a.lpart[blockIdx.x] = ((s_loss[0] + s_loss[1]) + s_loss[2]) + s_loss[3];
  }
}

// ---- chain rule: the arithmetic of a query's wave (k_kv_chain, below n3_elem) ----
// dq_b = sum over the slices, in slice order, of the DQ partials; then
//   DistMult        gE[a] += dq o R_p           gR[p] += dq o E_a
//   ComplEx tails   gE[a] += dq conj(R_p)       gR[p] += dq conj(E_a)
//   ComplEx heads   gE[a] += dq R_p             gR[p] += conj(dq) E_a
// (o elementwise, the rest complex products over (x[2j], x[2j + 1])).
__device__ __forceinline__ void kv_dq_sum(const float* __restrict__ part, int ns, int B, int b,
                                          int d, int l, float* dq) {
  for (int k = l; k < d; k += 64) {
    float s = 0.0f;
    for (int sl = 0; sl < ns; ++sl) s += part[((size_t)sl * B + b) * d + k];
    dq[k] = s;
  }
}

// component k of the two chain-rule rows: va into gE[a], vr into gR[p]
__device__ __forceinline__ void kv_chain_elem(int model, int t, const float* dq, const float* ea,
                                              const float* rp, int k, float& va, float& vr) {
  if (model == SKGE_DISTMULT) {
    va = dq[k] * rp[k];
    vr = dq[k] * ea[k];
  } else {
    const int kp = k ^ 1;
    const bool im = k & 1, tail = t == 0;
    if (tail) {   // dq conj(x): re dq.re x.re + dq.im x.im, im dq.im x.re - dq.re x.im
      va = im ? fmaf(dq[k], rp[kp], -(dq[kp] * rp[k])) : fmaf(dq[k], rp[k], dq[kp] * rp[kp]);
      vr = im ? fmaf(dq[k], ea[kp], -(dq[kp] * ea[k])) : fmaf(dq[k], ea[k], dq[kp] * ea[kp]);
    } else {      // dq r: re dq.re r.re - dq.im r.im, im dq.re r.im + dq.im r.re
      va = im ? fmaf(dq[kp], rp[k], dq[k] * rp[kp]) : fmaf(dq[k], rp[k], -(dq[kp] * rp[kp]));
      // conj(dq) a: re dq.re a.re + dq.im a.im, im dq.re a.im - dq.im a.re
      vr = im ? fmaf(dq[kp], ea[k], -(dq[k] * ea[kp])) : fmaf(dq[k], ea[k], dq[kp] * ea[kp]);
    }
  }
}

// ---- the loss: the partials in block order, one workgroup ----
__global__ __launch_bounds__(256) void k_kv_loss(const float* __restrict__ lpart, unsigned n,
                                                 float inv_b, float* __restrict__ loss) {
  __shared__ double s[256];
  double v = 0.0;
  for (unsigned i = threadIdx.x; i < n; i += 256) v += (double)lpart[i];
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss += (float)(s[0] * (double)inv_b);
}

// ==== 1vsAll: softmax cross-entropy against one target, with N3 ====
// (include/skge_hip.h, skge_onevsall_grad).  A query carries a
// target g; the forward is k_kv_gemm<OVA>, which leaves raw z in G and each
// row's (max, sum exp, sum z) per column tile; k_ova_combine turns them into
// lse_b and the loss term and rewrites G to (softmax - y') / B; the DQ and DE
// products, the chain rule, k_kv_loss and the updates are the core's.
__device__ __forceinline__ bool ova_query_ok(int a, int p, int t, int g, int N, int M) {
  return kv_query_ok(a, p, t, N, M) && g >= 0 && g < N;
}

// block-wide reductions in a fixed order (the tree of k_kv_loss); all 256 threads
__device__ __forceinline__ double block_sum256(double v, double* s) {
  __syncthreads();   // s may still be read from the call before
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  return s[0];
}
__device__ __forceinline__ double block_max256(double v, double* s) {
  __syncthreads();
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + o]);
    __syncthreads();
  }
  return s[0];
}

// Workgroup (b, c) of nsplit per query: every one combines query b's nby
// partials -- the row's maximum mx (exact in any order), then S = sum_tile
// s_tile exp(m_tile - mx) and T = sum_tile t_tile in fp64, thread i over tiles
// i, i + 256, .., then the fixed tree -- and rewrites columns [c chunk, (c + 1)
// chunk) of G's row in place:
//   G_be = (exp((z_be - mx) - log S) - y'_be) / B,   0 for an invalid query.
// The workgroup whose columns hold the target (workgroup 0 of an invalid query)
// reads z_g before it rewrites and leaves lse_b = mx + log S and the query's
// loss partial (mx - z_g) + log S + eps (z_g - T / N); at n3 > 0 it also counts
// the query's anchor, target and relation rows in occ [N + M] (integer adds:
// the counts do not depend on the order).  chunk is a multiple of
// 4: whole 16-byte groups below N move as float4, the last group by element;
// the pad columns past N are neither read nor written.
__global__ __launch_bounds__(256) void k_ova_combine(
    float* __restrict__ G, size_t ldg, int N, int M, int B, int nby, int nsplit, int chunk,
    const float* __restrict__ pm, const float* __restrict__ ps, const float* __restrict__ pt,
    const int* __restrict__ qa, const int* __restrict__ qp, const int* __restrict__ qt,
    const int* __restrict__ qg, float eps, float* __restrict__ lse_ws,
    float* __restrict__ lse_out, float* __restrict__ lpart, int* __restrict__ occ) {
  __shared__ double s_red[256];
  const int b = blockIdx.x / nsplit, c = blockIdx.x % nsplit, tid = threadIdx.x;
  const int g = qg[b];
  const bool ok = ova_query_ok(qa[b], qp[b], qt[b], g, N, M);
  double mloc = -INFINITY;
  for (int i = tid; i < nby; i += 256) mloc = fmax(mloc, (double)pm[(size_t)i * B + b]);
  const double mx = block_max256(mloc, s_red);   // finite: tile 0 holds column 0
  double sl = 0.0, tl = 0.0;
  for (int i = tid; i < nby; i += 256) {
    const size_t at = (size_t)i * B + b;
    sl += (double)ps[at] * exp((double)pm[at] - mx);
    tl += (double)pt[at];
  }
  const double S = block_sum256(sl, s_red);
  const double T = block_sum256(tl, s_red);
  const double logS = log(S);
  float* row = G + (size_t)b * ldg;
  const int c0 = c * chunk, c1 = min(N, c0 + chunk);
  const bool owner = ok ? (g >= c0 && g < c1) : c == 0;
  if (owner && tid == 0) {
    const float lse = (float)(mx + logS);
    lse_ws[b] = lse;
    if (lse_out) lse_out[b] = lse;
    float term = 0.0f;
    if (ok) {
      const double zg = (double)row[g];
      term = (float)((mx - zg) + logS + (double)eps * (zg - T / (double)N));
    }
    lpart[b] = term;
    if (ok && occ) {   // N3: the rows this query names, counted (k_ova_n3)
      atomicAdd(occ + qa[b], 1);
      atomicAdd(occ + g, 1);
      atomicAdd(occ + N + qp[b], 1);
    }
  }
  __syncthreads();   // z_g is read before any thread rewrites it
  const float fm = (float)mx, fl = (float)logS, inv_b = 1.0f / (float)B;
  const float yn = eps / (float)N, yg = (1.0f - eps) + yn;
  for (int j = c0 + 4 * tid; j < c1; j += 1024) {
    if (j + 4 <= N) {
      float4 v = *reinterpret_cast<const float4*>(row + j);
      float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int u = 0; u < 4; ++u)
        o[u] = ok ? (expf((o[u] - fm) - fl) - (j + u == g ? yg : yn)) * inv_b : 0.0f;
      *reinterpret_cast<float4*>(row + j) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
      for (int u = 0; j + u < N; ++u)
        row[j + u] = ok ? (expf((row[j + u] - fm) - fl) - (j + u == g ? yg : yn)) * inv_b : 0.0f;
    }
  }
}

// |x|_3^3 terms of row x at component k, weight c = n3 / B: the gradient
// 3 |x_k| x_k (DistMult) or 3 |c_j| (re, im) (ComplEx) -- 0, never NaN, at a
// zero component -- and the component's share of the norm (ComplEx: the even
// lane of a pair carries |c_j|^3)
__device__ __forceinline__ float n3_elem(int model, const float* x, int k, float& norm) {
  if (model == SKGE_DISTMULT) {
    const float ax = fabsf(x[k]);
    norm += ax * ax * ax;
    return 3.0f * ax * x[k];
  }
  const float re = x[k & ~1], im = x[k | 1];
  const float mod = sqrtf(fmaf(re, re, im * im));
  if (!(k & 1)) norm += mod * mod * mod;
  return 3.0f * mod * x[k];
}

// The N3 gradient, one wave per table row (E rows, then R rows).  Every
// occurrence of a row adds the same term, c 3 |x_k| x_k with c = n3 / B, so the
// sum over a batch is occ[row] times it: one product per element in place of
// one float atomic per occurrence, and the same bits whatever order the queries
// ran in.  It runs after the DE product's stores and gR's memset and before
// the chain rule's atomics; a row no valid query names is not touched.
__global__ __launch_bounds__(256) void k_ova_n3(int model, const float* __restrict__ E,
                                                const float* __restrict__ R, int N, int M, int d,
                                                const int* __restrict__ occ, float c,
                                                float* __restrict__ gE, float* __restrict__ gR) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), l = lane_id();
  if (row >= N + M) return;
  const int n = occ[row];
  if (n == 0) return;
  const bool ent = row < N;
  const float* x = ent ? E + (size_t)row * d : R + (size_t)(row - N) * d;
  float* g = ent ? gE + (size_t)row * d : gR + (size_t)(row - N) * d;
  const float w = c * (float)n;
  float norm = 0.0f;
  for (int k = l; k < d; k += 64) g[k] = fmaf(w, n3_elem(model, x, k, norm), g[k]);
}

// ---- the chain kernel: one wave per query, one template for both regimes ----
// dq_b into s_dq (kv_dq_sum), then kv_chain_elem's rows into gE[a] and gR[p]
// with float atomics and the mark of R row p.  An invalid query adds nothing
// and marks nothing.  TARGET (1vsAll): the query carries a target g, which
// must be a row of E too, and at n3 > 0 its n3 (|E_a|_3^3 + |R_p|_3^3 +
// |E_g|_3^3) joins its loss partial (the N3 gradient is k_ova_n3's).  Without
// TARGET (KvsAll) qg, n3 and lpart are not read and none of that code exists.
template <bool TARGET>
__global__ __launch_bounds__(256) void k_kv_chain(int model, const float* __restrict__ E,
                                                  const float* __restrict__ R, int N, int M, int d,
                                                  const int* __restrict__ qa,
                                                  const int* __restrict__ qp,
                                                  const int* __restrict__ qt,
                                                  const int* __restrict__ qg, int B,
                                                  const float* __restrict__ part, int ns,
                                                  float n3, float* __restrict__ gE,
                                                  float* __restrict__ gR,
                                                  int* __restrict__ r_touched,
                                                  float* __restrict__ lpart) {
  __shared__ float s_dq[4][KV_DMAX];
  const int w = threadIdx.x >> 6, l = lane_id();
  const int b = blockIdx.x * 4 + w;
  const bool live = b < B;
  const int a = live ? qa[b] : -1, p = live ? qp[b] : -1, t = live ? qt[b] : 0;
  int g = 0;
  bool ok;
  if constexpr (TARGET) {
    g = live ? qg[b] : -1;
    ok = live && ova_query_ok(a, p, t, g, N, M);
  } else {
    ok = live && kv_query_ok(a, p, t, N, M);
  }
  if (ok) kv_dq_sum(part, ns, B, b, d, l, s_dq[w]);
  __syncthreads();
  if (!ok) return;
  const float* ea = E + (size_t)a * d;
  const float* rp = R + (size_t)p * d;
  const float* eg = E + (size_t)g * d;
  float* ge = gE + (size_t)a * d;
  float* gr = gR + (size_t)p * d;
  const float* dq = s_dq[w];
  float norm = 0.0f;
  for (int k = l; k < d; k += 64) {
    float va, vr;
    kv_chain_elem(model, t, dq, ea, rp, k, va, vr);
    if constexpr (TARGET) {
      if (n3 > 0.0f) {
        n3_elem(model, ea, k, norm);
        n3_elem(model, rp, k, norm);
        n3_elem(model, eg, k, norm);
      }
    }
    atomicAdd(ge + k, va);
    atomicAdd(gr + k, vr);
  }
  if constexpr (TARGET) {
    if (n3 > 0.0f) {   // wave-uniform
      norm = wave_sum(norm);
      if (l == 0) lpart[b] += n3 * norm;
    }
  }
  if (l == 0) r_touched[p] = 1;
}

// ==== the host side: one plan, one check, one launch sequence ====
enum { KV_KVSALL = 0, KV_ONEVSALL = 1 };   // the regime

// ---- plan and workspace ----
struct KvPlan {
  size_t ldg;            // G's row pitch: N rounded up to 4 (16-byte rows)
  int wpr;               // bitmap words per query
  unsigned nbx, nby;     // forward tiles
  int kslice, ns;        // DQ slices of the entities
  int nsplit, chunk;     // 1vsAll, k_ova_combine: workgroups per query, columns per workgroup
  size_t o_q, o_g, o_part, o_lpart, o_ge, o_gr, o_touched;   // both regimes
  size_t o_bits;                                             // KvsAll
  size_t o_rowp, o_lse, o_occ;                               // 1vsAll
  size_t total;
};

// A regime's arena holds its own buffers only; lpart is one float per forward
// workgroup (KvsAll) or per query (1vsAll).  Q, G, the partials and the
// gradients lie where each regime has always had them.
static KvPlan kv_plan(int regime, int B, int N, int M, int d) {
  KvPlan p = {};
  p.ldg = ((size_t)N + 3) & ~(size_t)3;
  p.wpr = (int)(((long long)N + 31) / 32);
  p.nbx = (unsigned)((B + KV_T - 1) / KV_T);
  p.nby = (unsigned)(((long long)N + KV_T - 1) / KV_T);
  {   // DQ: about 512 workgroups, the partials at most 16 MB
    const long long tiles = (long long)p.nbx * ((d + KV_T - 1) / KV_T);
    const long long chunks = ((long long)N + KV_KC - 1) / KV_KC;
    const long long cap = std::max<long long>(1, (16ll << 20) / ((long long)B * d * 4));
    const long long want =
        std::max<long long>(1, std::min({chunks, (512 + tiles - 1) / tiles, cap}));
    const long long per = (chunks + want - 1) / want;
    p.kslice = (int)std::min<long long>(per * KV_KC, 1ll << 30);
    p.ns = (int)((chunks + per - 1) / per);
  }
  if (regime == KV_ONEVSALL) {
    // about 1024 workgroups, none with fewer than 1024 columns (but one per query)
    const long long want = std::max<long long>(
        1, std::min<long long>((1024 + B - 1) / B, ((long long)N + 1023) / 1024));
    const long long per = (((long long)N + want - 1) / want + 3) & ~3ll;
    p.chunk = (int)std::min<long long>(per, (1ll << 31) - 4);
    p.nsplit = (int)(((long long)N + p.chunk - 1) / p.chunk);
  }
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align256(bytes);
    return at;
  };
  const bool ova = regime == KV_ONEVSALL;
  p.o_q = take((size_t)B * d * sizeof(float));
  if (!ova) p.o_bits = take((size_t)B * p.wpr * sizeof(unsigned));
  p.o_g = take((size_t)B * p.ldg * sizeof(float));
  p.o_part = take((size_t)p.ns * B * d * sizeof(float));
  if (ova) {
    p.o_rowp = take((size_t)3 * p.nby * B * sizeof(float));
    p.o_lse = take((size_t)B * sizeof(float));
    p.o_occ = take(((size_t)N + M) * sizeof(int));
  }
  p.o_lpart = take((ova ? (size_t)B : (size_t)p.nbx * p.nby) * sizeof(float));
  p.o_ge = take((size_t)N * d * sizeof(float));
  p.o_gr = take((size_t)M * d * sizeof(float));
  p.o_touched = take((size_t)M * sizeof(int));
  p.total = o;
  return p;
}

// what every entry point refuses before any launch; n3 is 1vsAll's (KvsAll: 0)
static int kv_check(const char* who, int regime, int model, int N, int M, int d, int B,
                    float smoothing, float n3) {
  SKGE_CHECK_ARG(model_known(model), "%s: unknown model %d", who, model);
  if (!model_diag(model)) {
    set_error("%s: model %d (%s) is not served: %s scores a query against every entity with "
              "one dot product, which DistMult and ComplEx allow", who, model, model_name(model),
              regime == KV_ONEVSALL ? "1vsAll" : "KvsAll");
    return SKGE_ENOTSUP;
  }
  SKGE_CHECK_ARG(N >= 1 && M >= 1 && d >= 1 && B >= 1, "%s: bad sizes (N = %d, M = %d, d = %d, "
                 "B = %d)", who, N, M, d, B);
  if (B > KV_BMAX || d > KV_DMAX) {
    set_error("%s: B = %d, d = %d outside B <= %d, d <= %d", who, B, d, KV_BMAX, KV_DMAX);
    return SKGE_ENOTSUP;
  }
  SKGE_CHECK_ARG(model != SKGE_COMPLEX || d % 2 == 0, "%s: ComplEx needs an even d (%d)", who, d);
  SKGE_CHECK_ARG(smoothing >= 0.0f && smoothing < 1.0f, "%s: label smoothing %g outside [0, 1)",
                 who, (double)smoothing);
  SKGE_CHECK_ARG(n3 >= 0.0f && std::isfinite(n3), "%s: N3 weight %g is negative or not finite", who,
                 (double)n3);
  return SKGE_OK;
}

static int kv_check_workspace(const char* who, const KvPlan& p, const void* workspace,
                              size_t ws_bytes, int B, int N, int M, int d) {
  SKGE_CHECK_ARG(workspace && ws_bytes >= p.total, "%s: workspace needs %zu bytes (B = %d, "
                 "N = %d, M = %d, d = %d)", who, p.total, B, N, M, d);
  return SKGE_OK;
}

// ---- a batch: the arguments both _grad entry points take, then what kv_open
// derives from them ----
struct KvBatch {
  hipStream_t st;
  int model;
  const float *E, *R;
  int N, M, d;
  const int *qa, *qp, *qt;
  int B;
  float *gE, *gR;
  int* touched;
  float* loss;
  KvPlan p;
  char* ws;
  float *Q, *G, *part, *lpart;   // the workspace parts of both regimes
  unsigned qblocks;              // one wave per query, four to a workgroup
};

// The checks of a _grad entry point `who`, in the order the refusals are
// documented in; own_ok: the regime's own pointer arguments are not NULL.
static int kv_open(KvBatch& b, const char* who, int regime, bool own_ok, float smoothing, float n3,
                   void* workspace, size_t ws_bytes) {
  int rc = kv_check(who, regime, b.model, b.N, b.M, b.d, b.B, smoothing, n3);
  if (rc) return rc;
  SKGE_CHECK_ARG(b.E && b.R && b.qa && b.qp && b.qt && own_ok && b.gE && b.gR && b.touched &&
                     b.loss, "%s: NULL argument", who);
  b.p = kv_plan(regime, b.B, b.N, b.M, b.d);
  if ((rc = kv_check_workspace(who, b.p, workspace, ws_bytes, b.B, b.N, b.M, b.d))) return rc;
  SKGE_CHECK_ARG(((uintptr_t)workspace & 15) == 0 &&
                     (b.d % 4 != 0 || (((uintptr_t)b.E | (uintptr_t)b.R) & 15) == 0),
                 "%s: the workspace and, at d %% 4 == 0, E and R must be 16-byte aligned", who);
  b.ws = (char*)workspace;
  b.Q = (float*)(b.ws + b.p.o_q);
  b.G = (float*)(b.ws + b.p.o_g);
  b.part = (float*)(b.ws + b.p.o_part);
  b.lpart = (float*)(b.ws + b.p.o_lpart);
  b.qblocks = (unsigned)((b.B + 3) / 4);
  return SKGE_OK;
}

// gR and the marks cleared (gE is the DE product's plain stores), then Q
static int kv_queries(const KvBatch& b) {
  SKGE_CHECK_HIP(hipMemsetAsync(b.gR, 0, (size_t)b.M * b.d * sizeof(float), b.st));
  SKGE_CHECK_HIP(hipMemsetAsync(b.touched, 0, (size_t)b.M * sizeof(int), b.st));
  hipLaunchKernelGGL(k_kv_query, dim3(b.qblocks), dim3(256), 0, b.st, b.model, b.E, b.R, b.N, b.M,
                     b.d, b.qa, b.qp, b.qt, b.B, b.Q);
  return SKGE_OK;
}

// Z = Q E^T into G (and scores): the forward's operands; the epilogue's fields
// are the regime's
static KvGemm kv_forward(const KvBatch& b, float* scores) {
  KvGemm f = {};
  f.A = b.Q;
  f.lda = b.d;
  f.B = b.E;
  f.ldb = b.d;
  f.Mr = b.B;
  f.Nc = b.N;
  f.K = b.d;
  f.nbx = b.p.nbx;
  f.G = b.G;
  f.ldg = b.p.ldg;
  f.scores = scores;
  return f;
}

// the two products of G: the slices' partials of dq, and gE
static void kv_backward(const KvBatch& b) {
  const KvPlan& p = b.p;
  KvGemm q = {};   // dq = G E: rows the queries, columns the dims, over the entities
  q.A = b.G;
  q.lda = p.ldg;
  q.B = b.E;
  q.ldb = b.d;
  q.Mr = b.B;
  q.Nc = b.d;
  q.K = b.N;
  q.kslice = p.kslice;
  q.nbx = p.nbx;
  q.C = b.part;
  const unsigned ntd = (unsigned)((b.d + KV_T - 1) / KV_T);
  hipLaunchKernelGGL((k_kv_gemm<false, true, KV_DQ>), dim3(p.nbx * ntd * (unsigned)p.ns),
                     dim3(256), 0, b.st, q);
  KvGemm e = {};   // gE = G^T Q: rows the entities, columns the dims, over the queries
  e.A = b.G;
  e.lda = p.ldg;
  e.B = b.Q;
  e.ldb = b.d;
  e.Mr = b.N;
  e.Nc = b.d;
  e.K = b.B;
  e.nbx = p.nby;
  e.C = b.gE;
  hipLaunchKernelGGL((k_kv_gemm<true, true, KV_DE>), dim3(p.nby * ntd), dim3(256), 0, b.st, e);
}

// A _step entry point `who`: the tables checked, grad(gE, gR, touched) -- the
// regime's _grad into the workspace's own gradient buffers -- and the row
// updates of skge_update.hip.
template <class Grad>
static int kv_step(const char* who, int regime, void* stream, int model, const skge_table_t* ent,
                   const skge_table_t* rel, int d, int B, float smoothing, float n3,
                   void* workspace, size_t ws_bytes, Grad grad) {
  int rc = kv_check(who, regime, model, ent ? ent->rows : 1, rel ? rel->rows : 1, d, B, smoothing,
                    n3);
  if (rc) return rc;
  if ((rc = check_table(ent, "ent", false)) || (rc = check_table(rel, "rel", false))) return rc;
  SKGE_CHECK_ARG(ent->width == d && rel->width == d, "%s: table widths %d / %d, d = %d", who,
                 ent->width, rel->width, d);
  const KvPlan p = kv_plan(regime, B, ent->rows, rel->rows, d);
  if ((rc = kv_check_workspace(who, p, workspace, ws_bytes, B, ent->rows, rel->rows, d))) return rc;
  char* ws = (char*)workspace;
  float* gE = (float*)(ws + p.o_ge);
  float* gR = (float*)(ws + p.o_gr);
  int* touched = (int*)(ws + p.o_touched);
  if ((rc = grad(gE, gR, touched))) return rc;
  hipStream_t st = as_stream(stream);
  if ((rc = launch_update_table(st, ent, gE, nullptr))) return rc;   // every row
  return launch_update_table(st, rel, gR, touched);                   // the rows a query names
}

}  // namespace skge

using namespace skge;

// ---- KvsAll: the answers' bitmap, the BCE epilogue, one loss partial per
// forward workgroup ----
extern "C" size_t skge_kvsall_workspace_bytes(int model, int B, int N, int M, int d) {
  if (kv_check("skge_kvsall_workspace_bytes", KV_KVSALL, model, N, M, d, B, 0.0f, 0.0f) != SKGE_OK)
    return 0;
  return kv_plan(KV_KVSALL, B, N, M, d).total;
}

extern "C" int skge_kvsall_grad(void* stream, int model, const float* E, const float* R, int N,
                                int M, int d, const int* q_anchor, const int* q_rel,
                                const int* q_dir, int B, const int* ans_off, const int* ans_ids,
                                float smoothing, float* gE, float* gR, int* r_touched, float* loss,
                                float* scores, void* workspace, size_t ws_bytes) {
  KvBatch b = {as_stream(stream), model, E, R, N, M, d, q_anchor, q_rel, q_dir, B, gE, gR,
               r_touched, loss};
  int rc = kv_open(b, "skge_kvsall_grad", KV_KVSALL, ans_off && ans_ids, smoothing, 0.0f, workspace,
                   ws_bytes);
  if (rc) return rc;
  const KvPlan& p = b.p;
  unsigned* bits = (unsigned*)(b.ws + p.o_bits);
  SKGE_CHECK_HIP(hipMemsetAsync(bits, 0, (size_t)B * p.wpr * sizeof(unsigned), b.st));
  if ((rc = kv_queries(b))) return rc;
  hipLaunchKernelGGL(k_kv_labels, dim3(b.qblocks), dim3(256), 0, b.st, ans_off, ans_ids, B, N,
                     p.wpr, bits);
  KvGemm f = kv_forward(b, scores);
  f.bits = bits;
  f.wpr = p.wpr;
  f.eps = smoothing;
  f.eps_n = smoothing / (float)N;
  f.inv_b = 1.0f / (float)B;
  f.lpart = b.lpart;
  const unsigned nfwd = p.nbx * p.nby;
  hipLaunchKernelGGL((k_kv_gemm<false, false, KV_FWD>), dim3(nfwd), dim3(256), 0, b.st, f);
  kv_backward(b);
  hipLaunchKernelGGL(k_kv_chain<false>, dim3(b.qblocks), dim3(256), 0, b.st, model, E, R, N, M, d,
                     q_anchor, q_rel, q_dir, nullptr, B, b.part, p.ns, 0.0f, gE, gR, r_touched,
                     nullptr);
  hipLaunchKernelGGL(k_kv_loss, dim3(1), dim3(256), 0, b.st, b.lpart, nfwd, f.inv_b, loss);
  SKGE_CHECK_LAUNCH("kvsall grad");
  return SKGE_OK;
}

extern "C" int skge_kvsall_step(void* stream, int model, const skge_table_t* ent,
                                const skge_table_t* rel, int d, const int* q_anchor,
                                const int* q_rel, const int* q_dir, int B, const int* ans_off,
                                const int* ans_ids, float smoothing, float* loss, void* workspace,
                                size_t ws_bytes) {
  return kv_step("skge_kvsall_step", KV_KVSALL, stream, model, ent, rel, d, B, smoothing, 0.0f,
                 workspace, ws_bytes, [&](float* gE, float* gR, int* touched) {
                   return skge_kvsall_grad(stream, model, ent->param, rel->param, ent->rows,
                                           rel->rows, d, q_anchor, q_rel, q_dir, B, ans_off,
                                           ans_ids, smoothing, gE, gR, touched, loss, nullptr,
                                           workspace, ws_bytes);
                 });
}

// ---- 1vsAll: the softmax partials and their combine, the N3 counts and
// gradient, one loss partial per query ----
extern "C" size_t skge_onevsall_workspace_bytes(int model, int B, int N, int M, int d) {
  if (kv_check("skge_onevsall_workspace_bytes", KV_ONEVSALL, model, N, M, d, B, 0.0f, 0.0f) !=
      SKGE_OK)
    return 0;
  return kv_plan(KV_ONEVSALL, B, N, M, d).total;
}

extern "C" int skge_onevsall_grad(void* stream, int model, const float* E, const float* R, int N,
                                  int M, int d, const int* q_anchor, const int* q_rel,
                                  const int* q_dir, const int* q_target, int B, float smoothing,
                                  float n3, float* gE, float* gR, int* r_touched, float* loss,
                                  float* scores, float* lse, void* workspace, size_t ws_bytes) {
  KvBatch b = {as_stream(stream), model, E, R, N, M, d, q_anchor, q_rel, q_dir, B, gE, gR,
               r_touched, loss};
  int rc = kv_open(b, "skge_onevsall_grad", KV_ONEVSALL, q_target != nullptr, smoothing, n3,
                   workspace, ws_bytes);
  if (rc) return rc;
  const KvPlan& p = b.p;
  float* lse_ws = (float*)(b.ws + p.o_lse);
  int* occ = n3 > 0.0f ? (int*)(b.ws + p.o_occ) : nullptr;
  if (occ) SKGE_CHECK_HIP(hipMemsetAsync(occ, 0, ((size_t)N + M) * sizeof(int), b.st));
  if ((rc = kv_queries(b))) return rc;
  KvGemm f = kv_forward(b, scores);
  const size_t nrow = (size_t)p.nby * B;
  f.pm = (float*)(b.ws + p.o_rowp);
  f.ps = f.pm + nrow;
  f.pt = f.pm + 2 * nrow;
  hipLaunchKernelGGL((k_kv_gemm<false, false, KV_OVA>), dim3(p.nbx * p.nby), dim3(256), 0, b.st, f);
  hipLaunchKernelGGL(k_ova_combine, dim3((unsigned)B * (unsigned)p.nsplit), dim3(256), 0, b.st,
                     b.G, p.ldg, N, M, B, (int)p.nby, p.nsplit, p.chunk, f.pm, f.ps, f.pt, q_anchor,
                     q_rel, q_dir, q_target, smoothing, lse_ws, lse, b.lpart, occ);
  kv_backward(b);
  if (occ)
    hipLaunchKernelGGL(k_ova_n3, dim3((unsigned)(((size_t)N + M + 3) / 4)), dim3(256), 0, b.st,
                       model, E, R, N, M, d, occ, n3 / (float)B, gE, gR);
  hipLaunchKernelGGL(k_kv_chain<true>, dim3(b.qblocks), dim3(256), 0, b.st, model, E, R, N, M, d,
                     q_anchor, q_rel, q_dir, q_target, B, b.part, p.ns, n3, gE, gR, r_touched,
                     b.lpart);
  hipLaunchKernelGGL(k_kv_loss, dim3(1), dim3(256), 0, b.st, b.lpart, (unsigned)B, 1.0f / (float)B,
                     loss);
  SKGE_CHECK_LAUNCH("onevsall grad");
  return SKGE_OK;
}

extern "C" int skge_onevsall_step(void* stream, int model, const skge_table_t* ent,
                                  const skge_table_t* rel, int d, const int* q_anchor,
                                  const int* q_rel, const int* q_dir, const int* q_target, int B,
                                  float smoothing, float n3, float* loss, void* workspace,
                                  size_t ws_bytes) {
  return kv_step("skge_onevsall_step", KV_ONEVSALL, stream, model, ent, rel, d, B, smoothing, n3,
                 workspace, ws_bytes, [&](float* gE, float* gR, int* touched) {
                   return skge_onevsall_grad(stream, model, ent->param, rel->param, ent->rows,
                                             rel->rows, d, q_anchor, q_rel, q_dir, q_target, B,
                                             smoothing, n3, gE, gR, touched, loss, nullptr,
                                             nullptr, workspace, ws_bytes);
                 });
}
