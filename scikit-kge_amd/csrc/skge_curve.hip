// Segmented curve statistics of a labelled score array (skge_curve_stats;
// DESIGN.md 3.10): per segment the ROC numerator 2U, the PR trapezoid, the
// average precision and the accuracy-maximising threshold, from ONE descending
// sort of (segment, score), a scan and a reduction.
//   k_cs_keys        key = segment << 32 | ~ordered(score): ascending keys are
//                    segments ascending, scores descending; -0.0 becomes +0.0,
//                    a NaN sets status bit 1, a segment id out of range bit 2
//   (rocPRIM)        device radix sort of the keys with the labels as values:
//                    the one step that is not the project's own
//   k_cs_tile_sum / k_cs_tile_scan / k_cs_groups
//                    scan of (true labels, tie-group ends) packed in one
//                    uint64, in tiles of 2048 with carries; every group end
//                    writes its record: cumulative true labels, last index, key
//   k_cs_bounds      the group range [gb, ge) of every segment
//   k_cs_reduce      workgroup (segment, y of Y): the segment's terms, thread t
//                    of part y takes groups gb + 256 y + t + 256 Y j, j
//                    ascending; then the LDS tree 128, 64 .. 1
//   k_cs_final       the Y parts added in y order, and the outputs
// Integers (P, Nneg, 2U, best_correct) are exact; the doubles use IEEE
// division and the fixed tree above (Y depends on n and nseg only), so two runs
// give equal bytes.  A tie group or a segment may span any number of tiles:
// groups are found by comparing neighbouring keys across tile edges, and the
// cumulative counts come from the global scan.
#include <algorithm>
#include <limits.h>
#include <math.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "skge_host.h"

namespace skge {

constexpr int CS_IPT = 8;               // items per thread of a scan tile
constexpr int CS_TILE = 256 * CS_IPT;   // items per scan tile
constexpr int CS_NAN = 1, CS_BADSEG = 2;

struct CsPart {
  long long twoU;
  double pr, ap;
  long long bestv, bestk;   // max TP_k - FP_k and the smallest cut k that reaches it (0: none)
};

__device__ __forceinline__ uint32_t cs_inv_key(float f) {
#ifndef SKGE_MUTANT_NO_ZERO_CANON   // tools/mutants_linkpred.sh
  if (f == 0.0f) f = 0.0f;   // -0.0 and +0.0 are one score
#endif
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  const uint32_t ord = u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);   // ascending with the float
  return ~ord;
}
__device__ __forceinline__ float cs_key_score(uint64_t key) {
  const uint32_t ord = ~(uint32_t)key;
  const uint32_t u = (ord >> 31) ? ord ^ 0x80000000u : ~ord;
  return __builtin_bit_cast(float, u);
}

__global__ __launch_bounds__(256) void k_cs_keys(const float* __restrict__ score,
                                                 const int* __restrict__ seg, long long n,
                                                 int nseg, uint64_t* __restrict__ keys,
                                                 int* __restrict__ status) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const float f = score[i];
    int s = seg ? seg[i] : 0;
    if (f != f) atomicOr(status, CS_NAN);
    if (s < 0 || s >= nseg) {
      atomicOr(status, CS_BADSEG);
      s = 0;
    }
    keys[i] = (uint64_t)(uint32_t)s << 32 | cs_inv_key(f);
  }
}

// (label > 0) << 32 | (element i ends its group of equal keys)
__device__ __forceinline__ uint64_t cs_item(const uint64_t* __restrict__ keys,
                                            const signed char* __restrict__ lab, long long i,
                                            long long n) {
#ifdef SKGE_MUTANT_TIES_NOT_GROUPED
  const uint64_t end = 1;
#else
  const uint64_t end = (i == n - 1 || keys[i + 1] != keys[i]) ? 1 : 0;
#endif
  return (uint64_t)(lab[i] > 0 ? 1 : 0) << 32 | end;
}

__global__ __launch_bounds__(256) void k_cs_tile_sum(const uint64_t* __restrict__ keys,
                                                     const signed char* __restrict__ lab,
                                                     long long n, uint64_t* __restrict__ tile_tot) {
  __shared__ uint64_t s[256];
  const int tid = threadIdx.x;
  const long long i0 = (long long)blockIdx.x * CS_TILE + (long long)tid * CS_IPT;
  uint64_t x = 0;
  for (int j = 0; j < CS_IPT; ++j)
    if (i0 + j < n) x += cs_item(keys, lab, i0 + j, n);
  s[tid] = x;
  __syncthreads();
  for (int st = 128; st >= 1; st >>= 1) {
    if (tid < st) s[tid] += s[tid + st];
    __syncthreads();
  }
  if (tid == 0) tile_tot[blockIdx.x] = s[0];
}

// one workgroup: exclusive scan of the tile totals into the tiles' carries
// (thread t owns a run of tiles, k_pool_scan's form) and the group count
__global__ __launch_bounds__(256) void k_cs_tile_scan(const uint64_t* __restrict__ tile_tot,
                                                      long long ntiles,
                                                      uint64_t* __restrict__ tile_off,
                                                      int* __restrict__ gcount) {
  __shared__ uint64_t s[256];
  const int tid = threadIdx.x;
  const long long per = (ntiles + 255) / 256;
  const long long b0 = tid * per < ntiles ? tid * per : ntiles;
  const long long b1 = b0 + per < ntiles ? b0 + per : ntiles;
  uint64_t x = 0;
  for (long long b = b0; b < b1; ++b) x += tile_tot[b];
  s[tid] = x;
  __syncthreads();
  if (tid == 0) {
    uint64_t c = 0;
    for (int t = 0; t < 256; ++t) {
      const uint64_t v = s[t];
      s[t] = c;
      c += v;
    }
    *gcount = (int)(uint32_t)c;
  }
  __syncthreads();
  uint64_t c = s[tid];
  for (long long b = b0; b < b1; ++b) {
    tile_off[b] = c;
    c += tile_tot[b];
  }
#ifdef SKGE_MUTANT_DROP_LAST_CARRY   // stays in bounds: group indices only shrink
  __syncthreads();
  if (tid == 0 && ntiles > 1) tile_off[ntiles - 1] = 0;
#endif
}

// the scan's second pass: every group end writes its record at its group index
__global__ __launch_bounds__(256) void k_cs_groups(const uint64_t* __restrict__ keys,
                                                   const signed char* __restrict__ lab,
                                                   long long n,
                                                   const uint64_t* __restrict__ tile_off,
                                                   int* __restrict__ gTP, int* __restrict__ gIdx,
                                                   uint64_t* __restrict__ gkey) {
  __shared__ uint64_t s[256];
  const int tid = threadIdx.x;
  const long long i0 = (long long)blockIdx.x * CS_TILE + (long long)tid * CS_IPT;
  uint64_t it[CS_IPT], x = 0;
  for (int j = 0; j < CS_IPT; ++j) {
    it[j] = i0 + j < n ? cs_item(keys, lab, i0 + j, n) : 0;
    x += it[j];
  }
  s[tid] = x;
  __syncthreads();
  for (int st = 1; st < 256; st <<= 1) {   // inclusive scan of the threads' totals
    const uint64_t y = tid >= st ? s[tid - st] : 0;
    __syncthreads();
    s[tid] += y;
    __syncthreads();
  }
  uint64_t run = tile_off[blockIdx.x] + s[tid] - x;
  for (int j = 0; j < CS_IPT; ++j) {
    run += it[j];
    if (it[j] & 1) {
      const long long g = (long long)(uint32_t)run - 1;
      if (g >= 0 && g < n) {   // always true; keeps a wrong carry inside the arrays
        gTP[g] = (int)(run >> 32);
        gIdx[g] = (int)(i0 + j);
        gkey[g] = keys[i0 + j];
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_cs_bounds(const uint64_t* __restrict__ gkey,
                                                   const int* __restrict__ gcount, int nseg,
                                                   int* __restrict__ seg_gb,
                                                   int* __restrict__ seg_ge) {
  const int G = *gcount;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x) {
    const uint32_t s = (uint32_t)(gkey[g] >> 32);
    if (s >= (uint32_t)nseg) continue;
    if (g == 0 || (uint32_t)(gkey[g - 1] >> 32) != s) seg_gb[s] = g;
    if (g == G - 1 || (uint32_t)(gkey[g + 1] >> 32) != s) seg_ge[s] = g + 1;
  }
}

// a segment's counts before its first group
__device__ __forceinline__ void cs_base(const int* gTP, const int* gIdx, int gb, long long& tp,
                                        long long& cnt) {
  tp = gb > 0 ? gTP[gb - 1] : 0;
  cnt = gb > 0 ? (long long)gIdx[gb - 1] + 1 : 0;
}

__global__ __launch_bounds__(256) void k_cs_reduce(const int* __restrict__ gTP,
                                                   const int* __restrict__ gIdx,
                                                   const int* __restrict__ seg_gb,
                                                   const int* __restrict__ seg_ge,
                                                   const int* __restrict__ status,
                                                   CsPart* __restrict__ part) {
  __shared__ CsPart sp[256];
  if (*status) return;
  const int sg = blockIdx.x, y = blockIdx.y, Y = gridDim.y, tid = threadIdx.x;
  const int gb = seg_gb[sg], ge = seg_ge[sg];
  long long btp, bcnt;
  cs_base(gTP, gIdx, gb, btp, bcnt);
  const long long P = ge > gb ? gTP[ge - 1] - btp : 0;
  CsPart a = {0, 0.0, 0.0, 0, 0};
  for (long long g = (long long)gb + 256ll * y + tid; g < ge; g += 256ll * Y) {
    const long long tpk = gTP[g] - btp, ck = (long long)gIdx[g] + 1 - bcnt, fpk = ck - tpk;
    long long tpp = 0, cp = 0;
    if (g > gb) {
      tpp = gTP[g - 1] - btp;
      cp = (long long)gIdx[g - 1] + 1 - bcnt;
    }
    const long long fpp = cp - tpp, dtp = tpk - tpp;
    a.twoU += (fpk - fpp) * (tpk + tpp);
    if (dtp > 0) {   // a group without a true label adds exactly 0
      const double pk = (double)tpk / (double)ck;
      const double pp = cp > 0 ? (double)tpp / (double)cp : 1.0;
      const double w = (double)dtp / (double)P;
      a.pr += w * ((pk + pp) * 0.5);
      a.ap += w * pk;
    }
    const long long v = tpk - fpk, k = g - gb + 1;
    if (v > a.bestv) {   // k ascends within a thread: the first maximum stays
      a.bestv = v;
      a.bestk = k;
    }
  }
  sp[tid] = a;
  __syncthreads();
  for (int st = 128; st >= 1; st >>= 1) {
    if (tid < st) {
      const CsPart b = sp[tid + st];
      CsPart c = sp[tid];
      c.twoU += b.twoU;
      c.pr += b.pr;
      c.ap += b.ap;
      if (b.bestv > c.bestv || (b.bestv == c.bestv && b.bestk != 0 && b.bestk < c.bestk)) {
        c.bestv = b.bestv;
        c.bestk = b.bestk;
      }
      sp[tid] = c;
    }
    __syncthreads();
  }
  if (tid == 0) part[(size_t)sg * Y + y] = sp[0];
}

__global__ __launch_bounds__(256) void k_cs_final(const int* __restrict__ gTP,
                                                  const int* __restrict__ gIdx,
                                                  const uint64_t* __restrict__ gkey,
                                                  const int* __restrict__ seg_gb,
                                                  const int* __restrict__ seg_ge,
                                                  const int* __restrict__ status,
                                                  const CsPart* __restrict__ part, int nseg, int Y,
                                                  long long* __restrict__ counts,
                                                  double* __restrict__ areas,
                                                  float* __restrict__ thresh) {
  if (*status) return;
  for (int sg = blockIdx.x * blockDim.x + threadIdx.x; sg < nseg; sg += gridDim.x * blockDim.x) {
    const int gb = seg_gb[sg], ge = seg_ge[sg];
    long long btp, bcnt;
    cs_base(gTP, gIdx, gb, btp, bcnt);
    const long long P = ge > gb ? gTP[ge - 1] - btp : 0;
    const long long tot = ge > gb ? (long long)gIdx[ge - 1] + 1 - bcnt : 0;
    const long long Nn = tot - P;
    CsPart a = part[(size_t)sg * Y];
    for (int y = 1; y < Y; ++y) {
      const CsPart b = part[(size_t)sg * Y + y];
      a.twoU += b.twoU;
      a.pr += b.pr;
      a.ap += b.ap;
      if (b.bestv > a.bestv || (b.bestv == a.bestv && b.bestk != 0 && b.bestk < a.bestk)) {
        a.bestv = b.bestv;
        a.bestk = b.bestk;
      }
    }
    counts[4 * (size_t)sg] = P;
    counts[4 * (size_t)sg + 1] = Nn;
    counts[4 * (size_t)sg + 2] = a.twoU;
    counts[4 * (size_t)sg + 3] = a.bestv + Nn;
    const bool defined = P > 0 && Nn > 0;
    areas[2 * (size_t)sg] = defined ? a.pr : (double)NAN;
    areas[2 * (size_t)sg + 1] = defined ? a.ap : (double)NAN;
    thresh[sg] = a.bestk > 0 ? cs_key_score(gkey[gb + a.bestk - 1]) : INFINITY;
  }
}

// parts per segment: about 2048 workgroups, a function of nseg alone
static int cs_parts(int nseg) { return std::max(1, std::min(256, (2048 + nseg - 1) / nseg)); }

static unsigned cs_end_bit(int nseg) {
  unsigned b = 0;
  while (b < 31 && ((long long)1 << b) < nseg) ++b;
  return 32 + b;
}

static hipError_t cs_sort(void* tmp, size_t& bytes, const uint64_t* kin, uint64_t* kout,
                          const signed char* vin, signed char* vout, long long n, int nseg,
                          hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, (size_t)n, 0u,
                                   cs_end_bit(nseg), st);
}

struct CsLayout {
  size_t keys_a, keys_b, lab_b, gtp, gidx, ttot, toff, sgb, sge, part, gcount, tmp, tmp_bytes, total;
};

static bool cs_layout(long long n, int nseg, CsLayout* L) {
  const long long ntiles = (n + CS_TILE - 1) / CS_TILE;
  size_t tmp = 0;
  if (n > 0 && cs_sort(nullptr, tmp, nullptr, nullptr, nullptr, nullptr, n, nseg, 0) != hipSuccess)
    return false;
  size_t o = 0;
  auto take = [&](size_t b) {
    const size_t at = o;
    o += align256(b);
    return at;
  };
  L->keys_a = take((size_t)n * 8);
  L->keys_b = take((size_t)n * 8);
  L->lab_b = take((size_t)n);
  L->gtp = take((size_t)n * 4);
  L->gidx = take((size_t)n * 4);
  L->ttot = take((size_t)ntiles * 8);
  L->toff = take((size_t)ntiles * 8);
  L->sgb = take((size_t)nseg * 4);
  L->sge = take((size_t)nseg * 4);
  L->part = take((size_t)nseg * cs_parts(nseg) * sizeof(CsPart));
  L->gcount = take(4);
  L->tmp = take(tmp);
  L->tmp_bytes = tmp;
  L->total = o + 256;
  return true;
}

static bool cs_sizes_ok(long long n, int nseg) {
  return n >= 0 && n <= INT_MAX - CS_TILE && nseg >= 1;
}

}  // namespace skge

using namespace skge;

extern "C" size_t skge_curve_stats_workspace_bytes(int64_t n, int nseg) {
  CsLayout L;
  if (!cs_sizes_ok(n, nseg) || !cs_layout(n, nseg, &L)) return 0;
  return L.total;
}

extern "C" int skge_curve_stats(void* stream, const float* score, const signed char* label,
                                const int* seg, int64_t n, int nseg, void* workspace,
                                size_t ws_bytes, long long* counts_out, double* areas_out,
                                float* thresh_out, int* status_out) {
  SKGE_CHECK_ARG(n >= 0 && n <= INT_MAX - CS_TILE, "n = %lld outside 0 .. %d", (long long)n,
                 INT_MAX - CS_TILE);
  SKGE_CHECK_ARG(nseg >= 1, "nseg = %d: at least one segment", nseg);
  SKGE_CHECK_ARG(counts_out && areas_out && thresh_out && status_out, "NULL argument (outputs)");
  SKGE_CHECK_ARG(n == 0 || (score && label), "NULL argument (score, label)");
  SKGE_CHECK_ARG(workspace, "NULL argument (workspace)");
  CsLayout L;
  SKGE_CHECK_ARG(cs_layout(n, nseg, &L), "curve statistics: the sort's workspace query failed");
  SKGE_CHECK_ARG(ws_bytes >= L.total, "curve statistics workspace needs %zu bytes", L.total);
  hipStream_t st = as_stream(stream);
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  uint64_t* keys_a = (uint64_t*)(ws + L.keys_a);
  uint64_t* keys_b = (uint64_t*)(ws + L.keys_b);
  signed char* lab_b = (signed char*)(ws + L.lab_b);
  int* gTP = (int*)(ws + L.gtp);
  int* gIdx = (int*)(ws + L.gidx);
  uint64_t* ttot = (uint64_t*)(ws + L.ttot);
  uint64_t* toff = (uint64_t*)(ws + L.toff);
  int* sgb = (int*)(ws + L.sgb);
  int* sge = (int*)(ws + L.sge);
  CsPart* part = (CsPart*)(ws + L.part);
  int* gcount = (int*)(ws + L.gcount);
  const int Y = cs_parts(nseg);
  SKGE_CHECK_HIP(hipMemsetAsync(status_out, 0, sizeof(int), st));
  SKGE_CHECK_HIP(hipMemsetAsync(gcount, 0, sizeof(int), st));
  // sgb and sge are neighbours in the workspace: one clear (an empty segment: gb = ge = 0)
  SKGE_CHECK_HIP(hipMemsetAsync(sgb, 0, (L.sge - L.sgb) + (size_t)nseg * 4, st));
  if (n > 0) {
    const int eb = (int)std::min<long long>((n + 255) / 256, 4096);
    const int ntiles = (int)((n + CS_TILE - 1) / CS_TILE);
    hipLaunchKernelGGL(k_cs_keys, dim3(eb), dim3(256), 0, st, score, seg, (long long)n, nseg,
                       keys_a, status_out);
    size_t tmp = L.tmp_bytes;
    SKGE_CHECK_HIP(cs_sort(ws + L.tmp, tmp, keys_a, keys_b, label, lab_b, n, nseg, st));
    hipLaunchKernelGGL(k_cs_tile_sum, dim3(ntiles), dim3(256), 0, st, keys_b, lab_b, (long long)n,
                       ttot);
    hipLaunchKernelGGL(k_cs_tile_scan, dim3(1), dim3(256), 0, st, ttot, (long long)ntiles, toff,
                       gcount);
    // the group records' keys take the unsorted keys' place
    hipLaunchKernelGGL(k_cs_groups, dim3(ntiles), dim3(256), 0, st, keys_b, lab_b, (long long)n,
                       toff, gTP, gIdx, keys_a);
    hipLaunchKernelGGL(k_cs_bounds, dim3(eb), dim3(256), 0, st, keys_a, gcount, nseg, sgb, sge);
  }
  hipLaunchKernelGGL(k_cs_reduce, dim3(nseg, Y), dim3(256), 0, st, gTP, gIdx, sgb, sge, status_out,
                     part);
  hipLaunchKernelGGL(k_cs_final, dim3(std::min((nseg + 255) / 256, 4096)), dim3(256), 0, st, gTP,
                     gIdx, keys_a, sgb, sge, status_out, part, nseg, Y, counts_out, areas_out,
                     thresh_out);
  SKGE_CHECK_LAUNCH("curve statistics");
  return SKGE_OK;
}
