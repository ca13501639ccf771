// The sorted key lists of the top-k selections (skge_topk.hip,
// skge_neighbours.hip, k_rel_topk_rows of skge_relation.hip) and what every
// selection does with one: offer a tile's candidates to a list kept in LDS
// (list_offer2), write a list out (list_store), decode a finished one
// (list_decode_store).
//
// A list entry is one 64-bit key, (order-preserving bits of the fp32 score)
// << 32 | (0xffffffff - entity id): the larger key is the better entry under
// the contract's order (descending score, then ascending id among exactly
// equal scores), keys are distinct, and key 0 -- below every real key -- is
// an empty slot, which decodes to the padding (-1, -inf).  A wave holds one
// list in registers, slot l in lane l (and slot 64 + l for k > 64), sorted
// descending; inserting a key is one lane shift and two compares per slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace skge {

constexpr int TK_KMAX = 128;

typedef unsigned long long tkey_t;

__device__ __forceinline__ tkey_t make_key(float s, int e) {
  const uint32_t u = __float_as_uint(s == 0.0f ? 0.0f : s);   // -0 and +0 are one score
  const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((tkey_t)o << 32) | (tkey_t)(0xffffffffu - (uint32_t)e);
}
__device__ __forceinline__ int key_entity(tkey_t k) { return (int)(0xffffffffu - (uint32_t)k); }
__device__ __forceinline__ float key_score(tkey_t k) {
  const uint32_t o = (uint32_t)(k >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// the list's k-th entry (slot k - 1): what a candidate has to beat
__device__ __forceinline__ tkey_t list_kth(tkey_t lo, tkey_t hi, int k) {
  return k <= 64 ? __shfl(lo, k - 1) : __shfl(hi, k - 65);
}

// insert key K (distinct from every entry) into the descending list
__device__ __forceinline__ void list_insert(tkey_t& lo, tkey_t& hi, tkey_t K, int k, int l) {
  tkey_t up = __shfl_up(lo, 1);
  if (l == 0) up = ~0ull;
  if (k > 64) {
    tkey_t uph = __shfl_up(hi, 1);
    const tkey_t last = __shfl(lo, 63);
    if (l == 0) uph = last;
    hi = hi > K ? hi : (uph > K ? K : uph);
  }
  lo = lo > K ? lo : (up > K ? K : up);
}

// offer this wave's candidates (one key per lane, 0 = none) to the list;
// xb .. xe: the query's excluded ids, ascending (EXCL)
template <bool EXCL>
__device__ __forceinline__ void list_offer(tkey_t& lo, tkey_t& hi, tkey_t& thr, tkey_t cand, int k,
                                           int l, const int* xb, const int* xe) {
  unsigned long long m = __ballot(cand > thr);
  while (m) {
    const int b = __ffsll((long long)m) - 1;
    m &= m - 1;
    const tkey_t K = __shfl(cand, b);
    if (EXCL) {
      const int e = key_entity(K);
      const int* a = xb;
      const int* z = xe;
      while (a < z) {   // lower bound
        const int* mid = a + ((z - a) >> 1);
        if (*mid < e) a = mid + 1; else z = mid;
      }
      if (a < xe && *a == e) continue;
    }
    list_insert(lo, hi, K, k, l);
    thr = list_kth(lo, hi, k);
    m &= __ballot(cand > thr);
  }
}

// One wave offers two candidates per lane (0 = none) to a list kept in memory
// (LDS), slot l in list[l]: nothing is loaded unless one of them beats the
// k-th entry.  excl_off: the exclusion CSR, row v this list's, or nullptr.
__device__ __forceinline__ void list_offer2(tkey_t* list, tkey_t c0, tkey_t c1, int k, int l,
                                            const int* excl_off, const int* excl_ent, int v) {
  tkey_t thr = list[k - 1];
  if (__ballot(c0 > thr || c1 > thr) == 0) return;
  tkey_t lo = l < k ? list[l] : 0;
  tkey_t hi = 64 + l < k ? list[64 + l] : 0;
  if (excl_off) {
    const int* xb = excl_ent + excl_off[v];
    const int* xe = excl_ent + excl_off[v + 1];
    list_offer<true>(lo, hi, thr, c0, k, l, xb, xe);
    list_offer<true>(lo, hi, thr, c1, k, l, xb, xe);
  } else {
    list_offer<false>(lo, hi, thr, c0, k, l, nullptr, nullptr);
    list_offer<false>(lo, hi, thr, c1, k, l, nullptr, nullptr);
  }
  if (l < k) list[l] = lo;
  if (64 + l < k) list[64 + l] = hi;
}

// one wave copies a list of k keys
__device__ __forceinline__ void list_store(tkey_t* out, const tkey_t* list, int k, int l) {
  if (l < k) out[l] = list[l];
  if (64 + l < k) out[64 + l] = list[64 + l];
}

// a finished list to k (id, score) pairs, the empty slots as (-1, -inf)
__device__ __forceinline__ void list_decode_store(tkey_t lo, tkey_t hi, int k, int l, int* ids,
                                                  float* scores) {
  if (l < k) {
    ids[l] = lo ? key_entity(lo) : -1;
    scores[l] = lo ? key_score(lo) : -INFINITY;
  }
  if (64 + l < k) {
    ids[64 + l] = hi ? key_entity(hi) : -1;
    scores[64 + l] = hi ? key_score(hi) : -INFINITY;
  }
}

}  // namespace skge
