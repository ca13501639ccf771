// The sorted key lists of the top-k selections (skge_topk.hip,
// skge_neighbours.hip).
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

}  // namespace skge
