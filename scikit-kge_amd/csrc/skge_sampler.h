// Counter-based randomness of the device batch loop: the keyed epoch
// permutation (the stand-in for numpy's shuffle, skge/base.py:1257), the
// RandomModeSampler draws (skge/sample.py:41-46) and, over the type index'
// pools, the CorruptedSampler and LCWASampler draws (skge/sample.py:68-120).
#pragma once
#include "../../include/skge_hip.h"
#include "skge_device.h"

namespace skge {

// ---- keyed permutation of [0, T): 4-round Feistel + cycle walking ----
struct Perm {
  uint64_t T;
  int half;
  uint64_t key;
};

// half <= 32, so each half fits 32 bits and the round function is fmix32
__device__ __host__ __forceinline__ uint64_t feistel(uint64_t x, int half, uint64_t key) {
  const uint64_t mask = (1ull << half) - 1;
  uint64_t L = x >> half, R = x & mask;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t kr = (uint32_t)(key >> (16 * r)) ^ (0x9E3779B9u * (uint32_t)(r + 1));
    const uint64_t F = (uint64_t)fmix32((uint32_t)R ^ kr) & mask;
    const uint64_t nL = R;
    R = L ^ F;
    L = nL;
  }
  return (L << half) | R;
}

__device__ __host__ __forceinline__ uint64_t perm_index(uint64_t j, const Perm& pm) {
  uint64_t x = j;
  do {
    x = feistel(x, pm.half, pm.key);
  } while (x >= pm.T);
  return x;
}

inline int perm_half(int64_t T) {
  int bits = 1;
  while ((1ll << bits) < T) ++bits;
  return (bits + 1) / 2;
}

__device__ __forceinline__ uint64_t epoch_perm_key(uint64_t seed, uint64_t ek) {
  return mix64(seed ^ mix64(ek * 0xD6E8FEB86659FD93ull + 1));
}

__device__ __forceinline__ uint64_t epoch_sample_key(uint64_t seed, uint64_t ek) {
  return mix64(mix64(seed + 0xA0761D6478BD642Full) ^ (ek * 0xE7037ED1A0B428DBull));
}

// Counter-based draw `randint(n_ent)` for try `tr` of mode `mode` of global
// positive j in the epoch keyed by skey.
__device__ __forceinline__ int draw(uint64_t skey, long long j, int mode, int tr, int n) {
  uint32_t h = fmix32((uint32_t)j * 0x9E3779B1u ^ (uint32_t)skey);
  h = fmix32(h ^ (uint32_t)(skey >> 32) ^ ((uint32_t)((unsigned long long)j >> 32) * 0x85EBCA77u) ^
             ((uint32_t)mode * 0x27D4EB2Fu + (uint32_t)tr * 0x165667B1u));
  return (int)(((uint64_t)h * (uint32_t)n) >> 32);
}

// The record of the epoch's positive j (position j of the keyed permutation):
// (s, o, p, s') and o', each negative the first of ntries draws that is not a
// training triple, or -1 (skge/sample.py:41-46; ntries == 0 draws none).
// k_epoch_sample draws a whole epoch with it; any other place that draws
// records calls this body, so the pairs are the same bits.
__device__ __forceinline__ void sample_record(const int* __restrict__ trip, const Perm& pm,
                                              uint64_t skey, const TripleSet& set, int n_ent,
                                              int ntries, long long j, int4* rec, int* rec_n1) {
  const long long t = (long long)perm_index((uint64_t)j, pm);
  const int s = trip[3 * t], o = trip[3 * t + 1], p = trip[3 * t + 2];
  int neg0 = -1, neg1 = -1;
  for (int tr = 0; tr < ntries; ++tr) {
    const int c = draw(skey, j, 0, tr, n_ent);
    if (!set_contains(set, c, o, p)) {
      neg0 = c;
      break;
    }
  }
  for (int tr = 0; tr < ntries; ++tr) {
    const int c = draw(skey, j, 1, tr, n_ent);
    if (!set_contains(set, s, c, p)) {
      neg1 = c;
      break;
    }
  }
  rec[j] = make_int4(s, o, p, neg0);
  rec_n1[j] = neg1;
}

// ---- the typed and local-closed-world samplers (skge/sample.py:68-120) ----
//
// The type index as a CSR over 2 * n_rel pools: pool 2p + side holds the
// ascending unique entities seen as subject (side 0) or object (side 1) of
// relation p (include/skge_hip.h, skge_sampler_t).
struct Pools {
  const long long* off;   // [2 * n_rel + 1]
  const int* ent;
  int n_rel;
};

enum { SAMPLER_RANDOM = 0, SAMPLER_TYPED = 1, SAMPLER_LCWA = 2 };

// `c in pool [lo, end)` (ascending, unique): for pool 2p the reference's
// counts[(c, p)] > 0 (skge/sample.py:107).  Every load is inside the pool.
__device__ __forceinline__ bool pool_contains(const int* __restrict__ ent, long long lo,
                                              long long end, int c) {
  long long hi = end;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (ent[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && ent[lo] == c;
}

// The typed (KIND == SAMPLER_TYPED) and LCWA samplers' negatives of positive
// (s, o, p) at position j: sample_record's counter use and first-accepted-try
// rule; only what a try draws and what accepts it differ.
//   TYPED, mode m: c = pool[2p + m][draw(skey, j, m, tr, L)], L the pool's
//     length (L == 0 draws nothing), accepted if the corrupted triple is not
//     a training triple (skge/sample.py:82-85).
//   LCWA, mode 0: c = draw(skey, j, 0, tr, n_ent), accepted if c is in pool 2p
//     and (c, o, p) is not a training triple; mode 1 leaves (s, p), which the
//     positive itself counts, so it is sample_record's mode-1 loop.
// One lane per positive, as sample_record: an LCWA try is accepted with
// probability ~|subj(p)| / n_ent, so lanes of a wave leave the loop at
// different tries and the wave runs its slowest lane's count.  The
// wave-cooperative form (lanes test 64 consecutive tries of one positive, a
// ballot picks the lowest) has NOT been built or measured; the choice rests
// on a count of dependent searches only, and the LCWA launch is
// the slow one of the three kinds.
// A relation id outside [0, n_rel) has no pools: no pool negative is drawn.
template <int KIND>
__device__ __forceinline__ void draw_pools(uint64_t skey, const TripleSet& set, const Pools& pl,
                                           int n_ent, int ntries, long long j, int s, int o, int p,
                                           int& neg0, int& neg1) {
  const bool has = p >= 0 && p < pl.n_rel;
  long long b0 = 0, e0 = 0, b1 = 0, e1 = 0;
  if (has) {
    b0 = pl.off[2 * p];
    e0 = b1 = pl.off[2 * p + 1];
    if (KIND == SAMPLER_TYPED) e1 = pl.off[2 * p + 2];
  }
  neg0 = neg1 = -1;
  if (e0 > b0) {
    const int L = (int)(e0 - b0);
    for (int tr = 0; tr < ntries; ++tr) {
      int c;
      if (KIND == SAMPLER_TYPED) {
        c = pl.ent[b0 + draw(skey, j, 0, tr, L)];
      } else {
        c = draw(skey, j, 0, tr, n_ent);
        if (!pool_contains(pl.ent, b0, e0, c)) continue;
      }
      if (!set_contains(set, c, o, p)) {
        neg0 = c;
        break;
      }
    }
  }
  if (KIND == SAMPLER_TYPED) {
    if (e1 > b1) {
      const int L = (int)(e1 - b1);
      for (int tr = 0; tr < ntries; ++tr) {
        const int c = pl.ent[b1 + draw(skey, j, 1, tr, L)];
        if (!set_contains(set, s, c, p)) {
          neg1 = c;
          break;
        }
      }
    }
  } else {
    for (int tr = 0; tr < ntries; ++tr) {
      const int c = draw(skey, j, 1, tr, n_ent);
      if (!set_contains(set, s, c, p)) {
        neg1 = c;
        break;
      }
    }
  }
}

// the record of the epoch's positive j drawn with draw_pools (sample_record's
// layout); the two-launch TransE kernels call draw_pools themselves, one
// positive per wave, so every runner draws the same bits
template <int KIND>
__device__ __forceinline__ void sample_record_pools(const int* __restrict__ trip, const Perm& pm,
                                                    uint64_t skey, const TripleSet& set,
                                                    const Pools& pl, int n_ent, int ntries,
                                                    long long j, int4* rec, int* rec_n1) {
  const long long t = (long long)perm_index((uint64_t)j, pm);
  const int s = trip[3 * t], o = trip[3 * t + 1], p = trip[3 * t + 2];
  int neg0, neg1;
  draw_pools<KIND>(skey, set, pl, n_ent, ntries, j, s, o, p, neg0, neg1);
  rec[j] = make_int4(s, o, p, neg0);
  rec_n1[j] = neg1;
}

// ---- n negatives per positive over any modes (skge/sample.py:10-25) ----
//
// Sampler(n, modes).sample appends, per positive, n repetitions of one
// negative per entry of modes: K = n * nmodes slots, slot k = rep * nmodes +
// mi corrupting position modes[mi] (0: s, 1: o, 2: p).  The device form of
// skge_negatives_t: the modes packed two bits each, so that a lane picks its
// slot's mode with a shift instead of indexing a kernel-argument array.
struct Negatives {
  int K, nmodes;
  uint32_t modes;   // mode of entry mi in bits [2 mi, 2 mi + 2)
  int rel_range;    // TYPED's mode-2 range (skge/sample.py:80)
};

// the device form of a checked skge_negatives_t (check_negatives, skge_host.h)
inline Negatives negatives_of(const skge_negatives_t* negs) {
  uint32_t m = 0;
  for (int i = 0; i < negs->nmodes; ++i) m |= (uint32_t)negs->modes[i] << (2 * i);
  return {negs->n * negs->nmodes, negs->nmodes, m, negs->rel_range};
}

__device__ __forceinline__ int slot_mode(const Negatives& ng, int k) {
  return (int)((ng.modes >> (2 * (k % ng.nmodes))) & 3u);
}

// The corrupted id of slot k of positive (s, o, p) at position j of the
// epoch's order: the first of ntries candidates draw(skey, j, k, tr, range)
// that its kind accepts, or -1.  The draw's field is the SLOT, not the mode:
// at (1, [0, 1]) the two coincide and this is sample_record's (KIND ==
// SAMPLER_RANDOM) or sample_record_pools' draw, bit for bit.
//   mode 0 / 1: as those two draw and accept.
//   mode 2: a relation id p' from [0, n_rel) -- TYPED: from [0, rel_range),
//     the number of relations that occur used as an id range, the reference's
//     quirk -- accepted if (s, o, p') is not a training triple and, LCWA, s is
//     in pool 2p' (counts[(s, p')] > 0, skge/sample.py:106-107).
template <int KIND>
__device__ __forceinline__ int sample_slot(uint64_t skey, const TripleSet& set, const Pools& pl,
                                           int n_ent, int n_rel, const Negatives& ng, int ntries,
                                           long long j, int k, int s, int o, int p) {
  const int mode = slot_mode(ng, k);
  if (mode == 2) {
    const int range = KIND == SAMPLER_TYPED ? ng.rel_range : n_rel;
    for (int tr = 0; tr < ntries; ++tr) {
      const int c = draw(skey, j, k, tr, range);
      if (KIND == SAMPLER_LCWA &&
          !(c < pl.n_rel && pool_contains(pl.ent, pl.off[2 * c], pl.off[2 * c + 1], s)))
        continue;
      if (!set_contains(set, s, o, c)) return c;
    }
    return -1;
  }
  // the pool this slot draws from (TYPED) or tests against (LCWA mode 0)
  long long b = 0, e = 0;
  const bool pooled = KIND == SAMPLER_TYPED || (KIND == SAMPLER_LCWA && mode == 0);
  if (pooled) {
    if (p >= 0 && p < pl.n_rel) {
      b = pl.off[2 * p + (KIND == SAMPLER_TYPED ? mode : 0)];
      e = pl.off[2 * p + (KIND == SAMPLER_TYPED ? mode : 0) + 1];
    }
    if (e <= b) return -1;
  }
  const int range = KIND == SAMPLER_TYPED ? (int)(e - b) : n_ent;
  for (int tr = 0; tr < ntries; ++tr) {
    int c = draw(skey, j, k, tr, range);
    if (KIND == SAMPLER_TYPED) c = pl.ent[b + c];
    else if (pooled && !pool_contains(pl.ent, b, e, c)) continue;
    if (!(mode == 0 ? set_contains(set, c, o, p) : set_contains(set, s, c, p))) return c;
  }
  return -1;
}

}  // namespace skge
