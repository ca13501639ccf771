// Candidate pools: the grouped work list of the pool-restricted ranking and
// top-k entry points (skge_pools.hip; the gathered selection of skge_topk.hip
// reads it too).
//
// The pools are a CSR of ascending, unique entity ids (DeviceKG.pools'
// layout); every query vector names one pool, or -1 for all entities.  The
// vectors are grouped by pool on the device (k_pool_hist / k_pool_scan /
// k_pool_scatter), and an ITEM is one block of up to `bsz` vectors of one
// pool.  A consumer launches dim3(max_items, ns): workgroup (x, y) takes item
// x -- or leaves when x >= *n_items -- and slice y of that pool's candidates.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skge_rank_tile.h"

namespace skge {

struct PoolWork {
  const int4* items;         // (pool or -1, first slot of `order`, vectors, 0)
  const int* n_items;        // device: the items in use
  const int* order;          // [nv] vector ids, grouped by pool
  const int64_t* pool_off;   // [n_pools + 1]
  const int* pool_ent;
  int ns;                    // candidate slices per item (grid.y)
};

// slice y of ns of a pool of `size` candidates, in whole tiles of the score
// tile (skge_rank_tile.h): [ebeg, eend)
// (empty when the pool has fewer tiles than slices)
__device__ __forceinline__ void pool_slice(int size, int ns, int y, int& ebeg, int& eend) {
  const int tiles = (size + RT_EB - 1) / RT_EB;
  const int per = (tiles + ns - 1) / ns;
  const long long b = (long long)y * per * RT_EB;
  ebeg = b < size ? (int)b : size;
  eend = size - ebeg < per * RT_EB ? size : ebeg + per * RT_EB;
}

// the candidates of item `it` under w: the pool's size, and base so that
// candidate e is row (pool < 0 ? e : pool_ent[base + e])
__device__ __forceinline__ int pool_size(const PoolWork& w, int pool, int N, int64_t& base) {
  if (pool < 0) {
    base = 0;
    return N;
  }
  base = w.pool_off[pool];
  return (int)(w.pool_off[pool + 1] - base);
}

// The score tile's mapping (skge_rank_tile.h) of one item: its vectors through
// the order array (s_vec: their ids in LDS for the counting's end, unused by
// the selection); candidate e of the pool is row ent[e] (pool -1: row e)
struct RankPoolRows {
  const int* order;   // the item's first slot
  int vcnt;
  const int* ent;     // the pool's first entry, or nullptr
  const int* s_vec;
  __device__ __forceinline__ int vec(int i) const { return i < vcnt ? order[i] : -1; }
  __device__ __forceinline__ int row(int e) const { return ent ? ent[e] : e; }
  __device__ __forceinline__ int kept(int i) const { return s_vec[i]; }
};

}  // namespace skge
