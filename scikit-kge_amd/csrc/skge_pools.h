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

namespace skge {

constexpr int POOL_TILE = 128;   // candidate rows per LDS tile (RT_EB, TK_EB)

struct PoolWork {
  const int4* items;         // (pool or -1, first slot of `order`, vectors, 0)
  const int* n_items;        // device: the items in use
  const int* order;          // [nv] vector ids, grouped by pool
  const int64_t* pool_off;   // [n_pools + 1]
  const int* pool_ent;
  int ns;                    // candidate slices per item (grid.y)
};

// slice y of ns of a pool of `size` candidates, in whole tiles: [ebeg, eend)
// (empty when the pool has fewer tiles than slices)
__device__ __forceinline__ void pool_slice(int size, int ns, int y, int& ebeg, int& eend) {
  const int tiles = (size + POOL_TILE - 1) / POOL_TILE;
  const int per = (tiles + ns - 1) / ns;
  const long long b = (long long)y * per * POOL_TILE;
  ebeg = b < size ? (int)b : size;
  eend = size - ebeg < per * POOL_TILE ? size : ebeg + per * POOL_TILE;
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

}  // namespace skge
