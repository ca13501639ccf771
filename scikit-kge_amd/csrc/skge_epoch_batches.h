// The batches of an epoch, shared by every device epoch runner and by the
// pipelined runner's plan (skge_pipe_plan.h); no HIP header behind it.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace skge {

// batch geometry of StochasticTrainer._optim (skge/base.py:1246-1268):
// nbatches batches of bs = T / nbatches and the remainder, as (start, count)
// (k_triples_of_epoch, skge_tripleloop.hip, re-derives a positive's batch on the device)
struct EpochBatches {
  int64_t bs = 0, maxb = 0;
  std::vector<std::pair<int64_t, int64_t>> batches;
  int size() const { return (int)batches.size(); }
  const std::pair<int64_t, int64_t>& operator[](int k) const { return batches[k]; }
};

inline EpochBatches epoch_batches(int64_t T, int nbatches) {
  EpochBatches b;
  b.bs = T / nbatches;
  for (int64_t s0 = 0; s0 < T; s0 += b.bs) {
    const int64_t c = (s0 + b.bs <= T) ? b.bs : T - s0;
    b.batches.push_back({s0, c});
    b.maxb = std::max(b.maxb, c);
  }
  return b;
}

}  // namespace skge
