// Device pair loop for every model: one epoch of PairwiseStochasticTrainer
// with RandomModeSampler(1, [0, 1]) (skge/base.py:1242-1291, 1394-1427;
// skge/sample.py:28-46) or, through skge_pair_runner_create_ex, the typed or
// LCWA sampler (skge_sampler.h), captured once into a hipGraph and replayed.
//
//   k_epoch_sample (skge_pipeline.hip)  the epoch's permutation and every
//       negative, one thread per positive: records (s, o, p, s'), o'
//   k_pairs_of_epoch  every batch's explicit pairs at once, in the reference's
//       order (the records do not depend on the parameters) -- positive j
//       gives pair 2j (s-corrupted) and 2j+1 (o-corrupted); a negative the
//       sampler did not find in ntries draws becomes a SKIPPED pair (positive
//       relation -1, see skge_pair_grad) -- and clears the batches' gate words
//   per batch b (the reference's np.split geometry):
//     skge_pair_step  score + margin test + contributions (+ RESCAL dW) +
//       segment mean + updater + projection, gated on the batch's violations
//       (its own gate word)
//   k_pairs_epoch_end  the gate words' total into the caller's count, key + 1
//
// The per-batch kernels are the ones of the explicit-pair API, so a device
// epoch trains exactly like feeding the same pairs through skge_pair_step.
// Exception: HolE (d % 4 == 0, d <= 256) scores both pairs of a positive in
// one wave straight from the records (k_hole_pos, skge_grad.hip): the same
// pairs, contributions and counts, 7 correlations per positive instead of 12.
// DistMult and ComplEx (d <= 256) do the same with k_diag_pos: 5 row reads per
// positive instead of 12, one accumulator add per distinct row; RotatE with
// k_rot_pos.
#include "skge_loop_runner.h"

namespace skge {

__global__ __launch_bounds__(256) void k_pairs_of_epoch(const int4* __restrict__ rec,
                                                        const int* __restrict__ rec_n1,
                                                        long long T, int* __restrict__ pos,
                                                        int* __restrict__ neg,
                                                        int* __restrict__ gates, int nb,
                                                        int dedup) {
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < T;
       j += (long long)gridDim.x * blockDim.x) {
    if (j < nb) gates[j] = 0;
    if (pos == nullptr) continue;   // per-positive kernels: the records are their input
    const int4 r = rec[j];
    const int n1 = rec_n1[j];
    if (dedup) {   // RESCAL: each positive once ([T][3]), its two negatives ([T][2][3])
      const bool k0 = r.w >= 0, k1 = n1 >= 0;
      int* pp = pos + 3 * (size_t)j;
      int* nn = neg + 6 * (size_t)j;
      pp[0] = r.x;
      pp[1] = r.y;
      pp[2] = (k0 || k1) ? r.z : -1;
      nn[0] = k0 ? r.w : r.x;
      nn[1] = r.y;
      nn[2] = k0 ? r.z : -1;
      nn[3] = r.x;
      nn[4] = k1 ? n1 : r.y;
      nn[5] = k1 ? r.z : -1;
      continue;
    }
    int* pp = pos + 6 * (size_t)j;
    int* nn = neg + 6 * (size_t)j;
    // pair 2j: mode 0 corrupts s; pair 2j+1: mode 1 corrupts o (sample.py:41-46)
    const bool k0 = r.w >= 0, k1 = n1 >= 0;
    pp[0] = r.x;
    pp[1] = r.y;
    pp[2] = k0 ? r.z : -1;
    nn[0] = k0 ? r.w : -1;
    nn[1] = k0 ? r.y : -1;
    nn[2] = k0 ? r.z : -1;
    pp[3] = r.x;
    pp[4] = r.y;
    pp[5] = k1 ? r.z : -1;
    nn[3] = k1 ? r.x : -1;
    nn[4] = k1 ? n1 : -1;
    nn[5] = k1 ? r.z : -1;
  }
}

// The explicit pairs of an epoch drawn with n negatives per positive over any
// modes (k_epoch_sample_multi's pos3 [T][3], negK [T][K]): one lane per
// (positive j, slot k) writes pair jK + k, the order
// PairwiseStochasticTrainer._process_batch appends (skge/base.py:1394-1427:
// per positive, every negative its sampler returned).  Slot k's id replaces s
// (mode 0), o (mode 1) or p (mode 2); a slot holding -1 is a skipped pair in
// place, as k_pairs_of_epoch's.  Clears the batches' gate words.
__global__ __launch_bounds__(256) void k_pairs_of_epoch_multi(const int* __restrict__ pos3,
                                                              const int* __restrict__ negK,
                                                              long long T, Negatives ng,
                                                              int* __restrict__ pos,
                                                              int* __restrict__ neg,
                                                              int* __restrict__ gates, int nb) {
  const long long total = T * ng.K;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    if (i < nb) gates[i] = 0;
    if (pos == nullptr) continue;   // TransE per-positive kernel: the records are its input
    const long long j = i / ng.K;
    const int mode = slot_mode(ng, (int)(i - j * ng.K));
    const int s = pos3[3 * j], o = pos3[3 * j + 1], p = pos3[3 * j + 2];
    const int c = negK[i];
    const bool keep = c >= 0;
    int* pp = pos + 3 * (size_t)i;
    int* nn = neg + 3 * (size_t)i;
    pp[0] = s;
    pp[1] = o;
    pp[2] = keep ? p : -1;
    nn[0] = !keep ? -1 : mode == 0 ? c : s;
    nn[1] = !keep ? -1 : mode == 1 ? c : o;
    nn[2] = !keep ? -1 : mode == 2 ? c : p;
  }
}

__global__ __launch_bounds__(256) void k_pairs_epoch_end(const int* __restrict__ gates, int nb,
                                                         int* nviol_total, uint64_t* ek) {
  __shared__ int part[4];
  int v = 0;
  for (int k = threadIdx.x; k < nb; k += blockDim.x) v += gates[k];
  v = wave_sum_int(v);
  if (lane_id() == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    if (nviol_total) *nviol_total += part[0] + part[1] + part[2] + part[3];
    *ek += 1;
  }
}

}  // namespace skge

using namespace skge;

constexpr int TRANSE_POS_MIN_K = 10;   // k_transe_pos_multi is the default from here on

struct skge_pair_runner : LoopRunner {
  int* pairs = nullptr;   // the epoch's pairs: pos [2T][3], then neg [2T][3]
  int* nviol = nullptr;   // [nbatches]: each batch's gate word (its violations)
  int entity_apply = 0;   // 1: the batches' entity rows go through RESCAL's row-grouped apply
};

// the pair creates' finish
static int launch_pairs_epoch_end(hipStream_t st, const int* gates, int nb, int* nviol_total,
                                  uint64_t* epoch_key) {
  hipLaunchKernelGGL(k_pairs_epoch_end, dim3(1), dim3(256), 0, st, gates, nb, nviol_total,
                     epoch_key);
  SKGE_CHECK_LAUNCH("epoch end launch");
  return SKGE_OK;
}

extern "C" skge_pair_runner_t* skge_pair_runner_create_ex(
    void* stream, int model, int af, const skge_table_t* ent, const skge_table_t* rel, int d,
    const int* trip, int64_t T, const void* set, int64_t set_capacity, int nbatches,
    uint64_t seed, uint64_t* epoch_key, float margin, int ntries, int* nviol_total,
    const skge_sampler_t* smp) {
  const char* who = "pair runner";
  if (!check_loop_model(who, ent, rel, smp, model, d) ||
      !check_runner_args(who, trip, set, epoch_key, T, INT32_MAX, nbatches, set_capacity, 2 * T,
                         ntries, stream))
    return nullptr;
  hipStream_t st = as_stream(stream);
  const EpochBatches batches = epoch_batches(T, nbatches);
  const int bs = (int)batches.bs, nb = batches.size(), Pmax = (int)(2 * batches.maxb);
  // (the relation side is skge_pair_step's own refusal, at the capture)
  if (!check_touched(who, ent, (long long)4 * Pmax, "entity")) return nullptr;
  // HolE with the register-tiled correlations: both pairs of a positive in
  // one wave straight from the records, 4 entity slots and 1 relation slot per
  // positive (SKGE_HOLE_PAIRS=1 keeps the explicit pairs)
  const bool hpos = model == SKGE_HOLE && !env_flag("SKGE_HOLE_PAIRS", 0) &&
                    hole_pos_ok(af, ent, rel, d);
  // RESCAL on the matrix cores: each positive once in the GEMMs and dW, both
  // of its pairs per scatter wave (k_rescal_pos_scatter; SKGE_RESCAL_PAIRS=1
  // keeps the explicit pairs)
  const bool rpos = model == SKGE_RESCAL && !env_flag("SKGE_RESCAL_PAIRS", 0) &&
                    rescal_pair_mfma_selected(d, rel->rows);
  // DistMult / ComplEx: both pairs of a positive in one wave straight from the
  // records (k_diag_pos, skge_grad.hip; SKGE_DIAG_PAIRS=1 keeps the explicit
  // pairs)
  const bool dpos = !env_flag("SKGE_DIAG_PAIRS", 0) && diag_pos_ok(model, af, ent, rel, d);
  // RotatE: the same with k_rot_pos (SKGE_ROT_PAIRS=1 keeps the explicit pairs)
  const bool tpos = !env_flag("SKGE_ROT_PAIRS", 0) && rot_pos_ok(model, ent, rel, d);
  // RESCAL: every batch's relation buckets built once per epoch, up front (the
  // items do not depend on the parameters); SKGE_RESCAL_EPOCH_BUCKETS=0 keeps
  // the per-batch bucketing
  const bool rep = rpos && rescal_epoch_ok(rel->rows) && env_flag("SKGE_RESCAL_EPOCH_BUCKETS", 1);
  std::unique_ptr<skge_pair_runner_t> r(new skge_pair_runner_t());
  r->alloc_draw(T, 0);
  if (!hpos && !dpos && !tpos) r->pairs = (int*)r->alloc((size_t)T * 12 * sizeof(int), false);
  r->nviol = (int*)r->alloc((size_t)nb * sizeof(int), true);
  r->alloc_ws(rep ? rescal_epoch_ws_bytes(bs, nb, rel->rows, d)
                  : skge_pair_step_workspace_bytes(model, Pmax, rel->rows, d));
  int* pos = r->pairs;
  int* neg = r->pairs ? r->pairs + (size_t)T * 6 : nullptr;
  WStep wsync{};   // RESCAL with the in-front W step: synced back at the epoch's end
  return capture_epoch(
      r, who, st, model, d, batches,
      [&]() -> int {
        return launch_epoch_sample(st, trip, (long long)T, seed, epoch_key,
                                   triple_set_view(set, set_capacity), ent->rows, ntries, r->rec,
                                   r->rec_n1, smp);
      },
      [&]() -> int {
        hipLaunchKernelGGL(k_pairs_of_epoch, build_grid(T), dim3(256), 0, st, r->rec, r->rec_n1,
                           (long long)T, pos, neg, r->nviol, nb, rpos ? 1 : 0);
        SKGE_CHECK_LAUNCH("pairs launch");
        return rep ? rescal_epoch_bucket(st, pos, neg, (long long)T, bs, nb, rel->rows, d, r->ws,
                                         r->rec, r->rec_n1)
                   : SKGE_OK;
      },
      [&](int k, long long start, int count) -> int {
        int* gate = r->nviol + k;
        if (hpos || dpos || tpos) {
          const int rc =
              hpos   ? launch_hole_pos(st, af, ent, rel, d, r->rec, r->rec_n1, start, count, margin,
                                       gate, nullptr, nullptr)
              : dpos ? launch_diag_pos(st, model, af, ent, rel, d, r->rec, r->rec_n1, start, count,
                                       margin, gate)
                     : launch_rot_pos(st, ent, rel, d, r->rec, r->rec_n1, start, count, margin, gate);
          return rc ? rc : apply_tables(stream, ent, rel, gate_word(gate), 4 * count, count);
        }
        if (!rpos)
          return skge_pair_step(stream, model, af, ent, rel, d, pos + 6 * start, neg + 6 * start,
                                2 * count, margin, r->ws, r->ws_bytes, gate);
        WStep wst{};   // set by the fused front (Linear): the W step rides the entity apply
        int rc = rep ? skge_rescal_pos_grad_mfma_ep(st, af, ent, rel, d, r->rec, r->rec_n1,
                                                    (long long)T, bs, nb, k, margin, r->ws, gate, &wst)
                     : skge_rescal_pos_grad_mfma(st, af, ent, rel, d, pos + 3 * start,
                                                 neg + 6 * start, r->rec, r->rec_n1, start, count,
                                                 margin, r->ws, r->ws_bytes, gate);
        if (rc) return rc;
        if (wst.applied) {   // the row-grouped apply updated the entity rows and W
          r->entity_apply = 1;
        } else {   // the entity table's apply (and W's, unless the dW kernel updated it)
          skge_table_t te = *ent;
          te.gate = gate;
          const int ns = 4 * count;
          rc = wst.part ? apply_with_wstep(st, &te, ns, wst) : skge_accum_apply(stream, &te, 1, &ns);
        }
        if (wst.cur) wsync = wst;
        return rc;
      },
      [&]() -> int {
        if (wsync.cur)
          if (int rc = rescal_w_sync(st, wsync)) return rc;
        return launch_pairs_epoch_end(st, r->nviol, nb, nviol_total, epoch_key);
      });
}

extern "C" skge_pair_runner_t* skge_pair_runner_create(
    void* stream, int model, int af, const skge_table_t* ent, const skge_table_t* rel, int d,
    const int* trip, int64_t T, const void* set, int64_t set_capacity, int nbatches,
    uint64_t seed, uint64_t* epoch_key, float margin, int ntries, int* nviol_total) {
  return skge_pair_runner_create_ex(stream, model, af, ent, rel, d, trip, T, set, set_capacity,
                                    nbatches, seed, epoch_key, margin, ntries, nviol_total,
                                    nullptr);
}

// The pair loop with n negatives per positive over any modes: the same epoch
// (draw, build, one skge_pair_step per batch on K * count pairs, epoch end)
// and the same runner struct, so run / nlaunches / destroy are shared.  HolE
// and RESCAL run their explicit-pair kernels (k_hole_pos and RESCAL's rpos
// path are two-negative forms by construction).  TransE scores a positive and
// its K negatives in one wave straight from the records (k_transe_pos_multi,
// skge_grad.hip: the same pairs, decisions, sums and counts; 2 + K entity and
// 1 + K relation slots per positive) from K = 10 on; SKGE_TRANSE_PAIRS=1 / =0
// force the explicit pairs / the per-positive kernel.
extern "C" skge_pair_runner_t* skge_pair_runner_create_multi(
    void* stream, int model, int af, const skge_table_t* ent, const skge_table_t* rel, int d,
    const int* trip, int64_t T, const void* set, int64_t set_capacity, int nbatches,
    uint64_t seed, uint64_t* epoch_key, float margin, int ntries, int* nviol_total,
    const skge_sampler_t* smp, const skge_negatives_t* negs) {
  const char* who = "pair runner";
  int K = 0;
  // pairs, their 3 ids and their 4 entity slots are indexed with ints
  if (!check_loop_model(who, ent, rel, smp, model, d) ||
      check_negatives(negs, smp, rel->rows, who, &K) ||
      !check_runner_args(who, trip, set, epoch_key, T, INT32_MAX / (4 * K), nbatches, set_capacity,
                         2 * T, ntries, stream))
    return nullptr;
  hipStream_t st = as_stream(stream);
  const EpochBatches batches = epoch_batches(T, nbatches);
  const int Pmax = (int)(K * batches.maxb), nb = batches.size();
  if (!check_touched(who, ent, (long long)4 * Pmax, "entity") ||
      !check_touched(who, rel, model == SKGE_RESCAL ? rel->rows : (long long)2 * Pmax, "relation"))
    return nullptr;
  // TransE: the per-positive kernel from K = 10 on, where it was measured to
  // win (1.9x at K = 10, 2.2x at K = 20; at K = 2 the two forms tie and the
  // explicit pairs stay).  SKGE_TRANSE_PAIRS=1 forces the explicit
  // pairs, =0 the per-positive kernel, at any K.
  const bool tpos = (model == SKGE_TRANSE_L1 || model == SKGE_TRANSE_L2) &&
                    env_flag("SKGE_TRANSE_PAIRS", K >= TRANSE_POS_MIN_K ? 0 : 1) == 0 &&
                    ent->acc_replicas <= 1;
  std::unique_ptr<skge_pair_runner_t> r(new skge_pair_runner_t());
  r->alloc_draw(T, K);
  if (!tpos) r->pairs = (int*)r->alloc((size_t)T * K * 6 * sizeof(int), false);
  r->nviol = (int*)r->alloc((size_t)nb * sizeof(int), true);
  r->alloc_ws(skge_pair_step_workspace_bytes(model, Pmax, rel->rows, d));
  int* pos = r->pairs;
  int* neg = r->pairs ? r->pairs + (size_t)T * K * 3 : nullptr;
  const Negatives ng = negatives_of(negs);
  return capture_epoch(
      r, who, st, model, d, batches,
      [&]() -> int {
        return launch_epoch_sample_multi(st, trip, (long long)T, seed, epoch_key,
                                         triple_set_view(set, set_capacity), ent->rows, rel->rows,
                                         ntries, r->pos3, r->negK, smp, negs);
      },
      [&]() -> int {
        hipLaunchKernelGGL(k_pairs_of_epoch_multi, build_grid(T * K), dim3(256), 0, st, r->pos3,
                           r->negK, (long long)T, ng, pos, neg, r->nviol, nb);
        SKGE_CHECK_LAUNCH("pairs launch");
        return SKGE_OK;
      },
      [&](int k, long long start, int count) -> int {
        int* gate = r->nviol + k;
        if (tpos) {
          const int rc = launch_transe_pos_multi(st, model == SKGE_TRANSE_L1, ent, rel, d, r->pos3,
                                                 r->negK, start, count, ng, margin, gate);
          return rc ? rc
                    : apply_tables(stream, ent, rel, gate_word(gate), (2 + K) * count,
                                   (1 + K) * count);
        }
        const size_t at = (size_t)3 * K * start;
        return skge_pair_step(stream, model, af, ent, rel, d, pos + at, neg + at, K * count, margin,
                              r->ws, r->ws_bytes, gate);
      },
      [&]() -> int { return launch_pairs_epoch_end(st, r->nviol, nb, nviol_total, epoch_key); });
}

// The self-adversarial loop (TransE-L1 / -L2, RotatE): the
// multi-negative draw, then per batch ONE k_sadv_pos launch straight on the
// records and one apply of both tables, without a gate; the batches' losses
// are added into *loss_total, key + 1 at the epoch's end.  The runner struct
// is the pair loop's, so run / nlaunches / destroy are shared.
extern "C" skge_pair_runner_t* skge_sadv_runner_create(
    void* stream, int model, const skge_table_t* ent, const skge_table_t* rel, int d,
    const int* trip, int64_t T, const void* set, int64_t set_capacity, int nbatches,
    uint64_t seed, uint64_t* epoch_key, float gamma, float alpha, int ntries, float* loss_total,
    const skge_sampler_t* smp, const skge_negatives_t* negs) {
  const char* who = "sadv runner";
  int K = 0;
  // a batch's 2 + K entity slots per positive are indexed with ints
  if (check_sampler(smp, who) ||
      check_sadv(who, model, ent, rel, d, negs, smp, gamma, alpha, &K) ||
      !check_runner_args(who, trip, set, epoch_key, T, INT32_MAX / (2 + K), nbatches, set_capacity,
                         2 * T, ntries, stream))
    return nullptr;
  hipStream_t st = as_stream(stream);
  const EpochBatches batches = epoch_batches(T, nbatches);
  if (!check_touched(who, ent, (long long)(2 + K) * batches.maxb, "entity") ||
      !check_touched(who, rel, (long long)(1 + K) * batches.maxb, "relation"))
    return nullptr;
  std::unique_ptr<skge_pair_runner_t> r(new skge_pair_runner_t());
  r->alloc_draw(T, K);
  const Negatives ng = negatives_of(negs);
  return capture_epoch(
      r, who, st, model, d, batches,
      [&]() -> int {
        return launch_epoch_sample_multi(st, trip, (long long)T, seed, epoch_key,
                                         triple_set_view(set, set_capacity), ent->rows, rel->rows,
                                         ntries, r->pos3, r->negK, smp, negs);
      },
      []() -> int { return SKGE_OK; },   // k_sadv_pos reads the records
      [&](int, long long start, int count) -> int {
        const int rc = launch_sadv_pos(st, model, ent, rel, d, r->pos3, r->negK, start, count, ng,
                                       gamma, alpha, nullptr, nullptr, nullptr, loss_total);
        return rc ? rc
                  : apply_tables(stream, ent, rel, gate_none(), (2 + K) * count, (1 + K) * count);
      },
      [&]() -> int { return skge_epoch_advance(stream, epoch_key); });
}

extern "C" int skge_epoch_sample_multi(void* stream, const int* trip, int64_t T, const void* set,
                                       int64_t set_capacity, int n_ent, int n_rel, uint64_t seed,
                                       const uint64_t* epoch_key, int ntries, int* pos, int* neg,
                                       const skge_sampler_t* smp, const skge_negatives_t* negs) {
  if (int rc = check_sample_args(trip, set, epoch_key, pos, neg, T, set_capacity, n_ent, ntries, 1))
    return rc;
  return launch_epoch_sample_multi(as_stream(stream), trip, (long long)T, seed, epoch_key,
                                   triple_set_view(set, set_capacity), n_ent, n_rel, ntries, pos,
                                   neg, smp, negs);
}

extern "C" int skge_epoch_sample_ex(void* stream, const int* trip, int64_t T, const void* set,
                                    int64_t set_capacity, int n_ent, uint64_t seed,
                                    const uint64_t* epoch_key, int ntries, int* rec, int* rec_n1,
                                    const skge_sampler_t* smp) {
  if (int rc = check_sample_args(trip, set, epoch_key, rec, rec_n1, T, set_capacity, n_ent,
                                 ntries, 1))
    return rc;
  if (int rc = check_sampler(smp, "epoch sample")) return rc;
  return launch_epoch_sample(as_stream(stream), trip, (long long)T, seed, epoch_key,
                             triple_set_view(set, set_capacity), n_ent, ntries, (int4*)rec,
                             rec_n1, smp);
}

extern "C" int skge_epoch_sample(void* stream, const int* trip, int64_t T, const void* set,
                                 int64_t set_capacity, int n_ent, uint64_t seed,
                                 const uint64_t* epoch_key, int ntries, int* rec, int* rec_n1) {
  return skge_epoch_sample_ex(stream, trip, T, set, set_capacity, n_ent, seed, epoch_key, ntries,
                              rec, rec_n1, nullptr);
}

extern "C" int skge_pair_runner_run(skge_pair_runner_t* r, void* stream, int nepochs) {
  return run_graph(r, stream, nepochs);
}

extern "C" int skge_pair_runner_nlaunches(const skge_pair_runner_t* r) {
  return r ? r->nnodes : -1;
}

extern "C" int skge_pair_runner_entity_apply(const skge_pair_runner_t* r) {
  return r ? r->entity_apply : -1;
}

extern "C" void skge_pair_runner_destroy(skge_pair_runner_t* r) { delete r; }
