// Device logistic loop for HolE and RESCAL: one epoch of StochasticTrainer
// with RandomModeSampler(1, [0, 1]) (skge/base.py:1242-1316;
// skge/sample.py:28-46), captured once into a hipGraph and replayed.
//
//   k_epoch_sample (skge_pipeline.hip)  the epoch's permutation and every
//       negative, one thread per positive: records (s, o, p, s'), o'
//   k_triples_of_epoch  every batch's labelled triples and ys at once, in the
//       order `xys += samplef(xys)` gives (skge/base.py:1295): batch b of c
//       positives owns 3c positions -- the c positives (y = +1), then positive
//       j's s-corruption at c + 2j and o-corruption at c + 2j + 1 (y = -1); a
//       negative the sampler did not find in ntries draws is a SKIPPED triple
//       in place (relation -1, see skge_triple_grad), so the layout is fixed
//       and only the float add order differs from the reference's list
//   per batch b (the reference's np.split geometry, remainder batch included):
//     skge_triple_step  score + loss + contributions (+ RESCAL dW) + segment
//       mean + updater + projection; the loss added straight into the
//       caller's total.  No gate: a logistic batch always steps.
//   skge_epoch_advance  key + 1
//
// The per-batch kernels are the ones of the explicit-triple API, so a device
// epoch trains exactly like feeding the same triples through
// skge_triple_step.  Exception: HolE where the wave FFT applies scores a
// positive and both of its corruptions in one wave straight from the records
// (k_hole_logistic_pos below): the same triples, contributions and counts,
// 5 forward + 5 inverse transforms per positive instead of 9 + 9.
#include "skge_loop_runner.h"

namespace skge {

__global__ __launch_bounds__(256) void k_triples_of_epoch(const int4* __restrict__ rec,
                                                          const int* __restrict__ rec_n1,
                                                          long long T, long long bs,
                                                          int* __restrict__ trip,
                                                          float* __restrict__ ys) {
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < T;
       j += (long long)gridDim.x * blockDim.x) {
    // (the host's split of the same epoch: epoch_batches, skge_graph_runner.h)
    const long long s0 = (j / bs) * bs;                       // the batch's first positive
    const long long c = s0 + bs <= T ? bs : T - s0, jj = j - s0;
    const int4 r = rec[j];
    const int n1 = rec_n1[j];
    const bool k0 = r.w >= 0, k1 = n1 >= 0;
    const size_t at[3] = {(size_t)(3 * s0 + jj), (size_t)(3 * s0 + c + 2 * jj),
                          (size_t)(3 * s0 + c + 2 * jj + 1)};
    // (a skipped triple keeps the positive's ids: they are never read as rows)
    const int tr[3][3] = {{r.x, r.y, r.z},
                          {k0 ? r.w : r.x, r.y, k0 ? r.z : -1},    // mode 0 corrupts s
                          {r.x, k1 ? n1 : r.y, k1 ? r.z : -1}};    // mode 1 corrupts o
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      int* o = trip + 3 * at[t];
      o[0] = tr[t][0];
      o[1] = tr[t][1];
      o[2] = tr[t][2];
      ys[at[t]] = t == 0 ? 1.0f : -1.0f;
    }
  }
}

// The labelled triples of an epoch drawn with n negatives per positive over any
// modes (k_epoch_sample_multi's pos3 [T][3], negK [T][K]): batch b of c
// positives owns (1 + K) c positions -- the c positives (y = +1), then the
// negative of (positive j, slot k) at c + jK + k (y = -1), the order `xys +=
// samplef(xys)` gives with Sampler.sample's rep-major slots.  One lane per
// (positive, slot); the slot-0 lane writes the positive.  A slot holding -1 is
// a skipped triple in place (it keeps the positive's ids, which are not read).
__global__ __launch_bounds__(256) void k_triples_of_epoch_multi(const int* __restrict__ pos3,
                                                                const int* __restrict__ negK,
                                                                long long T, long long bs,
                                                                Negatives ng,
                                                                int* __restrict__ trip,
                                                                float* __restrict__ ys) {
  const long long total = T * ng.K;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long j = i / ng.K;
    const int k = (int)(i - j * ng.K);
    const long long s0 = (j / bs) * bs;                       // the batch's first positive
    const long long c = s0 + bs <= T ? bs : T - s0, jj = j - s0;
    const size_t base = (size_t)(1 + ng.K) * s0;
    const int s = pos3[3 * j], o = pos3[3 * j + 1], p = pos3[3 * j + 2];
    if (k == 0) {
      int* w = trip + 3 * (base + jj);
      w[0] = s;
      w[1] = o;
      w[2] = p;
      ys[base + jj] = 1.0f;
    }
    const int mode = slot_mode(ng, k);
    const int id = negK[i];
    const bool keep = id >= 0;
    const size_t at = base + c + jj * ng.K + k;
    int* w = trip + 3 * at;
    w[0] = keep && mode == 0 ? id : s;
    w[1] = keep && mode == 1 ? id : o;
    w[2] = !keep ? -1 : mode == 2 ? id : p;
    ys[at] = -1.0f;
  }
}

// ---------------------------------------------------------------------------
// HolE logistic, one positive and BOTH of its corruptions per wave.  Record j =
// (s, o, p, s'), o' gives the labelled triples (s,o,p) y = +1, (s',o,p) and
// (s,o',p) y = -1 (the last two only when kept: k0 = s' >= 0, k1 = o' >= 0).
// The five rows R[p], E[s], E[s'], E[o], E[o'] go through the wave FFT once
// (hole_fft_forward: the three scores as Hermitian sums), fs = -y sigmoid(-y f)
// per triple (hole.py:22-31), and the nine contribution rows of hole.py:32-38
// are summed per destination in the frequency domain, where they are linear
// (u = fp E[s] + f0 E[s']):
//   R[p] : conj(u^) E^o + f1 conj(E^s) E^o'     count 1 + k0 + k1
//   E[s] : conj(R^) (fp E^o + f1 E^o')           count 1 + k1
//   E[o] : R^ u^                                  count 1 + k0
//   E[s']: f0 conj(R^) E^o                        count 1     (k0)
//   E[o']: f1 R^ E^s                              count 1     (k1)
// = 3 + k0 + k1 inverse transforms (hole_fft_rows<false>).  Entity slots
// 4j..4j+3 name (s, o, s', o'), relation slot j names p; coinciding rows
// (s == o, s' == o, o' == s) are separate slots and separate atomic adds of the
// same row, which sum to what the explicit triples give.  A skipped negative's
// row is not loaded (zeros are transformed in its place) and adds nothing.
// LDS per wave: hole_fft_wave_floats(d) (two buffers of five complex rows).
// ---------------------------------------------------------------------------
struct HoleLogArgs {
  const float* E;
  const float* R;
  Accum accE, accR;
  const int4* rec;
  const int* rec_n1;
  long long start;   // this batch: positives [start, start + count)
  int count, d;
  float* loss;       // += the batch's loss
  const float2* tw;  // the twiddle table (hole_fft_table)
};

template <int KM>
__global__ __launch_bounds__(256) void k_hole_logistic_pos(HoleLogArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int wave = threadIdx.x >> 6, wpb = blockDim.x >> 6, l = lane_id();
  const int d = a.d;
  float2* const tw = reinterpret_cast<float2*>(smem);
  fft_twiddles(tw, a.tw, d);
  __syncthreads();
  float* const wb = smem + 2 * d + wave * hole_fft_wave_floats(d);
  const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float lsum = 0.0f;
  for (int j = blockIdx.x * wpb + wave; j < a.count; j += gridDim.x * wpb) {
    const int4 r4 = a.rec[a.start + j];
    const int s = uni(r4.x), o = uni(r4.y), p = uni(r4.z), neg0 = uni(r4.w);
    const int neg1 = uni(a.rec_n1[a.start + j]);
    const int k0 = neg0 >= 0 ? 1 : 0, k1 = neg1 >= 0 ? 1 : 0;
    float4 es[1], eo[1], rp[1], fs[1] = {z4}, fo[1] = {z4};
    load_row4<1>(a.R, p, d, rp);
    load_row4<1>(a.E, s, d, es);
    load_row4<1>(a.E, o, d, eo);
    if (k0) load_row4<1>(a.E, neg0, d, fs);
    if (k1) load_row4<1>(a.E, neg1, d, fo);
    float praw, raw0, raw1;
    const HoleSpec hs = hole_fft_forward(wb, tw, d, rp[0], es[0], fs[0], eo[0], fo[0], praw, raw0,
                                         raw1);
    float lp, fp, l0 = 0.0f, f0 = 0.0f, l1 = 0.0f, f1 = 0.0f;
    logistic(1.0f, praw, &lp, &fp);
    if (k0) logistic(-1.0f, raw0, &l0, &f0);
    if (k1) logistic(-1.0f, raw1, &l1, &f1);
    lsum += (lp + l0) + l1;
    const Accum aR = replica(a.accR, j);
    if (l < 4)
      commit_slot(a.accE, sel4(l, s, o, neg0, neg1), sel4(l, 1 + k1, 1 + k0, k0, k1), 4 * j + l);
    else if (l == 4)
      commit_slot(aR, p, 1 + k0 + k1, j);
    const float* z = hole_fft_rows<false>(wb, tw, d, hs, k0, k1, fp, f0, f1);
    acc_fft_row<KM>(aR, p, z, 2, d);
    acc_fft_row<KM>(a.accE, s, z, 0, d);
    acc_fft_row<KM>(a.accE, o, z, 1, d);
    if (k0) acc_fft_row<KM>(a.accE, neg0, z, 3, d);
    if (k1) acc_fft_row<KM>(a.accE, neg1, z, 3 + k0, d);
    __builtin_amdgcn_wave_barrier();   // the rows are read before the next positive's are put
  }
  __shared__ float lds_loss;
  if (a.loss) block_sum_add(a.loss, lsum, &lds_loss);   // one atomic per workgroup
}

// the per-positive kernel applies: the wave FFT's d (unless SKGE_HOLE_DIRECT=1)
// and tables the per-positive HolE kernels take
static bool hole_logistic_pos_ok(const skge_table_t* ent, const skge_table_t* rel, int d) {
  return hole_use_fft(d) && hole_pos_ok(SKGE_AF_LINEAR, ent, rel, d);
}

// one batch of the HolE device logistic loop (slots: 4 * count entity, count relation)
static int launch_hole_logistic_pos(hipStream_t st, const skge_table_t* ent,
                                    const skge_table_t* rel, int d, const int4* rec,
                                    const int* rec_n1, long long start, int count, float* loss) {
  int rc;
  if ((rc = check_table(ent, "ent", true)) || (rc = check_table(rel, "rel", true)) ||
      (rc = check_slots(ent, 4ll * count, "ent")) || (rc = check_slots(rel, count, "rel")))
    return rc;
  SKGE_CHECK_ARG(hole_logistic_pos_ok(ent, rel, d), "HolE logistic positive kernel: unsupported d or tables");
  HoleLogArgs a = {};
  a.E = ent->param;
  a.R = rel->param;
  a.accE = accum_of(ent);
  a.accR = accum_of(rel);
  a.rec = rec;
  a.rec_n1 = rec_n1;
  a.start = start;
  a.count = count;
  a.d = d;
  a.loss = loss;
  a.tw = hole_fft_table(d);
  SKGE_CHECK_ARG(a.tw != nullptr, "HolE FFT twiddle table allocation failed");
  const int blocks = std::max(1, std::min((count + 3) / 4, 8192));
  const size_t lds = hole_fft_lds_bytes(d, 4);
  switch (km_for(d)) {
    case 1: hipLaunchKernelGGL((k_hole_logistic_pos<1>), dim3(blocks), dim3(256), lds, st, a); break;
    case 2: hipLaunchKernelGGL((k_hole_logistic_pos<2>), dim3(blocks), dim3(256), lds, st, a); break;
    case 3: hipLaunchKernelGGL((k_hole_logistic_pos<3>), dim3(blocks), dim3(256), lds, st, a); break;
    default: hipLaunchKernelGGL((k_hole_logistic_pos<4>), dim3(blocks), dim3(256), lds, st, a); break;
  }
  SKGE_CHECK_LAUNCH("hole logistic positive kernel");
  return SKGE_OK;
}

}  // namespace skge

using namespace skge;

struct skge_triple_runner : LoopRunner {
  int* trip = nullptr;    // the epoch's labelled triples [3T][3], batch b's at 9 * start_b
  float* ys = nullptr;    // [3T]
};

// the shared refusals, then the models without a logistic loss
static bool check_triple_model(const char* who, const skge_table_t* ent, const skge_table_t* rel,
                               const skge_sampler_t* smp, int model, int d) {
  if (!check_loop_model(who, ent, rel, smp, model, d)) return false;
  if (model == SKGE_ROTATE)
    set_error("%s: RotatE is not served here (its scores are <= 0: no logistic loss)", who);
  else if (model != SKGE_HOLE && model != SKGE_RESCAL && !model_diag(model))
    set_error("%s: logistic loss is defined for HolE and RESCAL only (and DistMult and ComplEx)",
              who);
  else return true;
  return false;
}

// the explicit triples' slot map (skge_triple_grad) for a batch of n: 2 entity slots
// per triple; a relation slot per triple (HolE) or per relation (RESCAL's W)
static bool check_triple_touched(const char* who, int model, const skge_table_t* ent,
                                 const skge_table_t* rel, long long n) {
  return check_touched(who, ent, 2 * n, "entity") &&
         (model == SKGE_RESCAL ? check_touched(who, rel, rel->rows, "W")
                               : check_touched(who, rel, n, "relation"));
}

extern "C" skge_triple_runner_t* skge_triple_runner_create_ex(
    void* stream, int model, const skge_table_t* ent, const skge_table_t* rel, int d,
    const int* trip, int64_t T, const void* set, int64_t set_capacity, int nbatches, uint64_t seed,
    uint64_t* epoch_key, int ntries, float* loss_total, const skge_sampler_t* smp) {
  const char* who = "triple runner";
  if (!check_triple_model(who, ent, rel, smp, model, d) ||
      !check_runner_args(who, trip, set, epoch_key, T, INT32_MAX / 3, nbatches, set_capacity, 2 * T,
                         ntries, stream))
    return nullptr;
  hipStream_t st = as_stream(stream);
  const EpochBatches batches = epoch_batches(T, nbatches);
  const int Tmax = (int)(3 * batches.maxb);
  if (!check_triple_touched(who, model, ent, rel, Tmax)) return nullptr;
  // HolE in the wave FFT's range: a positive and both corruptions in one wave
  // straight from the records (SKGE_HOLE_TRIPLES=1 keeps the explicit triples)
  const bool hpos = model == SKGE_HOLE && !env_flag("SKGE_HOLE_TRIPLES", 0) &&
                    hole_logistic_pos_ok(ent, rel, d);
  std::unique_ptr<skge_triple_runner_t> r(new skge_triple_runner_t());
  r->alloc_draw(T, 0);
  if (!hpos) {
    r->trip = (int*)r->alloc((size_t)T * 9 * sizeof(int), false);
    r->ys = (float*)r->alloc((size_t)T * 3 * sizeof(float), false);
  }
  r->alloc_ws(hpos ? 0 : skge_triple_step_workspace_bytes(model, Tmax, rel->rows, d));
  return capture_epoch(
      r, who, st, model, d, batches,
      [&]() -> int {
        return launch_epoch_sample(st, trip, (long long)T, seed, epoch_key,
                                   triple_set_view(set, set_capacity), ent->rows, ntries, r->rec,
                                   r->rec_n1, smp);
      },
      [&]() -> int {
        if (hpos) return SKGE_OK;   // k_hole_logistic_pos reads the records
        hipLaunchKernelGGL(k_triples_of_epoch, build_grid(T), dim3(256), 0, st, r->rec, r->rec_n1,
                           (long long)T, (long long)batches.bs, r->trip, r->ys);
        SKGE_CHECK_LAUNCH("triples launch");
        return SKGE_OK;
      },
      [&](int, long long start, int count) -> int {
        if (!hpos)
          return skge_triple_step(stream, model, ent, rel, d, r->trip + 9 * start,
                                  r->ys + 3 * start, 3 * count, r->ws, r->ws_bytes, loss_total);
        const int rc = launch_hole_logistic_pos(st, ent, rel, d, r->rec, r->rec_n1, start, count,
                                                loss_total);
        return rc ? rc : apply_tables(stream, ent, rel, gate_callers(), 4 * count, count);
      },
      [&]() -> int { return skge_epoch_advance(stream, epoch_key); });
}

extern "C" skge_triple_runner_t* skge_triple_runner_create(
    void* stream, int model, const skge_table_t* ent, const skge_table_t* rel, int d,
    const int* trip, int64_t T, const void* set, int64_t set_capacity, int nbatches, uint64_t seed,
    uint64_t* epoch_key, int ntries, float* loss_total) {
  return skge_triple_runner_create_ex(stream, model, ent, rel, d, trip, T, set, set_capacity,
                                      nbatches, seed, epoch_key, ntries, loss_total, nullptr);
}

// The logistic loop with n negatives per positive over any modes: the same
// epoch (draw, build, one skge_triple_step per batch on (1 + K) * count
// triples, key + 1) and the same runner struct, so run / nlaunches / destroy
// are shared.  HolE runs its explicit-triple kernels: k_hole_logistic_pos is a
// two-negative form by construction.
extern "C" skge_triple_runner_t* skge_triple_runner_create_multi(
    void* stream, int model, const skge_table_t* ent, const skge_table_t* rel, int d,
    const int* trip, int64_t T, const void* set, int64_t set_capacity, int nbatches, uint64_t seed,
    uint64_t* epoch_key, int ntries, float* loss_total, const skge_sampler_t* smp,
    const skge_negatives_t* negs) {
  const char* who = "triple runner";
  int K = 0;
  // triples, their 3 ids and their 2 entity slots are indexed with ints
  if (!check_triple_model(who, ent, rel, smp, model, d) ||
      check_negatives(negs, smp, rel->rows, who, &K) ||
      !check_runner_args(who, trip, set, epoch_key, T, INT32_MAX / (3 * (1 + K)), nbatches,
                         set_capacity, 2 * T, ntries, stream))
    return nullptr;
  hipStream_t st = as_stream(stream);
  const EpochBatches batches = epoch_batches(T, nbatches);
  const int Tmax = (int)((1 + K) * batches.maxb);
  if (!check_triple_touched(who, model, ent, rel, Tmax)) return nullptr;
  std::unique_ptr<skge_triple_runner_t> r(new skge_triple_runner_t());
  r->alloc_draw(T, K);
  r->trip = (int*)r->alloc((size_t)T * (1 + K) * 3 * sizeof(int), false);
  r->ys = (float*)r->alloc((size_t)T * (1 + K) * sizeof(float), false);
  r->alloc_ws(skge_triple_step_workspace_bytes(model, Tmax, rel->rows, d));
  return capture_epoch(
      r, who, st, model, d, batches,
      [&]() -> int {
        return launch_epoch_sample_multi(st, trip, (long long)T, seed, epoch_key,
                                         triple_set_view(set, set_capacity), ent->rows, rel->rows,
                                         ntries, r->pos3, r->negK, smp, negs);
      },
      [&]() -> int {
        hipLaunchKernelGGL(k_triples_of_epoch_multi, build_grid(T * K), dim3(256), 0, st, r->pos3,
                           r->negK, (long long)T, (long long)batches.bs, negatives_of(negs),
                           r->trip, r->ys);
        SKGE_CHECK_LAUNCH("triples launch");
        return SKGE_OK;
      },
      [&](int, long long start, int count) -> int {
        const size_t at = (size_t)(1 + K) * start;
        return skge_triple_step(stream, model, ent, rel, d, r->trip + 3 * at, r->ys + at,
                                (1 + K) * count, r->ws, r->ws_bytes, loss_total);
      },
      [&]() -> int { return skge_epoch_advance(stream, epoch_key); });
}

extern "C" int skge_triple_runner_run(skge_triple_runner_t* r, void* stream, int nepochs) {
  return run_graph(r, stream, nepochs);
}

extern "C" int skge_triple_runner_nlaunches(const skge_triple_runner_t* r) {
  return r ? r->nnodes : -1;
}

extern "C" void skge_triple_runner_destroy(skge_triple_runner_t* r) { delete r; }
