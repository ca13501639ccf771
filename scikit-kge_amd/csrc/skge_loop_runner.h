// Host skeleton of the five loop creates (skge_pairloop.hip: pair _ex / _multi,
// sadv; skge_tripleloop.hip: triple _ex / _multi) on top of GraphRunnerCore:
// their shared refusals, LoopRunner's buffers and capture_epoch.  A create
// keeps its bounds, the form it selects, its buffers and its per-batch body.
#pragma once
#include <cstdlib>

#include "skge_graph_runner.h"
#include "skge_hole_fft.h"
#include "skge_sampler.h"

namespace skge {

// an integer switch of the environment; dflt when it is unset
inline int env_flag(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}

// What the pair and triple creates refuse first (the sadv create's model and
// tables are check_sadv's): a NULL table, a bad sampler, an unknown model code,
// complex rows (ComplEx, RotatE) of an odd d.
inline bool check_loop_model(const char* who, const skge_table_t* ent, const skge_table_t* rel,
                             const skge_sampler_t* smp, int model, int d) {
  if (!ent || !rel) set_error("%s: NULL table", who);
  else if (check_sampler(smp, who)) return false;
  else if (!model_known(model)) set_error("%s: unknown model", who);
  else if (model_complex_rows(model) && d % 2)
    set_error("%s: %s needs an even d", who, model_name(model));
  else return true;
  return false;
}

// a table with slot records holds a batch's `need` touched slots
inline bool check_touched(const char* who, const skge_table_t* t, long long need,
                          const char* what) {
  if (!t->acc_touched || need <= t->touched_cap) return true;
  set_error("%s: %s accumulator needs %lld touched slots, has %lld", who, what, need,
            (long long)t->touched_cap);
  return false;
}

// The runner of both loops: the epoch's draw and the per-batch workspace.
struct LoopRunner : GraphRunnerCore {
  int4* rec = nullptr;   // the (1, [0, 1]) draw: records (s, o, p, s') [T] and o' [T]
  int* rec_n1 = nullptr;
  int* pos3 = nullptr;   // the n-negatives draw: positives [T][3] and their slots [T][K]
  int* negK = nullptr;
  void* ws = nullptr;
  size_t ws_bytes = 0;

  // K = 0: the (1, [0, 1]) draw's records; K >= 1: the n-negatives draw's
  void alloc_draw(int64_t T, int K) {
    if (K == 0) {
      rec = (int4*)alloc((size_t)T * sizeof(int4), false);
      rec_n1 = (int*)alloc((size_t)T * sizeof(int), false);
    } else {
      pos3 = (int*)alloc((size_t)T * 3 * sizeof(int), false);
      negK = (int*)alloc((size_t)T * K * sizeof(int), false);
    }
  }

  // zero-filled once: RESCAL's kernels multiply the WE / EW rows and partial scores of
  // an absent negative by a zero coefficient, which only discards FINITE stale values
  void alloc_ws(size_t bytes) {
    ws_bytes = bytes;
    if (bytes) ws = alloc(bytes, true);
  }
};

// the grid of a build kernel over n items, one lane each
inline dim3 build_grid(int64_t n) {
  return dim3((unsigned)std::max((int64_t)1, std::min((n + 255) / 256, (int64_t)4096)));
}

// The gate of both tables in the apply that follows a per-positive kernel:
//   gate_word(g)    the batch's gate word (its violations): the pair creates
//   gate_none()     none, the batch always steps: the sadv create
//   gate_callers()  each table's own, as the caller set it: the triple create
struct GatePolicy {
  bool callers;
  int* word;
};
inline GatePolicy gate_word(int* g) { return {false, g}; }
inline GatePolicy gate_none() { return {false, nullptr}; }
inline GatePolicy gate_callers() { return {true, nullptr}; }

// that apply: nE entity and nR relation slots of the batch
inline int apply_tables(void* stream, const skge_table_t* ent, const skge_table_t* rel,
                        GatePolicy gp, int nE, int nR) {
  skge_table_t t[2] = {*ent, *rel};
  if (!gp.callers) t[0].gate = t[1].gate = gp.word;
  const int ns[2] = {nE, nR};
  return skge_accum_apply(stream, t, 2, ns);
}

// A create's captured epoch, after its alloc calls: a failed allocation and
// HolE's FFT table (made before the capture) are refused, then draw(), build()
// (the explicit pairs / triples, where the form has them), per_batch(k, start,
// count) over the batches and finish() are captured, the first failure
// skipping the rest.  The runner, or NULL and the error text.
template <class R, class Draw, class Build, class Batch, class Finish>
R* capture_epoch(std::unique_ptr<R>& r, const char* who, hipStream_t st, int model, int d,
                 const EpochBatches& batches, Draw draw, Build build, Batch per_batch,
                 Finish finish) {
  if (!r->alloc_ok) return fail("%s: device allocation failed", who);
  if (model == SKGE_HOLE && hole_use_fft(d) && !hole_fft_table(d))
    return fail("%s: HolE FFT twiddle table allocation failed", who);
  if (!r->begin_capture(st)) return nullptr;
  int rc = draw();
  if (!rc) rc = build();
  for (int k = 0; k < batches.size() && !rc; ++k)
    rc = per_batch(k, (long long)batches[k].first, (int)batches[k].second);
  if (!rc) rc = finish();
  return r->end_capture(st, rc) ? r.release() : nullptr;
}

}  // namespace skge
