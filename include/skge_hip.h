/*
 * skge_hip.h -- C ABI of libskgehip.so, the MI355X (gfx950) HIP implementation
 * of scikit-kge's mini-batch training hot path (score + gradient + update).
 *
 * The reference is pure Python/NumPy; its "FFI" for this path is the duck-typed
 * model / updater / trainer protocol of skge.  Each
 * entry point below replaces one piece of that protocol; the Python facade
 * (scikit-kge_amd/skge_amd) binds them with ctypes and keeps the reference's
 * class names, kwargs and return shapes.
 *
 * Conventions
 *  - Ownership: the caller allocates every buffer (device memory, e.g. torch
 *    tensors).  The library never frees caller memory.
 *  - Async: every call is stream-ordered on the caller's hipStream_t (passed as
 *    void*; NULL = the legacy default stream).  No call synchronises, allocates
 *    or copies to the host, so sequences of calls can be captured in a hipGraph.
 *  - Errors: int return, 0 = OK, <0 = error (SKGE_E*); the message of the
 *    last failure on the calling thread is returned by skge_last_error().
 *  - Triples are (s, o, p) int32 triplets, row-major [n][3]
 *    (skge/base.py:511, skge/util.py:104-110).
 *  - Parameters are fp32 row-major tables [rows][width]; width = d for E / R,
 *    d*d for RESCAL's W.
 *  - Accumulator invariant: between batches acc_sum == 0 and acc_cnt == 0
 *    for every table (zero them once at allocation).
 */
#ifndef SKGE_HIP_H
#define SKGE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKGE_ABI_VERSION 2

enum {
  SKGE_OK = 0,
  SKGE_EINVAL = -1,   /* bad argument (shape, enum, null pointer) */
  SKGE_EHIP = -2,     /* a HIP runtime call failed */
  SKGE_ENOTSUP = -3   /* unsupported configuration (e.g. d > 1024) */
};

/* models (skge/transe.py, skge/hole.py, skge/rescal.py; DistMult and ComplEx:
 * HolE's tables and conventions with the trilinear score, csrc/skge_diag.h).
 * Code 4 is unassigned: every entry point accepts 0..3, 5, 6 and 7 -- not
 * "<= 7" -- and answers 4 with SKGE_EINVAL like any unknown code.
 * skge_subgraph_rank takes 0..3 only.  SKGE_COMPLEX needs an even d: a row
 * holds d/2 complex components interleaved, (re, im) = (x[2j], x[2j+1]). */
enum {
  SKGE_TRANSE_L1 = 0,
  SKGE_TRANSE_L2 = 1,
  SKGE_HOLE = 2,
  SKGE_RESCAL = 3,
  SKGE_DISTMULT = 5,
  SKGE_COMPLEX = 6,
  /* RotatE (csrc/skge_rot.h): phi = -sum_j |E_s[j] * R_p[j] - E_o[j]| over the
   * d/2 complex components of ComplEx's row layout (d even), TransE's raw
   * pairwise margin loss, every component of R kept on the unit circle by
   * SKGE_POST_UNITMOD.  Served: skge_pair_grad, skge_score, skge_rank_known,
   * skge_topk, skge_rank_pools, skge_topk_pools, the pair loop runner and the
   * self-adversarial entry points (skge_sadv_*).
   * Refused with an error that names RotatE: the logistic entry points,
   * skge_relrank / skge_reltopk, skge_subgraph_rank, skge_rank and every
   * pipelined, two-launch, data-parallel and sharded runner. */
  SKGE_ROTATE = 7
};
/* activation functions (skge/actfun.py:13-57) */
enum { SKGE_AF_LINEAR = 0, SKGE_AF_SIGMOID = 1, SKGE_AF_TANH = 2, SKGE_AF_RELU = 3 };
/* updaters (skge/param.py:124-155) */
enum { SKGE_SGD = 0, SKGE_ADAGRAD = 1 };
/* post-update projections (skge/param.py:161-174) */
enum {
  SKGE_POST_NONE = 0,
  SKGE_POST_NORMALIZE = 1,
  SKGE_POST_NORMLESS1 = 2,
  /* every complex component (x[2j], x[2j+1]) of an updated row divided by its
   * modulus, a zero component set to (1, 0); width even and <= 1024, fp32 or
   * fixed-point sums.  Served by skge_accum_apply / skge_accum_apply2 /
   * skge_update_rows (and so the per-batch step and the pair loop); every
   * other consumer of a table refuses it by name */
  SKGE_POST_UNITMOD = 3
};
/* accumulator encodings */
enum {
  SKGE_ACC_F32 = 0,    /* acc_sum: fp32 [rows][width] */
  SKGE_ACC_I16X4 = 1,  /* acc_sum: exact integer sums of TransE-L1 sign contributions,
                          four elements per int64 (elements 4q..4q+3 in qword q, added
                          with one 64-bit integer atomic; exact while each 16-bit
                          field's total stays within +-32767, which a row whose
                          per-batch count is <= 32767 guarantees: the apply kernels
                          flag larger counts, skge_device_error bit 2) -- produced
                          only by skge_transe_sample_grad / the pipelined runner with
                          l1 != 0 and width % 4 == 0 */
  SKGE_ACC_FX64 = 3,   /* the deterministic reduce mode (float-valued models, off by
                          default): acc_sum is int64 [rows][width] fixed point with 40
                          fractional bits; every contribution is rounded once to that
                          grid and added with an exact integer atomic, so the sums --
                          and the parameters after the apply -- are the same bits run
                          to run whatever order the adds arrive in (the reference's
                          CSR mat-vec is deterministic too, skge/util.py:53-101).
                          Entity / narrow relation tables (width <= 1024, one copy) of
                          the per-batch paths and the device pair loop */
  SKGE_ACC_I8X4 = 4,   /* pipelined TransE-L1 runner's ENTITY table only: the exact sums
                          in four 8-bit fields per uint32 (acc_sum [rows][width/4]
                          dwords, one 32-bit integer atomic per quad), exact while a
                          row's per-batch count is <= 127 (the runner flags larger
                          counts); half the atomic bytes of int16x4 */
  SKGE_ACC_I32X2 = 2   /* pipelined runner's RELATION table only: the same exact sums
                          with 32-bit fields, two elements per int64 (a hot
                          relation's per-batch count passes 32767 long before any
                          entity row's does); the runner keeps these sums itself */
};

/*
 * One parameter table with its updater state and its segment-sum accumulator.
 * The gradient of a touched row r is
 *     g = (acc_sum[r] + rin * param[r]) / div + rout * param[r],
 *     div = fixed_div > 0 ? fixed_div : acc_cnt[r]
 * which covers every variant of the reference:
 *   mean                 Sm.dot(G) / n                     (transe.py:136)
 *   mean + rparam*P      hole.py:33,40,83  rescal.py:70,239
 *   (sum + rparam*P)/n   rescal.py:299-302 (rparam inside)
 *   (sum + rparam*W)/2   rescal.py:287-290 (divisor quirk)
 *
 * Touched rows are recorded in FIXED SLOTS (no shared counter): every
 * contribution site of a launch owns one slot of acc_touched and writes there
 * the row id it counted (or -1 if it added nothing); several slots may name
 * the same row, and consumers claim each row once (atomicExch on acc_cnt).
 * Slot maps:
 *   skge_pair_grad          ent: 4i+{0:sp,1:op,2:sn,3:on}   rel: 2i+{0:pp,1:pn}
 *   skge_triple_grad        ent: 2i+{0:s,1:o}               rel (HolE): i
 *   skge_rescal_wgrad       W:   slot p (all M slots)
 *   skge_transe_sample_grad ent: 4j+{0:s,1:o,2:s',3:o'}     rel: j
 * Consumers (apply / reset) take the slot count of the producing launch.
 * A narrow table with acc_touched == NULL is applied DENSELY: every row whose
 * count is non-zero (meant for small tables such as TransE's R; producers
 * then record nothing for it).  Replicated accumulators (acc_replicas > 1)
 * are produced by skge_transe_sample_grad only.
 */
typedef struct skge_table {
  float *param;        /* [rows][width] */
  float *state;        /* AdaGrad accumulator p2 [rows][width]; NULL for SGD */
  float *acc_sum;      /* [rows][width] */
  int *acc_cnt;        /* [rows] */
  int *acc_touched;    /* [touched_cap] slot -> row or -1; NULL: dense apply */
  int rows;
  int width;
  int touched_cap;     /* capacity of acc_touched (slots) */
  int acc_mode;        /* SKGE_ACC_F32 | SKGE_ACC_I16X4 | SKGE_ACC_FX64 (| runner-only modes) */
  int acc_replicas;    /* dense tables only: acc_sum / acc_cnt hold this many
                          copies ([replicas][rows][...]); producers spread their
                          adds over the copies (fewer same-address atomics on
                          hot rows such as TransE's 18 relations) and the apply
                          sums them.  0 or 1 = a single copy; else 2, 4, 8, 16
                          or 32. */
  int opt;             /* SKGE_SGD | SKGE_ADAGRAD */
  int post;            /* SKGE_POST_* */
  float lr;
  float rin, rout, fixed_div;
  const int *gate;     /* optional: if non-NULL and *gate == 0, the update is
                          skipped (the model returned None: no violations) */
  int *upd_count;      /* optional [rows]: AdaGrad applies add 1 per updated row
                          (Parameter.updateCounts, skge/param.py:149-150) */
  int *violations;     /* optional [rows], entity table of a TransE pair launch:
                          +1 per violating pair for each distinct entity of
                          {sn, on, sp, op} (E.violations, skge/transe.py:78-83) */
} skge_table_t;

int skge_abi_version(void);
const char *skge_last_error(void);
/* Synchronizes the stream and returns the error bits raised by device kernels
 * since the last reset (2 = a packed row's count exceeded 32767; 4 = an
 * SKGE_ACC_FX64 sum wrapped past its 2^23 range in gradient units -- every
 * fixed-point add checks its own signed overflow -- or a decoded sum was at
 * or past 2^22, half that range); reset != 0 clears them. */
int skge_device_error(void *stream, int reset);

/*
 * Pairwise scoring + contribution scatter for P explicit (positive, negative)
 * pairs.  Replaces the numeric part of Model._pairwise_gradients:
 *   TransE  skge/transe.py:48-165   (ent = E, rel = R)
 *   HolE    skge/hole.py:44-100     (ent = E, rel = R; af applied to scores)
 *   RESCAL  skge/rescal.py:78-139   (ent = E, rel = W; the dW part is
 *                                    skge_rescal_wgrad, fed by `coef`)
 * Writes the raw scores (pscore/nscore may be NULL), atomically adds the
 * violation count to *nviol, and accumulates every violating pair's
 * contribution rows into ent->acc_* / rel->acc_* (segment sum + counts).
 * coef (RESCAL only, [2P]): gp for every pair, then gn for every pair.
 * margin == -INFINITY: score only (nothing accumulated, no slots written).
 * A pair whose positive has relation -1 is SKIPPED (no score, no violation,
 * no contribution, coef 0; its negative is not read): the device pair loop
 * (skge_pair_runner_*) marks so a positive whose sampler found no negative
 * in ntries draws (skge/sample.py:41-46 drops that pair).  The same holds for
 * skge_pair_step.
 */
int skge_pair_grad(void *stream, int model, int af, const skge_table_t *ent,
                   const skge_table_t *rel, int d, const int *pos, const int *neg, int P,
                   float margin, float *pscore, float *nscore, float *coef, int *nviol);

/*
 * Logistic-loss scoring + contribution scatter for T labelled triples.
 * Replaces HolE._gradients (skge/hole.py:22-42) and RESCAL._gradients
 * (skge/rescal.py:37-76).  score may be NULL; *loss += sum logaddexp(0,-y*f);
 * coef [T] receives fs = -y*sigmoid(-y*f) (used by skge_rescal_wgrad).
 * A labelled triple whose relation is -1 is SKIPPED: it is not scored
 * (score[i] is left unwritten), adds nothing to the loss, makes no
 * contribution, takes no touched slot (its slots are written -1) and no
 * occurrence count, gets coef 0, and its s and o are not read.  The device
 * logistic loop (skge_triple_runner_*) marks so a negative its sampler did
 * not find in ntries draws (skge/sample.py:41-46 has no such triple).  The
 * same holds for skge_triple_step, and skge_rescal_wgrad leaves an item with
 * relation -1 out of every relation's sum and count.
 */
int skge_triple_grad(void *stream, int model, const skge_table_t *ent, const skge_table_t *rel,
                     int d, const int *trip, const float *ys, int T, float *score, float *coef,
                     float *loss);

/*
 * RESCAL relation-matrix gradient: for every relation p appearing in lists
 * a and b, acc_sum[p] = sum_i coef_i * outer(E[s_i], E[o_i]) and acc_cnt[p] =
 * number of occurrences (skge/rescal.py:61-70 and 113-125).
 */
int skge_rescal_wgrad(void *stream, const skge_table_t *ent, const skge_table_t *rel, int d,
                      const int *trip_a, const float *coef_a, int n_a, const int *trip_b,
                      const float *coef_b, int n_b);

/*
 * Materialise the segment mean held in a table's accumulator as the
 * reference's (grad_rows, sorted unique idx) pair (skge/util.py:53-101):
 * idx_out [rows], g_out [rows][width], *U_out = number of touched rows.
 * Resets the accumulator.  workspace: skge_collect_workspace_bytes(rows).
 */
size_t skge_collect_workspace_bytes(int rows);
int skge_accum_collect(void *stream, const skge_table_t *t, int *idx_out, float *g_out,
                       int *U_out, void *workspace, size_t ws_bytes);

/* Reset a table's accumulator (the rows in the first nslots slots) without
 * producing gradients. */
int skge_accum_reset(void *stream, const skge_table_t *t, int nslots);

/*
 * Updater call: param[idx] -= ... for U explicit (row, gradient) pairs, then
 * the projection.  Replaces ParameterUpdate.__call__ (skge/param.py:115-118)
 * with SGD._update (param.py:129-130) or AdaGrad._update (param.py:140-155),
 * then normalize / normless1 (param.py:161-174).  idx must be unique.
 */
int skge_update_rows(void *stream, const skge_table_t *t, const float *g, const int *idx, int U);

/*
 * Fused: segment mean + updater + projection straight from the accumulators
 * of up to 4 tables (trainer._batch_step, skge/base.py:1306-1316), resetting
 * the accumulator rows it reads.  nslots[i]: slot count of table i (the
 * producing launch's slot map, see skge_table_t).
 */
int skge_accum_apply(void *stream, const skge_table_t *tables, int ntables, const int *nslots);

/*
 * Explicit-pair training step: skge_pair_grad + (RESCAL dW) + apply
 * (one _pairwise_gradients + _batch_step, skge/base.py:1417-1427).  RESCAL
 * needs a workspace of skge_pair_step_workspace_bytes(model, P, rel->rows, d)
 * bytes (0 for the other models): for d <= 1024 and <= 8192 relations the
 * triples are grouped by relation and W[p] E[o], E[s] W[p] and dW run as fp32
 * MFMA GEMMs (skge_rescal.hip), otherwise as per-pair GEMVs.  The workspace
 * must hold finite floats on entry (zero it once after allocating; the calls
 * leave it finite): a skipped pair's stale rows are discarded by a zero
 * coefficient, which does not discard a NaN.  The same holds for
 * skge_triple_step; the runners zero their own workspace at create.
 */
size_t skge_pair_step_workspace_bytes(int model, int P, int M, int d);
int skge_pair_step(void *stream, int model, int af, const skge_table_t *ent,
                   const skge_table_t *rel, int d, const int *pos, const int *neg, int P,
                   float margin, void *workspace, size_t ws_bytes, int *nviol);

/*
 * Labelled-triple (logistic) training step: skge_triple_grad + (RESCAL dW) +
 * apply (one StochasticTrainer._process_batch, skge/base.py:1293-1316).
 * RESCAL needs skge_triple_step_workspace_bytes(model, T, rel->rows, d)
 * bytes of workspace (0 for HolE): relation-grouped fp32 MFMA GEMMs for
 * d <= 1024 and <= 8192 relations, per-triple GEMVs otherwise.
 */
size_t skge_triple_step_workspace_bytes(int model, int T, int M, int d);
int skge_triple_step(void *stream, int model, const skge_table_t *ent, const skge_table_t *rel,
                     int d, const int *trip, const float *ys, int T, void *workspace,
                     size_t ws_bytes, float *loss);

/*
 * Which kernels skge_pair_step (logistic == 0, n_items = P) or
 * skge_triple_step (logistic != 0, n_items = T) runs for a model of width d
 * with n_rel relations: SKGE_PATH_* | KM << 8, KM the registers per lane that
 * hold a row (1, 2, 3, 4, 8 or 16).  A query only -- nothing is launched --
 * answered by the predicates the launchers themselves branch on, so a test can
 * pin the path a shape is meant to reach.  SKGE_EINVAL for an unknown model, a
 * logistic TransE, or d outside 1..1024.
 */
#define SKGE_PATH_GENERIC 0            /* k_pair_grad / k_triple_grad */
#define SKGE_PATH_HOLE_FAST 1          /* register-tiled correlations */
#define SKGE_PATH_HOLE_FFT 2           /* wave FFT correlations */
#define SKGE_PATH_RESCAL_MFMA_SMALL 3  /* MFMA GEMMs, one-workgroup bucketing */
#define SKGE_PATH_RESCAL_MFMA_SORT 4   /* MFMA GEMMs, count / scan / scatter bucketing */
#define SKGE_PATH_RESCAL_VALU 5        /* per-pair GEMVs + k_rescal_wgrad */
int skge_step_path(int model, int logistic, int d, int n_rel, int n_items);

/* ---------------- device-resident batch loop (throughput path) ---------------- */

/*
 * Build the set of training triples used by the negative sampler's rejection
 * test (skge/sample.py:41-44): an open-addressing table of `capacity` 16-byte
 * slots (power of two >= 2*T) followed by a one-hash filter of 8*capacity
 * bits that answers most "not a training triple" queries with one load.
 * `set` must hold skge_triple_set_bytes(capacity) bytes; zeroed by this call.
 */
size_t skge_triple_set_bytes(int64_t capacity);
int skge_triple_set_build(void *stream, const int *trip, int64_t T, void *set,
                          int64_t capacity);

/*
 * One PairwiseStochasticTrainer mini-batch of TransE, fully on device
 * (skge/base.py:1268-1284 + 1394-1427 with RandomModeSampler(1, [0, 1])):
 * positive j of the batch is triple perm_epoch(start + j) (a keyed bijection
 * of [0, T), keyed by *epoch_key so that a captured graph reshuffles per
 * epoch); for each positive, mode 0 corrupts s and mode 1 corrupts o with up
 * to ntries rejection draws against the triple set; both pairs are scored,
 * margin-tested and their contributions accumulated.  nviol_total (optional)
 * accumulates over batches; neg_out (optional, [count][2]) records the sampled
 * corrupted entity per mode (-1 = skipped).
 */
int skge_transe_sample_grad(void *stream, int l1, const skge_table_t *ent,
                            const skge_table_t *rel, int d, const int *trip, int64_t T,
                            const void *set, int64_t set_capacity, int64_t start, int count,
                            uint64_t seed, const uint64_t *epoch_key, float margin, int ntries,
                            int *nviol, int *nviol_total, int *neg_out);

/* Data-parallel TransE-L1 (one model over G ranks): the pipelined runner's
 * data-parallel form, skge_pipe_runner_dp_* below. */

/* perm_out[j] = perm_epoch(j) for j < n (tests / host-side replay). */
int skge_epoch_permutation(void *stream, int64_t T, uint64_t seed, const uint64_t *epoch_key,
                           int64_t *perm_out, int64_t n);

/* *epoch_key += 1 (one-thread kernel, so a captured epoch graph advances it). */
int skge_epoch_advance(void *stream, uint64_t *epoch_key);

/*
 * Native epoch runner: captures one epoch of the device batch loop
 * (nbatches sample_grad + apply launches + epoch_advance; the reference's
 * np.split geometry, skge/base.py:1246-1268) into a hipGraph once, then
 * replays it.  Returns an opaque handle (NULL on error).
 */
typedef struct skge_runner skge_runner_t;
skge_runner_t *skge_runner_create(void *stream, int l1, const skge_table_t *ent,
                                  const skge_table_t *rel, int d, const int *trip, int64_t T,
                                  const void *set, int64_t set_capacity, int nbatches,
                                  uint64_t seed, uint64_t *epoch_key, float margin, int ntries,
                                  int *nviol, int *nviol_total);
int skge_runner_run(skge_runner_t *r, void *stream, int nepochs);
int skge_runner_nlaunches(const skge_runner_t *r);
void skge_runner_destroy(skge_runner_t *r);

/*
 * Ordering of one run of ANY runner below (its _run / _profile calls on
 * run_stream) against the stream the caller works on, paid for on the host:
 * run_stream never receives a cross-stream event wait, and caller_stream
 * only when asked.  (These two calls are the exception to "no call
 * synchronises".)
 *
 * begin, before the run's first launch, returns a path code or SKGE_E*:
 *   0  the streams are the same, or hipStreamQuery(caller_stream) found
 *      nothing in flight: nothing is enqueued on either stream;
 *   1  the caller's stream had work in flight: the HOST waited for it
 *      (hipStreamSynchronize); still nothing is enqueued on run_stream.
 * Any other status of the query (e.g. a capturing caller_stream) is SKGE_EHIP.
 * end, after the last launch, returns a path code or SKGE_E*:
 *   0  the streams are the same: nothing to do;
 *   1  queued == 0: the HOST waited for run_stream (hipStreamSynchronize);
 *      nothing is enqueued on caller_stream.  A wait queued on caller_stream
 *      sits unsatisfied in its hardware queue while the replays run, and
 *      that is what was measured to cost ~0.9 us on every replayed launch
 *      (profiles/run_ordering);
 *   2  queued != 0: an event recorded on run_stream (no timing) that
 *      caller_stream waits for; the call returns at once.
 * run_stream must not be NULL; caller_stream NULL = the legacy default stream.
 */
int skge_run_order_begin(void *run_stream, void *caller_stream);
int skge_run_order_end(void *run_stream, void *caller_stream, int queued);

/*
 * Device pair loop for any model (TransE L1/L2, HolE, RESCAL): one epoch of
 * PairwiseStochasticTrainer with RandomModeSampler(1, [0, 1])
 * (skge/base.py:1242-1291, 1394-1427; skge/sample.py:28-46) captured into a
 * hipGraph: the epoch's permutation and negatives (the same keyed draws as
 * the TransE runners), then per batch the explicit pairs (positive j ->
 * pairs 2j: s-corrupted, 2j+1: o-corrupted; a negative not found in ntries
 * draws -> a skipped pair) and one skge_pair_step.  ent needs 8 * batch_size
 * touched slots, rel (if it records slots) 4 * batch_size.  *nviol_total
 * accumulates the violations.  nlaunches reports the graph's node count.
 * skge_pair_runner_create_ex is the same loop with the negatives of another
 * sampler (skge_sampler_t below: the typed or LCWA sampler); nothing after the
 * draw differs.
 */
typedef struct skge_pair_runner skge_pair_runner_t;
/* The epoch's draws as the pair loop (and the pipelined TransE runner) make
 * them: rec [T][4] = (s, o, p, s' or -1), rec_n1 [T] = o' or -1, for
 * position j of the epoch's order (tests / host-side replay). */
int skge_epoch_sample(void *stream, const int *trip, int64_t T, const void *set,
                      int64_t set_capacity, int n_ent, uint64_t seed, const uint64_t *epoch_key,
                      int ntries, int *rec, int *rec_n1);
skge_pair_runner_t *skge_pair_runner_create(void *stream, int model, int af,
                                            const skge_table_t *ent, const skge_table_t *rel,
                                            int d, const int *trip, int64_t T, const void *set,
                                            int64_t set_capacity, int nbatches, uint64_t seed,
                                            uint64_t *epoch_key, float margin, int ntries,
                                            int *nviol_total);
/*
 * The negative sampler of skge_epoch_sample_ex and of the pair / logistic
 * loops' _ex constructors.  Every kind writes the same records, (s, o, p, s')
 * and o' per positive, each negative the first of ntries keyed draws
 * draw(key, j, mode, try, n) that passes the kind's test, else -1:
 *   RANDOM  RandomModeSampler(1, [0, 1]) (skge/sample.py:28-46): an entity
 *           id, accepted if the corrupted triple is not a training triple.
 *   TYPED   CorruptedSampler(1, xs, type_index(xs)) over modes [0, 1]
 *           (skge/sample.py:68-88): mode m draws an index into pool 2p + m
 *           (n = the pool's length; an empty pool draws nothing), the
 *           candidate is that pool entry, accepted as RANDOM's.
 *   LCWA    LCWASampler(1, [0, 1], xs, sz) (skge/sample.py:91-110): mode 0
 *           draws an entity id, accepted if it is in pool 2p (binary search:
 *           the reference's counts[(s', p)] > 0) and the corrupted triple is
 *           not a training triple; mode 1 keeps s, whose (s, p) the positive
 *           itself counts, so it is RANDOM's mode-1 draw bit for bit.
 * The pools are a CSR over 2 * n_rel lists: pool 2p + side holds the
 * ascending unique entity ids seen as subject (side 0) or object (side 1) of
 * relation p in the training triples; pool_off [2 * n_rel + 1] and pool_ent
 * are device memory.  A positive whose relation is not below n_rel draws no
 * pool negative.  The pools' CONTENTS are device data and are not checked:
 * offsets must be non-decreasing within pool_ent and entries valid entity
 * ids.  smp == NULL means RANDOM, as the entry points without _ex.
 */
#define SKGE_SAMPLER_RANDOM 0
#define SKGE_SAMPLER_TYPED 1
#define SKGE_SAMPLER_LCWA 2
typedef struct {
  int kind, n_rel;
  const int64_t *pool_off; /* [2 * n_rel + 1]; unused for RANDOM */
  const int *pool_ent;     /* ascending, unique within a pool */
} skge_sampler_t;
int skge_epoch_sample_ex(void *stream, const int *trip, int64_t T, const void *set,
                         int64_t set_capacity, int n_ent, uint64_t seed,
                         const uint64_t *epoch_key, int ntries, int *rec, int *rec_n1,
                         const skge_sampler_t *smp);
skge_pair_runner_t *skge_pair_runner_create_ex(void *stream, int model, int af,
                                               const skge_table_t *ent, const skge_table_t *rel,
                                               int d, const int *trip, int64_t T, const void *set,
                                               int64_t set_capacity, int nbatches, uint64_t seed,
                                               uint64_t *epoch_key, float margin, int ntries,
                                               int *nviol_total, const skge_sampler_t *smp);
/* skge_runner_create drawing its negatives with smp: the typed / LCWA
 * instances of its sample_grad kernels draw, one positive per wave, by the
 * rule of skge_epoch_sample_ex -- the same pairs, bit for bit (NULL or RANDOM:
 * skge_runner_create itself).  The runner keeps smp's pointers only; the
 * caller owns the pools for the runner's lifetime. */
skge_runner_t *skge_runner_create_smp(void *stream, int l1, const skge_table_t *ent,
                                      const skge_table_t *rel, int d, const int *trip, int64_t T,
                                      const void *set, int64_t set_capacity, int nbatches,
                                      uint64_t seed, uint64_t *epoch_key, float margin,
                                      int ntries, int *nviol, int *nviol_total,
                                      const skge_sampler_t *smp);
int skge_pair_runner_run(skge_pair_runner_t *r, void *stream, int nepochs);
int skge_pair_runner_nlaunches(const skge_pair_runner_t *r);
/* How the captured batches update the entity rows: 0 = sums accumulated by
 * the gradient launch, then an apply launch; 1 = RESCAL's row-grouped apply
 * (one wave per distinct row of the batch sums and applies; no apply launch).
 * Fixed at capture; -1 for a NULL runner. */
int skge_pair_runner_entity_apply(const skge_pair_runner_t *r);
void skge_pair_runner_destroy(skge_pair_runner_t *r);

/*
 * Device logistic loop (HolE, RESCAL): one epoch of StochasticTrainer with
 * RandomModeSampler(1, [0, 1]) (skge/base.py:1242-1316, skge/sample.py:28-46)
 * captured into a hipGraph: the epoch's permutation and negatives (the same
 * keyed draws as the other runners, replayed by skge_epoch_sample), then per
 * batch of c positives (the np.split geometry, remainder batch included) its
 * 3c labelled triples in the order `xys += samplef(xys)` gives -- the c
 * positives (y = +1), then for positive j its s-corruption at c + 2j and its
 * o-corruption at c + 2j + 1 (y = -1); a negative not found in ntries draws is
 * a skipped triple in place (relation -1, see skge_triple_grad) -- and one
 * skge_triple_step on them.  Every batch steps (there is no gate).  HolE with
 * d in the wave FFT's range and tables the per-positive kernels take scores a
 * positive and its two corruptions in one wave straight from the records
 * (k_hole_logistic_pos: 5 forward and 5 inverse transforms per positive
 * instead of 9 and 9; SKGE_HOLE_TRIPLES=1 keeps the explicit triples).  ent
 * needs 6 * batch_size touched slots, rel (if it records slots) 3 *
 * batch_size, RESCAL's W rel->rows.  The loss of every batch is added into
 * *loss_total (optional); *epoch_key += 1 at the end of the epoch.
 * nlaunches reports the graph's node count.
 */
typedef struct skge_triple_runner skge_triple_runner_t;
skge_triple_runner_t *skge_triple_runner_create(void *stream, int model, const skge_table_t *ent,
                                                const skge_table_t *rel, int d, const int *trip,
                                                int64_t T, const void *set, int64_t set_capacity,
                                                int nbatches, uint64_t seed, uint64_t *epoch_key,
                                                int ntries, float *loss_total);
/* the same loop drawing its negatives with smp (skge_sampler_t above) */
skge_triple_runner_t *skge_triple_runner_create_ex(void *stream, int model,
                                                   const skge_table_t *ent,
                                                   const skge_table_t *rel, int d,
                                                   const int *trip, int64_t T, const void *set,
                                                   int64_t set_capacity, int nbatches,
                                                   uint64_t seed, uint64_t *epoch_key, int ntries,
                                                   float *loss_total, const skge_sampler_t *smp);
int skge_triple_runner_run(skge_triple_runner_t *r, void *stream, int nepochs);
int skge_triple_runner_nlaunches(const skge_triple_runner_t *r);
void skge_triple_runner_destroy(skge_triple_runner_t *r);

/*
 * n negatives per positive over any modes: the reference's Sampler(n, modes)
 * (skge/sample.py:10-25) for the three kinds above.  A positive has K = n *
 * nmodes SLOTS, slot k = rep * nmodes + mi corrupting position modes[mi]
 * (0: s, 1: o, 2: p) -- rep-major, then the order of modes, the order
 * Sampler.sample appends.  Slot k's candidates are draw(key, j, k, try,
 * range): the draw's field is the slot, so (1, {0, 1}) draws the records of
 * skge_epoch_sample_ex bit for bit.  Modes 0 and 1 draw and accept as
 * skge_sampler_t describes.  Mode 2 draws a relation id p' -- RANDOM and LCWA
 * from [0, n_rel), TYPED from [0, rel_range), rel_range being the number of
 * relations that occur (the reference uses len(type_index) as an id range,
 * skge/sample.py:80) -- accepted if (s, o, p') is not a training triple and,
 * LCWA, s is in pool 2p' (skge/sample.py:106-107).
 * Needed: n >= 1, nmodes in [1, 8], every mode in {0, 1, 2}, K <= 64, and
 * rel_range in [1, n_rel] when a mode is 2; a pool kind's smp->n_rel must be
 * n_rel.
 *
 * skge_epoch_sample_multi writes, for position j of the epoch's order,
 * pos [T][3] = the positive (s, o, p) and neg [T][K] = slot k's corrupted id
 * (an entity for modes 0 and 1, a relation for mode 2) or -1 if none of ntries
 * candidates was accepted.
 *
 * skge_pair_runner_create_multi / skge_triple_runner_create_multi are the pair
 * loop and the logistic loop over those draws (run, nlaunches and destroy are
 * the ones above).  Every batch's explicit input is built once per epoch in
 * the reference's order -- pair loop: positive j gives pairs jK .. jK + K - 1
 * (skge/base.py:1394-1427); logistic loop: a batch of c positives is the c
 * positives, then the negative of (j, k) at c + jK + k (`xys +=
 * samplef(xys)`); a slot holding -1 is a skipped pair / triple in place -- and
 * each batch is one skge_pair_step on K * c pairs or one skge_triple_step on
 * (1 + K) * c triples (every model runs its explicit-pair / explicit-triple
 * kernels here).  ent needs 4 * K * batch_size touched slots for pairs and
 * 2 * (1 + K) * batch_size for triples, rel (if it records slots) half that
 * (RESCAL's W: rel->rows); a smaller table is refused.
 */
typedef struct {
  int n, nmodes;
  int modes[8];
  int rel_range; /* TYPED with a mode 2: len(type_index); else n_rel */
} skge_negatives_t;
int skge_epoch_sample_multi(void *stream, const int *trip, int64_t T, const void *set,
                            int64_t set_capacity, int n_ent, int n_rel, uint64_t seed,
                            const uint64_t *epoch_key, int ntries, int *pos, int *neg,
                            const skge_sampler_t *smp, const skge_negatives_t *negs);
skge_pair_runner_t *skge_pair_runner_create_multi(void *stream, int model, int af,
                                                  const skge_table_t *ent,
                                                  const skge_table_t *rel, int d, const int *trip,
                                                  int64_t T, const void *set,
                                                  int64_t set_capacity, int nbatches,
                                                  uint64_t seed, uint64_t *epoch_key, float margin,
                                                  int ntries, int *nviol_total,
                                                  const skge_sampler_t *smp,
                                                  const skge_negatives_t *negs);
skge_triple_runner_t *skge_triple_runner_create_multi(void *stream, int model,
                                                      const skge_table_t *ent,
                                                      const skge_table_t *rel, int d,
                                                      const int *trip, int64_t T, const void *set,
                                                      int64_t set_capacity, int nbatches,
                                                      uint64_t seed, uint64_t *epoch_key,
                                                      int ntries, float *loss_total,
                                                      const skge_sampler_t *smp,
                                                      const skge_negatives_t *negs);

/*
 * Self-adversarial negative-sampling loss for the distance models (TransE-L1,
 * TransE-L2, RotatE; phi <= 0), over the records of skge_epoch_sample_multi:
 * positive j = pos3[j] = (s, o, p) with K = n * nmodes slots negK[j][k], slot k
 * corrupting position modes[k % nmodes] with the id it holds; a slot holding
 * -1 is absent (no part in the softmax, the loss, the gradient or the counts).
 *   L_j   = -log sigmoid(gamma + phi_pos) - sum_k w_k log sigmoid(-(gamma + phi_k))
 *   w_k   = softmax over the valid slots of alpha * phi_k (max-subtracted); a
 *           constant: no gradient flows through it.  alpha = 0: 1 / Kv.
 *   c_pos = -sigmoid(-(gamma + phi_pos)),  c_k = w_k sigmoid(gamma + phi_k)
 * Each of the 1 + Kv triples of a positive contributes c * d phi / d row to
 * its rows s, o and p (the model's own directions: TransE's signs /
 * differences, RotatE's unit vectors) and counts as one occurrence of each;
 * the apply takes the library's mean over occurrences, then the updater and
 * the projection.  There is no margin test, no gate and no violation count.
 * One wave per positive (k_sadv_pos, csrc/skge_grad.hip).  Slot map: ent
 * (2 + K) j + {0: s, 1: o, 2 + k: slot k's entity}, rel (1 + K) j + {0: p,
 * 1 + k: slot k's relation}.
 * skge_sadv_grad: scores, coefficients and accumulators for skge_accum_collect;
 *   *loss += sum_j L_j; optional outputs pscore [P], nscore [P][K] and coef
 *   [P][1 + K] (c_pos, then c_k), an absent slot's score and coefficient 0.
 * skge_sadv_step: the same launch and the apply of both tables (every batch
 *   steps).
 * skge_sadv_runner_create: the device loop -- per epoch one
 *   skge_epoch_sample_multi draw, per batch one launch on the records and one
 *   apply, the losses added into *loss_total, *epoch_key += 1; (1, {0, 1}) is
 *   taken too, as K = 2.  Driven by skge_pair_runner_run / _nlaunches / _destroy.
 * Refused (SKGE_EINVAL / NULL, the text names what is wrong): any other model,
 * odd d for RotatE, d > 1024, negatives outside skge_negatives_t's bounds,
 * alpha < 0, non-finite gamma / alpha, packed accumulators, a replicated entity
 * accumulator, fewer touched slots than the map needs (with the count needed),
 * SKGE_POST_UNITMOD on a table it cannot serve.
 */
int skge_sadv_grad(void *stream, int model, const skge_table_t *ent, const skge_table_t *rel,
                   int d, const int *pos3, const int *negK, int P, const skge_negatives_t *negs,
                   float gamma, float alpha, float *pscore, float *nscore, float *coef,
                   float *loss);
int skge_sadv_step(void *stream, int model, const skge_table_t *ent, const skge_table_t *rel,
                   int d, const int *pos3, const int *negK, int P, const skge_negatives_t *negs,
                   float gamma, float alpha, float *loss);
skge_pair_runner_t *skge_sadv_runner_create(void *stream, int model, const skge_table_t *ent,
                                            const skge_table_t *rel, int d, const int *trip,
                                            int64_t T, const void *set, int64_t set_capacity,
                                            int nbatches, uint64_t seed, uint64_t *epoch_key,
                                            float gamma, float alpha, int ntries,
                                            float *loss_total, const skge_sampler_t *smp,
                                            const skge_negatives_t *negs);

/*
 * KvsAll (1-N) training of SKGE_DISTMULT and SKGE_COMPLEX: B queries (anchor
 * q_anchor[b], relation q_rel[b], direction q_dir[b]: 0 asks for the tails of
 * (a, p, ?), 1 for the heads of (?, p, a)), each scored against EVERY entity
 * row, with binary cross-entropy against its known answers ans_ids[ans_off[b]
 * .. ans_off[b + 1]) (a device CSR; ids outside [0, N) are ignored):
 *   q_b  = the query vector of skge_rank / skge_topk (DistMult E_a o R_p;
 *          ComplEx E_a R_p for tails, conj(R_p) E_a for heads)
 *   z_be = q_b . E_e
 *   y'_be = (1 - smoothing) [e answers b] + smoothing / N
 *   L    = (1 / B) sum_b sum_e -(y' log sigma(z) + (1 - y') log(1 - sigma(z)))
 * The model's activation plays no part.  The gradient is the plain gradient
 * of L -- no mean over a row's occurrences: every entity row occurs in every
 * query, and the anchors' and relations' chain-rule terms are summed.
 * Launches (csrc/skge_kvsall.hip): the query vectors, the answers' bitmap,
 * three fp32 MFMA products (Z = Q E^T with the loss epilogue writing G =
 * (sigma(z) - y') / B; dq = G E over slices of the entities; gE = G^T Q), the
 * chain rule (float atomics into gE[a] and gR[p]) and the loss's fixed-order
 * sum.
 * skge_kvsall_grad: gE [N][d] (every row written), gR [M][d] and r_touched
 *   [M] (zeroed first; a relation row no query names stays exactly 0 and
 *   unmarked, a named one is marked 1), *loss += L; scores (optional, tests)
 *   receives z [B][N].  No regulariser.
 * skge_kvsall_step: the same, then the tables' updater and projection (opt,
 *   lr, state, post, upd_count) with g + (rin + rout) * param on EVERY entity
 *   row and on the marked relation rows; an unmarked relation row keeps its
 *   bits, state included.  The accumulator fields, fixed_div and gate are not
 *   used.  No device-to-host copy and no synchronisation.
 * A query naming a row outside its table scores as the zero vector and has no
 * chain-rule term.  workspace: skge_kvsall_workspace_bytes (0 for arguments
 * the entry points refuse), 16-byte aligned; B * N is indexed in size_t.
 * Refused, the text naming what was asked: a model code other than 5 / 6
 * (0..3 and 7: SKGE_ENOTSUP, by name; 4 and anything else: SKGE_EINVAL),
 * B > 4096 or d > 1024 (SKGE_ENOTSUP), sizes < 1, odd d for ComplEx,
 * smoothing outside [0, 1), NULL arguments, a short workspace (SKGE_EINVAL).
 */
size_t skge_kvsall_workspace_bytes(int model, int B, int N, int M, int d);
int skge_kvsall_grad(void *stream, int model, const float *E, const float *R, int N, int M,
                     int d, const int *q_anchor, const int *q_rel, const int *q_dir, int B,
                     const int *ans_off, const int *ans_ids, float smoothing, float *gE,
                     float *gR, int *r_touched, float *loss, float *scores, void *workspace,
                     size_t ws_bytes);
int skge_kvsall_step(void *stream, int model, const skge_table_t *ent, const skge_table_t *rel,
                     int d, const int *q_anchor, const int *q_rel, const int *q_dir, int B,
                     const int *ans_off, const int *ans_ids, float smoothing, float *loss,
                     void *workspace, size_t ws_bytes);

/*
 * 1vsAll training of SKGE_DISTMULT and SKGE_COMPLEX (Lacroix et al. 2018):
 * softmax cross-entropy of every query against its ONE target, with the
 * nuclear 3-norm regulariser N3.  A query is (anchor q_anchor[b], relation
 * q_rel[b], direction q_dir[b], target q_target[b]): direction 0 is (a, p, ?)
 * with the triple's object for target, 1 is (?, p, a) with its subject; one
 * query per training triple and direction, never deduplicated.  With q_b the
 * query vector of skge_kvsall_grad, z_be = q_b . E_e, eps = smoothing:
 *   y'_be = (1 - eps) [e == g_b] + eps / N
 *   lse_b = log sum_e exp(z_be)                       (max-subtracted)
 *   L_ce  = (1 / B) sum_b ( lse_b - sum_e y'_be z_be )
 *   G_be  = ( exp(z_be - lse_b) - y'_be ) / B
 *   gE[e] = sum_b G_be q_b        dq_b = sum_e G_be E_e
 *   L_n3  = (n3 / B) sum_b ( |E_a|_3^3 + |R_p|_3^3 + |E_g|_3^3 )
 * dq_b goes through q's Jacobian into gE[a_b] and gR[p_b] as in
 * skge_kvsall_grad.  |x|_3^3 sums |x_k|^3 (DistMult) or (re^2 + im^2)^(3/2)
 * over the d / 2 interleaved complex components (ComplEx); its gradient,
 * 3 |x_k| x_k or 3 |c_j| (re, im) times n3 / B, is added once per occurrence
 * to gE[a], gR[p] and gE[g]; it is 0, never NaN, at a zero component.
 * *loss += L_ce + L_n3.  The gradient is the plain gradient of that sum, no
 * mean over occurrences; the model's activation plays no part.
 * Launches (csrc/skge_kvsall.hip): the query vectors; Z = Q E^T, whose
 * epilogue leaves raw z in G and, per row and 128-column tile, max z, sum
 * exp(z - max) and sum z; the combine (lse_b, the query's loss partial, G
 * rewritten in place to (softmax - y') / B); dq = G E; gE = G^T Q; at n3 > 0
 * the N3 gradient, one plain add per element of every row a query names (its
 * occurrence count times the row's term); the chain rule (float atomics); the
 * loss's fixed-order sum.
 * skge_onevsall_grad: gE [N][d] (every row written), gR [M][d] and r_touched
 *   [M] as skge_kvsall_grad leaves them; scores (optional) receives z [B][N],
 *   lse (optional) lse_b [B].  No rparam regulariser.
 * skge_onevsall_step: the same, then skge_kvsall_step's updates: every entity
 *   row, the marked relation rows, g + (rin + rout) * param.
 * A query is invalid when its anchor, relation, direction or target lies
 * outside its table: its G row is zero, it adds no loss, no chain-rule term, no
 * N3 term and no mark, B still counts it, and nothing is read or written out
 * of bounds for it.  workspace: skge_onevsall_workspace_bytes (0 for arguments
 * the entry points refuse), 16-byte aligned: Q, G, the dq partials, 3 nby B row
 * partials (nby = ceil(N / 128)), lse, one loss partial per query, N + M
 * occurrence counts, and the step's gE, gR and marks; no answer bitmap.
 * Refused as skge_kvsall_* refuse (models other than 5 / 6 by name, B > 4096,
 * d > 1024, sizes < 1, odd d for ComplEx, smoothing outside [0, 1), NULL
 * arguments, a short workspace), and n3 < 0 or not finite (SKGE_EINVAL).
 */
size_t skge_onevsall_workspace_bytes(int model, int B, int N, int M, int d);
int skge_onevsall_grad(void *stream, int model, const float *E, const float *R, int N, int M,
                       int d, const int *q_anchor, const int *q_rel, const int *q_dir,
                       const int *q_target, int B, float smoothing, float n3, float *gE,
                       float *gR, int *r_touched, float *loss, float *scores, float *lse,
                       void *workspace, size_t ws_bytes);
int skge_onevsall_step(void *stream, int model, const skge_table_t *ent, const skge_table_t *rel,
                       int d, const int *q_anchor, const int *q_rel, const int *q_dir,
                       const int *q_target, int B, float smoothing, float n3, float *loss,
                       void *workspace, size_t ws_bytes);

/*
 * Pipelined epoch runner for TransE-L1 with packed accumulators (the
 * throughput path).  Same result, bit for bit, as skge_runner_create's loop
 * with the same tables and arguments: all negatives of an epoch are drawn in
 * one launch, then each mini-batch is ONE launch that scores batch b while
 * applying batch b-1's updates.  Below 16k slot records per batch with d <= 64
 * (the default there; SKGE_PIPE_FUSED=1 forces it up to d <= 256): k_pipe_fused,
 * whose work items are first one scoring item per positive, then one item per
 * four slot records of the previous batch (applied) and four of the batch
 * before (zeroed); a row the previous batch touched is updated by each of its
 * readers itself, from its pre-update value, which stays readable because the
 * applier writes the row's other buffer (the runner's second copy of E and
 * its AdaGrad state; run() and profile() end by copying every row back into
 * the caller's tables).  Otherwise k_pipe_batch: apply waves beside scoring
 * waves that wait for a pending row's publisher (one apply wave per slot
 * record below 16k slot records; above, owner marks over the slot records).
 * Needs ent
 * in SKGE_ACC_I16X4 mode (SKGE_ACC_I8X4: int8x4 sums, counts <= 127), rel in
 * SKGE_ACC_I16X4 or SKGE_ACC_I32X2 mode (the encoding of the relation sums
 * the runner keeps), d % 4 == 0, an entity table with slot records (capacity
 * >= 4 * batch), a dense single-copy relation table and no gates.  Any batch
 * size: a row's 16-bit packed sums are exact while its per-batch count is
 * <= 32767 (each occurrence adds a coefficient no larger than the count it
 * adds), and the apply reports a larger count through skge_pipe_runner_error
 * (bit 2); 32-bit relation sums are exact below 2^29 positives.  Allocates
 * its extra accumulator copies, row buffers and per-row words itself (freed
 * by destroy).  *epoch_key must only advance (the runner advances it once per
 * epoch).  Replaces the per-batch loop of skge/base.py:1268-1284.
 */
typedef struct skge_pipe_runner skge_pipe_runner_t;
skge_pipe_runner_t *skge_pipe_runner_create(void *stream, const skge_table_t *ent,
                                            const skge_table_t *rel, int d, const int *trip,
                                            int64_t T, const void *set, int64_t set_capacity,
                                            int nbatches, uint64_t seed, uint64_t *epoch_key,
                                            float margin, int ntries, int *nviol_total);
/* skge_pipe_runner_create with a flags word: 0, or SKGE_PIPE_DP (the
 * data-parallel form below: TransE-L1, no hot rows, driven launch by launch;
 * run() / profile() refuse it). */
#define SKGE_PIPE_DP 1
skge_pipe_runner_t *skge_pipe_runner_create_ex(void *stream, const skge_table_t *ent,
                                               const skge_table_t *rel, int d, const int *trip,
                                               int64_t T, const void *set, int64_t set_capacity,
                                               int nbatches, uint64_t seed, uint64_t *epoch_key,
                                               float margin, int ntries, int *nviol_total,
                                               int flags);
/*
 * Pipelined HolE pairwise runner (skge/hole.py:44-100, E post normless1):
 * the same epoch structure as skge_pipe_runner_create -- launch g scores
 * batch b (both pairs of a positive per wave: k_hole_pos's seven correlations
 * and arithmetic) while other workgroups apply batch b-1's rows -- with fp32
 * sums: ent F32 with slot records (capacity >= 4 * batch), rel F32 dense
 * single copy, d % 4 == 0, 4 <= d <= 256, af an SKGE_AF_* code, no gates.
 * Draws the same pairs as skge_pair_runner_create's HolE path; parameters
 * equal its to fp32 rounding.  Driven by skge_pipe_runner_run / _profile /
 * _error / _nlaunches / _destroy.  Replaces skge/base.py:1268-1284 for HolE.
 */
skge_pipe_runner_t *skge_hole_pipe_runner_create(void *stream, int af, const skge_table_t *ent,
                                                 const skge_table_t *rel, int d, const int *trip,
                                                 int64_t T, const void *set, int64_t set_capacity,
                                                 int nbatches, uint64_t seed, uint64_t *epoch_key,
                                                 float margin, int ntries, int *nviol_total);
/*
 * The pipelined runners drawing their negatives with smp (skge_sampler_t; NULL
 * or RANDOM: the constructors above, kernel for kernel).  Only the epoch's
 * draw launch differs: the kind's instance writes the records of
 * skge_epoch_sample_ex and, as the RANDOM launch, the runner's copy of the
 * epoch key, and draws no negative once the error word is set.  The hot rows
 * are chosen by occurrences, as ever; SKGE_PIPE_HOT_NEG=1 adds a pool kind's
 * expected corruptions per epoch (a pool of length L gets its relation's
 * positives / L per member) -- the same bits either way, and measured slower.
 * SKGE_PIPE_DP with a pool kind is refused.  The runner keeps smp's pointers
 * only; the caller owns the pools for the runner's lifetime.
 */
skge_pipe_runner_t *skge_pipe_runner_create_smp(void *stream, const skge_table_t *ent,
                                                const skge_table_t *rel, int d, const int *trip,
                                                int64_t T, const void *set, int64_t set_capacity,
                                                int nbatches, uint64_t seed, uint64_t *epoch_key,
                                                float margin, int ntries, int *nviol_total,
                                                int flags, const skge_sampler_t *smp);
skge_pipe_runner_t *skge_hole_pipe_runner_create_smp(void *stream, int af,
                                                     const skge_table_t *ent,
                                                     const skge_table_t *rel, int d,
                                                     const int *trip, int64_t T, const void *set,
                                                     int64_t set_capacity, int nbatches,
                                                     uint64_t seed, uint64_t *epoch_key,
                                                     float margin, int ntries, int *nviol_total,
                                                     const skge_sampler_t *smp);
/* The pipelined runners' draw launch on its own (tests / host-side replay):
 * skge_epoch_sample_ex's records through the launch the runners capture, with
 * its two extra duties -- *key_copy = *epoch_key (optional), and no negative
 * drawn (every s' and o' is -1) when *err (optional, device) is non-zero.
 * ntries >= 0. */
int skge_pipe_epoch_sample(void *stream, const int *trip, int64_t T, const void *set,
                           int64_t set_capacity, int n_ent, uint64_t seed,
                           const uint64_t *epoch_key, int ntries, int *rec, int *rec_n1,
                           const skge_sampler_t *smp, const int *err, uint64_t *key_copy);
int skge_pipe_runner_run(skge_pipe_runner_t *r, void *stream, int nepochs);
/* synchronizes the stream; returns 0, or a bit set (results then invalid):
 * 1 = a bounded cross-workgroup wait gave up, 2 = a row's per-batch count
 * exceeded 32767 (packed sums may have wrapped); or a negative error code */
int skge_pipe_runner_error(skge_pipe_runner_t *r, void *stream);
int skge_pipe_runner_nlaunches(const skge_pipe_runner_t *r);
/* Hot entity rows of a TransE pipelined runner (hand-off kernel, int16x4
 * sums): rows whose subject/object occurrences put them in >= 4 slots of an
 * average batch and >= 8x the average row's (the hubs of a skewed KG), at
 * most 256.  Their per-batch sums and counts are spread over 4 replicas
 * (positive w into replica w % 4), and every scoring wave that reads a hub
 * computes its updated value itself from the replicas (exact integer sums:
 * bitwise the same result), so nothing waits on a hub and its atomics do not
 * serialise on one row.  Returns their number (0: none). */
int skge_pipe_runner_hot_rows(const skge_pipe_runner_t *r);
/* The batch kernel the runner launches: 0 k_pipe_batch, 1 k_pipe_fused,
 * 2 k_hole_pipe (-1: NULL runner) -- what a profile of its launches is named. */
int skge_pipe_runner_kernel(const skge_pipe_runner_t *r);
/* The plan of the runner skge_pipe_runner_create_ex (hole == 0, with flags) or
 * skge_hole_pipe_runner_create (hole != 0) would build over these tables, T
 * and nbatches -- decided where the constructors decide it, and answered
 * without a device: no HIP call is made and no pointer of the tables is
 * dereferenced (they are only tested for NULL, as the constructors test them).
 * kernel: skge_pipe_runner_kernel's code; grouped: owner marks (more than 16k
 * slot records per batch); e8 / w32: int8x4 entity / int32x2 relation sums;
 * fft / pair: the HolE forms; kq: quads per lane (1, 2, 4); rel_reps: relation
 * sum replicas; nlaunches: skge_pipe_runner_nlaunches' figure; device_bytes:
 * what the runner allocates beside the caller's tables, an upper bound where
 * hot rows are looked for (counted at the 256 the search may keep).  Refuses
 * (SKGE_EINVAL and the constructors' error text) what they refuse about the
 * flags, the tables, T, nbatches and the slot capacity.  Reads SKGE_PIPE_FUSED
 * and SKGE_HPIPE_RREPS as the constructors do. */
typedef struct skge_pipe_plan {
  int kernel, grouped, e8, w32, fft, pair, kq, rel_reps, nlaunches;
  uint64_t device_bytes;
} skge_pipe_plan_t;
int skge_pipe_runner_plan(const skge_table_t *ent, const skge_table_t *rel, int d, int64_t T,
                          int nbatches, int flags, int hole, skge_pipe_plan_t *out);
/* One epoch launched eagerly (trains like run(1)) with HIP events around every
 * launch: us_out[i] = launch i's duration (i = 0: negative draws, 1..nb1:
 * batches, nb1+1: flush, nb1+2: key advance); stats_out[3i..3i+2] = entity
 * rows applied, relation rows applied, violating pairs scored by launch i.
 * Both arrays need nlaunches entries (x3 for stats).  For the roofline.
 * Diagnostics: if trace_out is given, batch launch trace_launch (1..nb1+1)
 * records per-wave s_memrealtime stamps (10 ns): trace_out[0] = scoring
 * waves B, [1] = apply waves A, then 6 words per scoring wave (start, rows
 * loaded, pending rows settled, scored, atomics done, pending mask | 256 if
 * violating) and 2 per apply wave (start, end); trace_len must hold them. */
int skge_pipe_runner_profile(skge_pipe_runner_t *r, void *stream, float *us_out, int *stats_out,
                             int n, int trace_launch, uint64_t *trace_out, int64_t trace_len);
void skge_pipe_runner_destroy(skge_pipe_runner_t *r);
/* Batches per epoch (nb1; launch nb1 is the flush), or -1. */
int skge_pipe_runner_nbatches(const skge_pipe_runner_t *r);

/* ---- data-parallel form of the pipelined runner (SKGE_PIPE_DP) ----
 * ONE model replicated over G ranks (skge_amd/dp.py; skge/base.py:1268-1284,
 * 1394-1427 over the union batch).  Every rank creates the runner with the
 * same tables, KG, nbatches and seed (so every rank draws the same epoch
 * records) and runs, per epoch:
 *   dp_begin;
 *   for b in 0..nb1-1:
 *     dp_batch(b, lo, hi, rec_out, fold = G == 1)  -- ONE launch: applies batch
 *         b-1's rows (all ranks' contributions) and scores the rank's slice
 *         [lo, hi) of batch b, adding its contributions locally and writing
 *         one record per scored positive (skge_pipe_dp_record_bytes(d) each);
 *     all-gather of the slices' records (the caller's collective, rank-major:
 *         union position w's record at w);
 *     dp_scatter(b, gathered, lo, hi)  -- adds the other ranks' positives
 *         (skipped work when there are none);
 *   dp_batch(nb1, 0, 0, NULL, 0) (the flush); dp_end.
 * Sums are exact integers, so every replica equals one GPU's run over the
 * union batches bit for bit.  Each rank's violations (its slices) go to its
 * nviol_total at the flush. */
size_t skge_pipe_dp_record_bytes(int d);
int skge_pipe_runner_dp_begin(skge_pipe_runner_t *r, void *stream);
int skge_pipe_runner_dp_batch(skge_pipe_runner_t *r, void *stream, int b, int lo, int hi,
                              void *rec_out, int fold);
int skge_pipe_runner_dp_scatter(skge_pipe_runner_t *r, void *stream, int b, const void *recs,
                                int lo, int hi);
int skge_pipe_runner_dp_end(skge_pipe_runner_t *r, void *stream);

/* ---------------- row-sharded TransE-L1 step ----------------
 *
 * The entity table split by row over G ranks (rank g owns rows r % G == g at
 * local index r / G), the relation table replicated.  One mini-batch of
 * PairwiseStochasticTrainer (skge/base.py:1394-1427, TransE._pairwise_gradients
 * skge/transe.py:48-165, AdaGrad + normalize skge/param.py:140-167) over the
 * union of every rank's positives is, on each rank:
 *   skge_shard_route   -> exchange request ids (all-to-all) ->
 *   skge_shard_gather  -> exchange rows back (all-to-all) ->
 *   skge_shard_score   -> exchange contributions (all-to-all) ->
 *   skge_shard_accum   -> all-reduce the relation sums and counts ->
 *   skge_accum_apply({entity shard: nslots = requests received}, {rel: dense}).
 * The exchanges belong to the caller (RCCL via torch.distributed).  All sums
 * are exact integers, so the result equals one GPU's step on the union batch
 * bit for bit.  Positives come from skge_epoch_sample records (rec, rec_n1).
 */

/* Bucket the requests (s, o, s', o') of positives [start, start+count) by
 * owner: send_ids [4*count] (owner-major, request order within a bucket),
 * req_pos [4*count] = slot of request 4j+k in send_ids (-1: skipped negative),
 * counts [G] int64 = bucket sizes.  G <= 64. */
size_t skge_shard_route_workspace_bytes(int count, int G);
int skge_shard_route(void *stream, const int *rec, const int *rec_n1, int64_t start, int count,
                     int G, int *send_ids, int *req_pos, long long *counts, void *workspace,
                     size_t ws_bytes);
/* The fixed-capacity layout of the graph-capturable step (no host-side split
 * sizes): send_ids [G][C] = bucket g holds the requests owned by rank g in
 * request order, unused slots -1 (the all-to-alls then move G equal slices);
 * req_pos [4*count] = bucket slot of request 4j+k (-1: skipped negative).  A
 * bucket needing more than C slots sets *err |= 1 (its requests are dropped:
 * the caller must check *err).  The consumers below skip ids < 0. */
int skge_shard_route_cap(void *stream, const int *rec, const int *rec_n1, int64_t start,
                         int count, int G, int C, int *send_ids, int *req_pos, void *workspace,
                         size_t ws_bytes, int *err);
/* Owner side: rows_out[i] = E_shard[ids[i] / G] for i < n ([n][d] fp32;
 * ids[i] < 0: nothing written). */
int skge_shard_gather(void *stream, const float *E_shard, int d, int G, const int *ids, int64_t n,
                      float *rows_out);
/* Contribution record of one request: int32 count, pad to 16 B, int8[d]. */
long long skge_shard_contrib_stride(int d);
/* Requester side: score both pairs of every positive from the fetched rows
 * (fetched[req_pos[4j+k]]) and rel (dense packed accumulator, replicated
 * table), apply the strict margin test, write one contribution record per
 * request into contrib [n_send][stride] and add the relation contributions
 * into rel's accumulator; violations into the 64 sharded counters vshards
 * (64 x 32 ints, folded by skge_shard_fold_violations). */
int skge_shard_score(void *stream, const skge_table_t *rel, int d, const int *rec,
                     const int *rec_n1, int64_t start, int count, const float *fetched,
                     const int *req_pos, float margin, void *contrib, int *vshards);
/* Owner side: add the n received records into ent_shard's packed sums (local
 * row ids[i] / G), touched slot i per record (-1 for ids[i] < 0); touched_cap >= n. */
int skge_shard_accum(void *stream, const skge_table_t *ent_shard, int G, const int *ids,
                     const void *contrib, int64_t n);
/* *nviol_total += the violation shards, which are cleared. */
int skge_shard_fold_violations(void *stream, int *vshards, int *nviol_total);

/* ---------------- measurement ----------------
 *
 * Measured gather + RMW-scatter roofline: one launch of the same row traffic
 * as a training launch without its dependencies.  n_rmw waves each read and
 * write back one random row of P, A (fp32 [rows][d]) and S (packed sums,
 * u64 [rows][d/4]) = 20d bytes; then n_gather waves each gather
 * rows_per_wave random rows of P (4d bytes each) and add atom_rows_per_wave
 * rows of 64-bit atomics into S (2d bytes each).  out [n_gather] receives a
 * per-wave checksum.  The values of P, A, S are left unchanged.  Not part of
 * the training path (bench.py times it beside the training kernels). */
int skge_roofline_gather(void *stream, float *P, float *A, void *S, int rows, int d, int n_gather,
                         int rows_per_wave, int atom_rows_per_wave, int n_rmw, uint32_t salt,
                         float *out);
/* Hand-off latency probe: the pipelined runner's publish / wait form (16-B
 * write-through payload, drain, write-through flag; the waiter polls the flag
 * and re-reads the payload with write-through loads) ping-ponged `rounds`
 * times between two workgroups.  buf: >= 1024 device bytes (zeroed here);
 * out [3] (device u64): out[0] = 10-ns ticks for all rounds (two hops each),
 * out[1] = payload mismatches (0 expected), out[2] = 1 if a bounded wait gave
 * up.  Lets a bench line say how slow this box's hand-offs are. */
int skge_handoff_probe(void *stream, void *buf, int rounds, uint64_t *out);

/* ---------------- evaluation ---------------- */

/*
 * Filtered link-prediction ranks: FilteredRankingEval.positions
 * (skge/base.py:913-1031) with TransEEval (skge/run_transe.py:15-29; the L1
 * distance for either norm, as there) or HolEEval (skge/run_hole.py:12-19);
 * RESCAL scores E_s W_p E_o the same way.  For each test triple i = (s, o, p)
 * of queries[nq][3]: ranks_out[4i..4i+3] = tail rank of o given (s, p) raw and
 * filtered, head rank of s given (o, p) raw and filtered, where rank = 1 +
 * #entities scoring strictly higher (ties in the true entity's favour) and
 * the filtered count skips entities forming a known triple (set: a triple set
 * built by skge_triple_set_build over the known triples; NULL = no filter).
 * E [N][d], R [M][d] (W [M][d][d] for RESCAL), d <= 1024; workspace of
 * skge_rank_workspace_bytes(nq, d) bytes.
 */
size_t skge_rank_workspace_bytes(int nq, int d);
/*
 * skge_rank with the filter given as each query's KNOWN ANSWERS instead of a
 * triple set: tail_ent[tail_off[i] .. tail_off[i+1]) = every o' != o with
 * (s, o', p) known, head_ent[head_off[i] .. head_off[i+1]) = every s' != s
 * with (s', o, p) known (int32, offsets nq + 1).  rank_filtered = rank_raw -
 * #{those answers scoring strictly above the true entity}: the same positions
 * as skge_rank, with no triple-set lookups in the all-entity pass (which also
 * spreads each query block over entity slices).  Workspace:
 * skge_rank_known_workspace_bytes(nq, d).
 */
size_t skge_rank_known_workspace_bytes(int nq, int d);
int skge_rank_known(void *stream, int model, const float *E, const float *R, int N, int d,
                    const int *queries, int nq, const int *tail_off, const int *tail_ent,
                    const int *head_off, const int *head_ent, void *workspace, size_t ws_bytes,
                    int *ranks_out);
int skge_rank(void *stream, int model, const float *E, const float *R, int N, int d,
              const int *queries, int nq, const void *set, int64_t set_capacity,
              void *workspace, size_t ws_bytes, int *ranks_out);

/*
 * Top-k link prediction: for each query i = (anchor a, relation p) of
 * queries[nq][2], the k best entities j as the tail of (a, p, j) (direction 0)
 * or the head of (j, p, a) (direction 1), scored with the query vectors and
 * the sequential fp32 chain of the ranking entry points above.
 *
 * ONE DIFFERENCE from skge_rank / skge_rank_known: those score both TransE
 * codes with the L1 distance (the reference evaluator's form); here
 * SKGE_TRANSE_L1 scores -sum|q - E_j| and SKGE_TRANSE_L2 scores
 * -sum (q - E_j)^2, the model's own training score.  Pass SKGE_TRANSE_L1 for
 * an L2-trained model to get the evaluator's order.
 *
 * excl_off [nq + 1] / excl_ent: per query, entity ids that are never returned
 * (int32, ascending and unique within a query); excl_off NULL = none.
 * Result: ent_out / score_out [nq][k], ordered by descending score, then
 * ascending entity id among exactly equal fp32 scores; when fewer than k
 * entities are eligible (k > N is legal) the remaining slots hold entity -1
 * and score -inf.  1 <= k <= 128, d <= 1024; ids are not range-checked here.
 * Caller-owned buffers, stream-ordered; workspace of
 * skge_topk_workspace_bytes(nq, d, k, N) bytes.
 */
size_t skge_topk_workspace_bytes(int nq, int d, int k, int N);
int skge_topk(void *stream, int model, const float *E, const float *R, int N, int d,
              const int *queries, int nq, int direction, int k, const int *excl_off,
              const int *excl_ent, void *workspace, size_t ws_bytes, int *ent_out,
              float *score_out);

/* ---------------- subgraph embeddings and ranking ---------------- */

/*
 * Subgraph embeddings: Experiment.make_subgraphs (skge/base.py:122-202), the
 * sub_algo == "transe" branch.  Subgraph i has the members
 * mem_ent[mem_off[i] .. mem_off[i+1]) (entity ids, int32; mem_off int64
 * [S + 1]).  SA[i] = the mean of E[m] over its members; when SV is given,
 * SV[i] = sum (E[m] - SA[i])^2 / (count - 1) for count > 2 and SA[i]
 * otherwise (the reference's quirk, base.py:154-157), by two passes (the
 * mean, then the squared differences).  A group with more members than the
 * split threshold (256) is summed in pieces that are added in
 * piece order: no float atomics, the same bits on every run.
 * E [N][d], SA / SV [S][d], d <= 1024, S > 0; member ids are not
 * range-checked here.  The workspace function takes the CSR's member total,
 * mem_off[S]; a smaller workspace (at least that of 0 members) is legal and
 * leaves the groups whose pieces do not fit unsplit.
 */
size_t skge_subgraph_embed_workspace_bytes(int S, int d, int64_t n_members);
int skge_subgraph_embed(void *stream, const float *E, int N, int d, const int64_t *mem_off,
                        const int *mem_ent, int S, float *SA, float *SV, void *workspace,
                        size_t ws_bytes);

/*
 * Subgraph ranks: FilteredRankingEval.subgraph_positions (skge/base.py:
 * 828-911) with the model's own score in both directions.  For test triple
 * i = (s, o, p) of queries[nq][3] every row x of X [S][d] (SA or SV) scores
 * as the object of (s, p, x) (tail) and as the subject of (x, p, o) (head),
 * with the query vectors and the sequential fp32 chain of the ranking entry
 * points above.  skip_tail[i] / skip_head[i]: a subgraph id that is not
 * ranked, or -1.  ans_off int64 [N + 1] / ans_sub int32: per entity the
 * ascending ids of the subgraphs whose members contain it.
 * ranks_out[2i], [2i+1] = 1 + #{eligible subgraphs scoring strictly above the
 * best-scoring eligible subgraph that contains o (tail) or s (head)}, ties in
 * the answer's favour; when no eligible subgraph contains the answer, the
 * number of eligible subgraphs + 1 and found_out = 0 (else 1).
 * d <= 1024, S > 0; ids are not range-checked here.  Workspace:
 * skge_subgraph_rank_workspace_bytes(nq, d).
 */
size_t skge_subgraph_rank_workspace_bytes(int nq, int d);
int skge_subgraph_rank(void *stream, int model, const float *E, const float *R, int N, int d,
                       const float *X, int S, const int *queries, int nq, const int *skip_tail,
                       const int *skip_head, const int64_t *ans_off, const int *ans_sub,
                       void *workspace, size_t ws_bytes, int *ranks_out, int *found_out);

/* ---------------- nearest neighbours in embedding space ---------------- */

#define SKGE_SIM_COSINE 0
#define SKGE_SIM_DOT 1

/*
 * Nearest neighbours: for each of nq queries the k rows of T [N][d] (any fp32
 * table with finite values) most similar to it; cosineMatrix + similarity of
 * the reference's eval-embeddings.py.  Exactly one query form:
 *   rows [nq]     query i is row rows[i] of T; the id rows[i] itself is never
 *                 returned (other rows with an equal vector are);
 *   Q [nq][d]     external vectors; nothing is excluded;
 *   both NULL     needs nq == N: every row in order, itself excluded.
 * Arithmetic: dot(q, j) is the fp32 fma chain over kk = 0 .. d - 1 from 0.0f
 * (what v_mfma_f32_32x32x2_f32 computes); n2_j the same chain of row j with
 * itself; r_j = n2_j == 0 ? 0 : 1 / sqrtf(n2_j), correctly rounded; SKGE_SIM_DOT
 * returns dot, SKGE_SIM_COSINE (dot * r_q) * r_j -- so a zero row has cosine
 * 0 with everything.
 * Result: ids_out / sim_out [nq][k], ordered by descending similarity, then
 * ascending id among exactly equal fp32 values (skge_topk's order); slots
 * beyond the eligible rows (k > N - 1) hold id -1 and -inf.  1 <= k <= 128,
 * d >= 1; row ids are not range-checked here.  Caller-owned buffers,
 * stream-ordered; workspace of skge_neighbours_workspace_bytes(nq, N, d, k)
 * bytes.
 */
size_t skge_neighbours_workspace_bytes(int nq, int N, int d, int k);
int skge_neighbours(void *stream, const float *T, int N, int d, const float *Q, const int *rows,
                    int nq, int metric, int k, void *workspace, size_t ws_bytes, int *ids_out,
                    float *sim_out);

/* ---------------- relation prediction ---------------- */

/*
 * The relation slot of the triple: every relation j of 0 .. M - 1 scored for a
 * pair (s, o),
 *   TransE  -sum_k |E_s[k] + R_j[k] - E_o[k]|, evaluated as -sum|q - R_j| with
 *           q = E_o - E_s (one fp32 subtract per component), the sequential
 *           chain of the ranking entry points above on row R_j;
 *   HolE    R_j . q, q = ccorr(E_s, E_o) (the chain of the ranking entry
 *           points' correlation), the same dot chain on row R_j;
 *   RESCAL  sum_a sum_b E_s[a] W_j[a][b] E_o[b]: t_b = the fp32 fma chain over
 *           a = 0 .. d - 1 from 0.0f (what v_mfma_f32_32x32x2_f32 accumulates),
 *           then sum_b t_b E_o[b] in a fixed order (no float atomics: the same
 *           bits on every run).  The true relation's score comes out of the
 *           same code as every other's.
 * E [N][d], R [M][d] (W [M][d][d] for RESCAL), d <= 1024, M >= 1.  Ids inside
 * device arrays are not range-checked here.
 *
 * skge_relrank: for test triple i = (s, o, p) of queries[nq][3],
 * ranks_out[2i] = 1 + #{relations scoring strictly above p} (ties in p's
 * favour) and ranks_out[2i + 1] = that rank - #{known relations of the pair
 * scoring strictly above p}: known_rel[known_off[i] .. known_off[i + 1]) holds
 * every p' != p with (s, o, p') known (int32, ascending, unique);
 * known_off NULL = no filter (both columns equal).  Both TransE codes are
 * scored with the L1 distance, as skge_rank / skge_rank_known do.
 *
 * skge_reltopk: for pair i = (s, o) of pairs[nq][2] the k best relations into
 * rel_out / score_out [nq][k], in skge_topk's order (descending score, then
 * ascending id among exactly equal fp32 scores), padding (-1, -inf; k > M is
 * legal) and exclusion lists (excl_off [nq + 1] / excl_rel, relation ids).
 * SKGE_TRANSE_L2 scores -sum (q - R_j)^2 here, as in skge_topk.  1 <= k <= 128.
 *
 * Caller-owned buffers, stream-ordered; nq == 0 launches nothing.  RESCAL's
 * score matrix [nq][M] lives in the workspace and is filled a block of queries
 * at a time when it would pass 256 MB; the workspace functions return what the
 * entry points need for the given model.
 */
size_t skge_relrank_workspace_bytes(int nq, int d, int M, int model);
int skge_relrank(void *stream, int model, const float *E, const float *R, int N, int M, int d,
                 const int *queries, int nq, const int *known_off, const int *known_rel,
                 void *workspace, size_t ws_bytes, int *ranks_out);
size_t skge_reltopk_workspace_bytes(int nq, int d, int k, int M, int model);
int skge_reltopk(void *stream, int model, const float *E, const float *R, int N, int M, int d,
                 const int *pairs, int nq, int k, const int *excl_off, const int *excl_rel,
                 void *workspace, size_t ws_bytes, int *rel_out, float *score_out);

/* ---------------- type-constrained ranking: candidate pools ---------------- */

/*
 * skge_rank_known and skge_topk restricted to CANDIDATE POOLS: each query
 * vector is ranked against, or selects among, the members of one pool instead
 * of all N entities -- the type-constrained protocol (a relation's range or
 * domain), or any explicit or sampled candidate list.
 *
 * The pools are a CSR as DeviceKG.pools builds it for the typed samplers
 * (skge_sampler_t): pool_off int64 [n_pools + 1], pool_ent int32, the ids
 * ASCENDING AND UNIQUE within a pool.  Pools may be empty and may overlap.
 * Pool id -1 means every entity 0 .. N - 1 (n_pools == 0 with NULL pool
 * arrays is legal: every id must then be -1).  The library groups the
 * vectors by pool on the device; they may come in any order.
 *
 * skge_rank_pools: vec_pool [2 nq], vector 2i = the tail query of test triple
 * i = (s, o, p) of queries[nq][3], vector 2i + 1 its head query.  Query
 * vectors, the true entity's score (recomputed with the counting pass's
 * arithmetic, so the true entity never outranks itself), the strict >
 * comparison and both TransE codes scored by L1 are skge_rank_known's.
 *   ranks_out[4i + 2 dir]     = 1 + #{pool members scoring strictly above the
 *                               true entity}; the true entity is a candidate
 *                               whether its pool holds it or not (it adds 0);
 *                               an empty pool gives 1;
 *   ranks_out[4i + 2 dir + 1] = that rank - #{known answers of the query that
 *                               are members of the vector's pool and score
 *                               strictly above the true entity}.
 * tail_off / tail_ent / head_off / head_ent: skge_rank_known's known-answer
 * CSR, unchanged (every known answer, true entity excluded); answers outside
 * the pool are ignored here (a binary search in the ascending pool), and
 * under pool -1 every answer counts.  With vec_pool all -1, or one explicit
 * pool 0 .. N - 1, the result equals skge_rank_known's integer for integer.
 *
 * skge_topk_pools: skge_topk (its score forms, order, padding (-1, -inf),
 * exclusion CSR, 1 <= k <= 128, k above the pool size legal) with query i
 * selecting among the members of pool query_pool[i] that are not excluded.
 *
 * Refused before any launch, with an error text: NULL arguments, a model
 * outside 0 .. 3, d > 1024, n_pools < 0, n_pools > 0 with NULL pool arrays,
 * k out of range, a workspace below the workspace function's size.  nq == 0
 * launches nothing.  Pool ids and entity ids inside device arrays are NOT
 * range-checked here (skge_amd's evaluator and predictor check them on the
 * host).  Caller-owned buffers, stream-ordered.
 */
size_t skge_rank_pools_workspace_bytes(int nq, int d, int n_pools);
int skge_rank_pools(void *stream, int model, const float *E, const float *R, int N, int d,
                    const int *queries, int nq,
                    const int64_t *pool_off, const int *pool_ent, int n_pools,
                    const int *vec_pool,
                    const int *tail_off, const int *tail_ent,
                    const int *head_off, const int *head_ent,
                    void *workspace, size_t ws_bytes, int *ranks_out);

size_t skge_topk_pools_workspace_bytes(int nq, int d, int k, int N, int n_pools);
int skge_topk_pools(void *stream, int model, const float *E, const float *R, int N, int d,
                    const int *queries, int nq, int direction, int k,
                    const int64_t *pool_off, const int *pool_ent, int n_pools,
                    const int *query_pool,
                    const int *excl_off, const int *excl_ent,
                    void *workspace, size_t ws_bytes, int *ent_out, float *score_out);

/* ---------------- link-prediction AUC and triple classification ---------------- */

/*
 * skge_score: the raw score of every explicit triple trip[i] = (s, o, p), the
 * model's own training score before any activation:
 *   SKGE_TRANSE_L1  -sum |E_s + R_p - E_o|      SKGE_TRANSE_L2  -sum (E_s + R_p - E_o)^2
 *   SKGE_HOLE       R_p . ccorr(E_s, E_o)       SKGE_RESCAL     E_s W_p E_o   (R = W [M][d][d])
 * Plain pointers: no table structs, no accumulators, nothing is updated.
 * TransE and HolE take one wave per triple; RESCAL groups the triples by
 * relation on the device and computes E_S W_p per group on the fp32 MFMA.
 * Every sum has a fixed order and there are no float atomics: the same input
 * gives the same bytes on every run.
 *
 * Refused before any launch, with an error text: a model outside 0 .. 3,
 * n < 0 (or above INT_MAX / 4), N < 1, M < 1, d outside 1 .. 1024 (the step
 * kernels' range), NULL pointers, a workspace below the workspace function's
 * size.  n == 0 launches nothing.  The ids inside trip are NOT range-checked
 * here (skge_amd checks them on the host).  Caller-owned buffers,
 * stream-ordered.  The workspace function returns 0 for sizes it refuses.
 */
size_t skge_score_workspace_bytes(int model, int n, int M, int d);
int skge_score(void *stream, int model, const float *E, const float *R, int N, int M, int d,
               const int *trip, int64_t n, void *workspace, size_t ws_bytes, float *score_out);

/*
 * skge_curve_stats: ranking-curve statistics of n labelled scores (label > 0 =
 * true), per segment seg[i] in 0 .. nseg - 1 (seg NULL: one segment).  Each
 * segment is sorted descending by score and cut into groups of exactly equal
 * score (-0.0 and +0.0 are one group, +-inf are legal).  With TP_k / FP_k the
 * cumulative counts through group k (TP_0 = FP_0 = 0), P and Nneg the totals:
 *   counts_out[4 s + 0 .. 3] = P, Nneg,
 *                              2U = sum_k (FP_k - FP_k-1)(TP_k + TP_k-1)
 *                                   (ROC-AUC = 2U / (2 P Nneg)),
 *                              best_correct = max over cuts k >= 0 of
 *                                             TP_k + (Nneg - FP_k);
 *   areas_out[2 s + 0]       = sum_k (TP_k - TP_k-1) / P . (prec_k + prec_k-1) / 2,
 *                              prec_k = TP_k / (TP_k + FP_k), prec_0 = 1: the
 *                              trapezoid under the precision-recall points;
 *   areas_out[2 s + 1]       = sum_k (TP_k - TP_k-1) / P . prec_k (average precision);
 *   thresh_out[s]            = the score of the best cut's last group (the
 *                              smallest k among equal maxima), +inf for cut 0
 *                              ("predict none"); the rule is score >= thresh.
 * The integers are exact.  The doubles use IEEE division and a summation tree
 * fixed by (n, nseg): two runs give equal bytes.  An empty segment gives
 * zeros, NaN areas and +inf; P == 0 or Nneg == 0 gives NaN areas.
 *
 * *status_out is cleared first, then: bit 1 = a NaN score, bit 2 = a segment
 * id outside 0 .. nseg - 1.  With a bit set NO result is written.
 *
 * Refused before any launch: n < 0 (or above INT_MAX - 2048), nseg < 1, NULL
 * pointers (score / label may be NULL when n == 0), a workspace below the
 * workspace function's size (0 = sizes refused, or no device to size the sort
 * for).  n == 0 is legal.  Caller-owned buffers, stream-ordered.
 */
size_t skge_curve_stats_workspace_bytes(int64_t n, int nseg);
int skge_curve_stats(void *stream, const float *score, const signed char *label, const int *seg,
                     int64_t n, int nseg, void *workspace, size_t ws_bytes,
                     long long *counts_out, double *areas_out, float *thresh_out, int *status_out);

#ifdef __cplusplus
}
#endif
#endif /* SKGE_HIP_H */
