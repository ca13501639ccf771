// Host-side helpers for the C ABI: error reporting and argument checks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/skge_hip.h"
#include "skge_device.h"

namespace skge {

void set_error(const char* fmt, ...);

#define SKGE_CHECK_ARG(cond, ...)            \
  do {                                       \
    if (!(cond)) {                           \
      ::skge::set_error(__VA_ARGS__);        \
      return SKGE_EINVAL;                    \
    }                                        \
  } while (0)

#define SKGE_CHECK_LAUNCH(what)                                                   \
  do {                                                                            \
    hipError_t _e = hipGetLastError();                                            \
    if (_e != hipSuccess) {                                                       \
      ::skge::set_error("%s: %s", what, hipGetErrorString(_e));                   \
      return SKGE_EHIP;                                                           \
    }                                                                             \
  } while (0)

#define SKGE_CHECK_HIP(call)                                                      \
  do {                                                                            \
    hipError_t _e = (call);                                                       \
    if (_e != hipSuccess) {                                                       \
      ::skge::set_error("%s: %s", #call, hipGetErrorString(_e));                  \
      return SKGE_EHIP;                                                           \
    }                                                                             \
  } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// workspace parts start on 256-byte boundaries
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// The grid of a pass that crosses `blocks` query blocks with `tiles` units of
// the other operand (128-row tiles of a table; relations): about 2048
// workgroups, enough to fill the chip.  ns slices of `per` units each.
struct SlicePlan {
  int per, ns;
};
inline SlicePlan slice_plan(int blocks, int tiles) {
  const int want = std::max(1, std::min(tiles, (2048 + blocks - 1) / std::max(1, blocks)));
  const int per = (tiles + want - 1) / want;
  return {per, (tiles + per - 1) / per};
}

// registers per lane needed to hold a row of width d in the lane-strided
// layout (see skge_device.h); 0 = unsupported
inline int km_for(int d) {
  if (d <= 64) return 1;
  if (d <= 128) return 2;
  if (d <= 192) return 3;
  if (d <= 256) return 4;
  if (d <= 512) return 8;
  if (d <= 1024) return 16;
  return 0;
}

// the model codes of include/skge_hip.h: 0..3, 5, 6, 7 (4 is unassigned)
inline bool model_known(int model) {
  return (model >= SKGE_TRANSE_L1 && model <= SKGE_RESCAL) || model == SKGE_DISTMULT ||
         model == SKGE_COMPLEX || model == SKGE_ROTATE;
}
// a code's name for an error text: the one code-to-name table
inline const char* model_name(int model) {
  switch (model) {
    case SKGE_TRANSE_L1: return "TransE-L1";
    case SKGE_TRANSE_L2: return "TransE-L2";
    case SKGE_HOLE: return "HolE";
    case SKGE_RESCAL: return "RESCAL";
    case SKGE_DISTMULT: return "DistMult";
    case SKGE_COMPLEX: return "ComplEx";
    case SKGE_ROTATE: return "RotatE";
    default: return "?";
  }
}
// rows of d/2 interleaved complex components: ComplEx and RotatE
inline bool model_complex_rows(int model) { return model == SKGE_COMPLEX || model == SKGE_ROTATE; }
// DistMult / ComplEx: HolE's table shapes and slot maps, skge_diag.h's scores
inline bool model_diag(int model) { return model == SKGE_DISTMULT || model == SKGE_COMPLEX; }
// the model's code and width: ComplEx and RotatE rows hold d/2 interleaved
// (re, im) pairs
#define SKGE_CHECK_MODEL(model, d)                                                       \
  do {                                                                                   \
    SKGE_CHECK_ARG(::skge::model_known(model), "unknown model %d", model);               \
    SKGE_CHECK_ARG((model) != SKGE_COMPLEX || (d) % 2 == 0, "ComplEx needs an even d (%d)", d); \
    SKGE_CHECK_ARG((model) != SKGE_ROTATE || (d) % 2 == 0, "RotatE needs an even d (%d)", d); \
  } while (0)
// an entry point RotatE is not served by (include/skge_hip.h, SKGE_ROTATE)
#define SKGE_REFUSE_ROTATE(model, who)                                                   \
  SKGE_CHECK_ARG((model) != SKGE_ROTATE, "%s: RotatE is not served here", who)

// SKGE_POST_UNITMOD is applied by the row applies of skge_update.hip only
// (update_row, apply_row, apply_row_rep_block).  Every other consumer of a
// table would read "not NONE and not NORMALIZE" as normless1, so it refuses the
// code by name first: true (and the error text) when t carries it.
inline bool refuses_unitmod(const skge_table_t* t, const char* who) {
  if (!t || t->post != SKGE_POST_UNITMOD) return false;
  set_error("%s: post SKGE_POST_UNITMOD (unit-modulus components, RotatE's relation table) is "
            "not served here; use the per-batch step or the pair loop", who);
  return true;
}
// what a table with SKGE_POST_UNITMOD must be for the row applies
inline int check_unitmod(const skge_table_t* t) {
  if (t->post != SKGE_POST_UNITMOD) return SKGE_OK;
  SKGE_CHECK_ARG(t->width % 2 == 0 && t->width <= 1024,
                 "post SKGE_POST_UNITMOD needs an even width <= 1024 (%d)", t->width);
  SKGE_CHECK_ARG(t->acc_mode == SKGE_ACC_F32 || t->acc_mode == SKGE_ACC_FX64,
                 "post SKGE_POST_UNITMOD needs fp32 or fixed-point sums (acc_mode %d)", t->acc_mode);
  return SKGE_OK;
}

int* dev_err_word();   // skge_update.hip: the device error word (Accum::err)
inline Accum accum_of(const skge_table_t* t) {
  Accum a;
  a.sum = t->acc_sum;
  a.cnt = t->acc_cnt;
  a.touched = t->acc_touched;
  a.width = t->width;
  a.mode = t->acc_mode;
  a.replicas = t->acc_replicas > 1 ? t->acc_replicas : 1;
  a.rows = t->rows;
  a.err = t->acc_mode == SKGE_ACC_FX64 ? dev_err_word() : nullptr;
  return a;
}

inline int check_table(const skge_table_t* t, const char* name, bool need_acc) {
  SKGE_CHECK_ARG(t != nullptr, "%s: table is NULL", name);
  SKGE_CHECK_ARG(t->param != nullptr, "%s: param is NULL", name);
  SKGE_CHECK_ARG(t->rows > 0 && t->width > 0, "%s: bad shape %d x %d", name, t->rows, t->width);
  SKGE_CHECK_ARG(t->acc_mode == SKGE_ACC_F32 || t->acc_mode == SKGE_ACC_I16X4 ||
                     t->acc_mode == SKGE_ACC_FX64,
                 "%s: unknown accumulator mode %d", name, t->acc_mode);
  SKGE_CHECK_ARG(t->acc_mode != SKGE_ACC_FX64 || (t->width <= 1024 && t->acc_replicas <= 1),
                 "%s: the deterministic (fixed-point) accumulator needs width <= 1024 and one "
                 "copy", name);
  // (the fixed-point sums are one int64 per element, added and applied element
  // by element -- acc_row, mean_row, apply_row: any width, bounded above)
  SKGE_CHECK_ARG(t->acc_mode == SKGE_ACC_F32 || t->acc_mode == SKGE_ACC_FX64 ||
                     (t->width % 4 == 0 && t->width <= 1024),
                 "%s: packed accumulator needs width %% 4 == 0 and <= 1024", name);
  // packed sums are TransE-L1's exact integer sign sums: no regularisation
  // terms and the occurrence count as the divisor (the packed applies' fast
  // AdaGrad step / projection forms are argued for exactly that case,
  // skge_device.h adagrad_step_fast)
  SKGE_CHECK_ARG(t->acc_mode != SKGE_ACC_I16X4 ||
                     (t->rin == 0.0f && t->rout == 0.0f && t->fixed_div <= 0.0f),
                 "%s: packed accumulator needs rin == rout == 0 and no fixed divisor", name);
  if (need_acc) {
    SKGE_CHECK_ARG(t->acc_sum && t->acc_cnt, "%s: accumulator buffers missing", name);
  }
  SKGE_CHECK_ARG(t->acc_replicas <= 1 || t->acc_touched == nullptr,
                 "%s: replicated accumulators must be dense (acc_touched NULL)", name);
  SKGE_CHECK_ARG(t->acc_replicas <= 1 || t->acc_replicas == 2 || t->acc_replicas == 4 ||
                     t->acc_replicas == 8 || t->acc_replicas == 16 || t->acc_replicas == 32,
                 "%s: acc_replicas must be 1, 2, 4, 8, 16 or 32", name);
  return SKGE_OK;
}

// producers that do not spread over replicas
inline int check_single(const skge_table_t* t, const char* name) {
  SKGE_CHECK_ARG(t->acc_replicas <= 1, "%s: this producer needs a single accumulator copy", name);
  return SKGE_OK;
}

// producers that only write fp32 accumulators
inline int check_f32(const skge_table_t* t, const char* name) {
  // float-valued sums: fp32 atomics, or the deterministic fixed-point form
  // (producers add through acc_row, which handles both)
  SKGE_CHECK_ARG(t->acc_mode == SKGE_ACC_F32 || t->acc_mode == SKGE_ACC_FX64,
                 "%s: this producer needs an fp32 (or fixed-point) accumulator", name);
  return SKGE_OK;
}

// slot records: a table without acc_touched is dense (nothing recorded)
inline int check_slots(const skge_table_t* t, long long nslots, const char* name) {
  if (t->acc_touched == nullptr) return SKGE_OK;
  SKGE_CHECK_ARG(nslots >= 0 && nslots <= t->touched_cap,
                 "%s: %lld touched slots needed, capacity %d", name, nslots, t->touched_cap);
  return SKGE_OK;
}

// the arguments of a stand-alone epoch draw (skge_epoch_sample_ex / _multi,
// skge_pipe_epoch_sample): out0 / out1 its two output arrays, ntries_min 1, or
// 0 for the pipelined draw
inline int check_sample_args(const void* trip, const void* set, const void* epoch_key,
                             const void* out0, const void* out1, int64_t T, int64_t set_capacity,
                             int n_ent, int ntries, int ntries_min) {
  SKGE_CHECK_ARG(trip && set && epoch_key && out0 && out1, "NULL argument");
  SKGE_CHECK_ARG(T > 0 && T <= INT32_MAX, "T must be in [1, 2^31)");
  SKGE_CHECK_ARG(set_capacity >= 2 * T && !(set_capacity & (set_capacity - 1)),
                 "set capacity must be a power of 2 >= 2T");
  SKGE_CHECK_ARG(n_ent > 0 && ntries >= ntries_min, "bad n_ent / ntries");
  return SKGE_OK;
}

inline TripleSet triple_set_view(const void* set, int64_t capacity) {
  TripleSet ts;
  ts.slots = (const int4*)set;
  ts.filter = (const uint32_t*)((const int4*)set + capacity);
  ts.mask = (uint64_t)(capacity - 1);
  ts.fmask = (uint64_t)(8 * capacity - 1);
  return ts;
}

// skge_eval.hip: the ranking entry points' steps, for callers that rank rows
// of another table (skge_subgraph.hip).  launch_rank_query: the query vectors
// of nq test triples (s, o, p) into Q [2 nq][d] (2i: tail, 2i + 1: head) and
// the true entities' scores into tgt [2 nq].  launch_rank_count: raw[v] +=
// #{rows of T [rows][d] scoring strictly above tgt[v] under Q[v]}, v < nv
// (l1: the L1 distance, else the dot product; rank_score's chain).
void launch_rank_query(hipStream_t st, int model, const float* E, const float* R, int N, int d,
                       const int* queries, int nq, float* Q, float* tgt);
void launch_rank_count(hipStream_t st, bool l1, const float* T, int rows, int d, const float* Q,
                       const float* tgt, int nv, int* raw);
// ... with the form named: RT_L1, RT_DOT or RT_CMOD (skge_rank_tile.h)
void launch_rank_count_form(hipStream_t st, int form, const float* T, int rows, int d,
                            const float* Q, const float* tgt, int nv, int* raw);

// skge_topk.hip: the top-k selection and merge, for callers that select rows
// of another table (skge_relation.hip).  For query vectors Q [nq][d] the k best
// rows of T [rows][d] into ent_out / score_out [nq][k] in skge_topk's order
// and padding; model picks the score's form as skge_topk does (TRANSE_L1:
// -sum|q - T_j|, TRANSE_L2: -sum (q - T_j)^2, else the dot product); excl_*:
// skge_topk's exclusion CSR over row ids.  lists: topk_lists_bytes(nq, k,
// rows) bytes of workspace.
//
// With a grouped work list over n_pools >= 0 pools (skge_pools.h), the
// selection is GATHERED: query i selects among the rows its pool lists (the
// ids returned are the pool's entries), the query blocks are the list's items
// (built with topk_block_size(k) vectors per item) and every pool is cut into
// the plan's slices (pools->ns is set here).
// launch_topk_query: skge_topk's query vectors (anchor, p) of one direction
// into Q [nq][d].
// launch_list_merge: the merge alone (k_list_merge), for a selection of
// another kind (skge_neighbours.hip): each query's ns sorted lists [nq][ns][k]
// of keys (skge_topk_list.h) into its k best, decoded.
struct PoolWork;
void launch_list_merge(hipStream_t st, const void* lists, int nq, int ns, int k, int* ids_out,
                       float* score_out);
void launch_topk_query(hipStream_t st, int model, const float* E, const float* R, int d,
                       const int* queries, int nq, int direction, float* Q);
int topk_block_size(int k);
size_t topk_lists_bytes(int nq, int k, int rows, int n_pools = -1);
void launch_topk_select(hipStream_t st, int model, const float* T, int rows, int d, const float* Q,
                        int nq, int k, const int* excl_off, const int* excl_ent, void* lists,
                        int* ent_out, float* score_out, const PoolWork* pools = nullptr,
                        int n_pools = -1);

// skge_pools.hip: group nv query vectors by pool id (vec_pool [nv], -1 = all
// entities) into items of up to bsz vectors.  pool_items_max: the bound on the
// item count the consumers size their grids with; pool_group_bytes: the
// workspace launch_pool_group needs (16-B aligned base).  *w: the list, its
// arrays inside ws.
int pool_items_max(int nv, int n_pools, int bsz);
size_t pool_group_bytes(int nv, int n_pools, int bsz);
int launch_pool_group(hipStream_t st, const int* vec_pool, int nv, int n_pools, int bsz,
                      const int64_t* pool_off, const int* pool_ent, void* ws, PoolWork* w);

// skge_pipeline.hip: draw every negative of the epoch whose key is *epoch_key
// (rec[j] = (s, o, p, s' or -1), rec_n1[j] = o' or -1 for positive j of the
// epoch's order) with the sampler smp (nullptr: RANDOM, k_epoch_sample as the
// pipelined runners launch it; check_sampler first)
int launch_epoch_sample(hipStream_t st, const int* trip, long long T, uint64_t seed,
                        const uint64_t* epoch_key, TripleSet set, int n_ent, int ntries,
                        int4* rec, int* rec_n1, const skge_sampler_t* smp = nullptr);
// SKGE_EINVAL (and the error text) for an unknown kind or, for a pool kind,
// n_rel <= 0 or NULL pools; the pools' contents are not read
int check_sampler(const skge_sampler_t* smp, const char* who);
// skge_pipeline.hip: the n-negatives draw (include/skge_hip.h,
// skge_negatives_t).  check_negatives: SKGE_EINVAL (and the error text) for
// the refusals listed there; *K = n * nmodes.  launch_epoch_sample_multi:
// pos [T][3], neg [T][K] of the epoch whose key is *epoch_key (both checks
// first).
int check_negatives(const skge_negatives_t* negs, const skge_sampler_t* smp, int n_rel,
                    const char* who, int* K);
int launch_epoch_sample_multi(hipStream_t st, const int* trip, long long T, uint64_t seed,
                              const uint64_t* epoch_key, TripleSet set, int n_ent, int n_rel,
                              int ntries, int* pos, int* neg, const skge_sampler_t* smp,
                              const skge_negatives_t* negs);
// skge_grad.hip: TransE with K negatives per positive, one wave per positive
// (k_transe_pos_multi): batch positives [start, start + count) of pos3 [T][3]
// / negK [T][K] scored, margin-tested and accumulated; slots per positive:
// 2 + K entity, 1 + K relation.  *nviol += the violating pairs.
struct Negatives;
int launch_transe_pos_multi(hipStream_t st, int l1, const skge_table_t* ent,
                            const skge_table_t* rel, int d, const int* pos3, const int* negK,
                            long long start, int count, const Negatives& ng, float margin,
                            int* nviol);

// skge_grad.hip: the self-adversarial loss (TransE-L1 / -L2, RotatE), one wave
// per positive and its K slots (k_sadv_pos).  check_sadv: what every entry
// point of the loss refuses before any launch, by name (the model, odd d for
// RotatE, d > 1024, non-finite gamma / alpha, alpha < 0, check_negatives' list,
// packed sums, a replicated entity table, check_unitmod); *K = n * nmodes.
// launch_sadv_pos: batch positives [start, start + count) scored, weighted and
// accumulated (slots per positive: 2 + K entity, 1 + K relation; a smaller
// table is refused with the count needed); *loss += the batch's loss; pscore
// [count], nscore [count][K], coef [count][1 + K] optional.
int check_sadv(const char* who, int model, const skge_table_t* ent, const skge_table_t* rel, int d,
               const skge_negatives_t* negs, const skge_sampler_t* smp, float gamma, float alpha,
               int* K);
int launch_sadv_pos(hipStream_t st, int model, const skge_table_t* ent, const skge_table_t* rel,
                    int d, const int* pos3, const int* negK, long long start, int count,
                    const Negatives& ng, float gamma, float alpha, float* pscore, float* nscore,
                    float* coef, float* loss);

// skge_grad.hip: HolE pairwise, one positive (both of its pairs) per wave
bool hole_pos_ok(int af, const skge_table_t* ent, const skge_table_t* rel, int d);
// the per-positive HolE kernels run their correlations through the wave FFT
// (skge_hole_fft.h) for this d (unless SKGE_HOLE_DIRECT=1)
bool hole_use_fft(int d);
// the kernels launch_pair runs for a HolE batch of width d (SKGE_PATH_GENERIC /
// _HOLE_FAST / _HOLE_FFT; record: the call scatters contributions)
int hole_step_path(int d, bool logistic_mode, bool record);
int launch_hole_pos(hipStream_t st, int af, const skge_table_t* ent, const skge_table_t* rel,
                    int d, const int4* rec, const int* rec_n1, long long start, int count,
                    float margin, int* nviol, int* fold, int* total);

// skge_grad.hip: DistMult / ComplEx pairwise, one positive (both of its pairs)
// per wave (k_diag_pos): d <= 256, fp32 or fixed-point sums, one entity copy
bool diag_pos_ok(int model, int af, const skge_table_t* ent, const skge_table_t* rel, int d);
int launch_diag_pos(hipStream_t st, int model, int af, const skge_table_t* ent,
                    const skge_table_t* rel, int d, const int4* rec, const int* rec_n1,
                    long long start, int count, float margin, int* nviol);

// skge_grad.hip: RotatE pairwise, one positive (both of its pairs) per wave
// (k_rot_pos): even d <= 256, fp32 or fixed-point sums, one entity copy
bool rot_pos_ok(int model, const skge_table_t* ent, const skge_table_t* rel, int d);
int launch_rot_pos(hipStream_t st, const skge_table_t* ent, const skge_table_t* rel, int d,
                   const int4* rec, const int* rec_n1, long long start, int count, float margin,
                   int* nviol);

// The RESCAL W updater's step after the fused front (skge_rescal.hip
// k_rescal_front_fused): W[p] from relation p's split-K dW partial tiles,
// gated on the batch's violations; run by the entity apply's launch
// (skge_update.hip k_apply_wstep).  part == nullptr: no W step pending.
struct WStep {
  const float* part;      // [M][nt * nt][splits][64 * 64]
  const int* rel_off;     // [M + 1] the batch's relation bucket offsets
  const int* dwcnt;       // [M] dW items per relation (combined dW), or nullptr: the buckets
  float* W;
  float* A;               // AdaGrad state or nullptr
  int* ucnt;              // optional updateCounts
  const int* gate;        // the batch's violation count
  int M, d, splits, opt;
  float lr, rin, rout, fdiv;
  // the W step done inside the fused front, speculatively into the other
  // buffer (one dW split per tile): the apply only makes it current when the
  // batch has violations (*cur ^= 1); cur == nullptr: the step above
  int* cur;               // 0: W_b in W / A (the caller's), 1: in W1 / A1
  float* W1;
  float* A1;
  // set by the row-grouped RESCAL apply (skge_rescal.hip k_rescal_fold): the
  // entity rows and the W step's flip are done; only the epoch end's W sync
  // (cur) is left to the caller
  int applied;
};
int apply_with_wstep(hipStream_t st, const skge_table_t* ent, int nslots, const WStep& w);
// end of an epoch with the in-front W step: the current buffer back into the
// caller's W / state, cur = 0 (skge_rescal.hip)
int rescal_w_sync(hipStream_t st, const WStep& w);

}  // namespace skge

// skge_rescal.hip / skge_update.hip: the device pair loop's RESCAL batch
bool rescal_pair_mfma_selected(int d, int M);
// rescal_front buckets n triples over M relations in one workgroup
// (k_rs_bucket_small) rather than by count / scan / scatter (skge_rescal.hip)
bool rs_small_bucket(int M, int n);
// the device pair loop's RESCAL buckets for a whole epoch (skge_rescal.hip)
bool rescal_epoch_ok(int M);
size_t rescal_epoch_ws_bytes(int bs, int nb, int M, int d);
int rescal_epoch_bucket(hipStream_t st, const int* pos, const int* neg, long long T, int bs, int nb,
                        int M, int d, void* ws, const int4* rec = nullptr,
                        const int* rec_n1 = nullptr);
// the epoch's row grouping fits (k_rs_rows_ep: 4 bs slots per batch in LDS)
bool rs_rows_ok(int bs);
int skge_rescal_pos_grad_mfma_ep(hipStream_t st, int af, const skge_table_t* ent,
                                 const skge_table_t* rel, int d, const int4* rec,
                                 const int* rec_n1, long long T, int bs, int nb, int b,
                                 float margin, void* ws, int* nviol,
                                 skge::WStep* wstep = nullptr);
int skge_rescal_pos_grad_mfma(hipStream_t st, int af, const skge_table_t* ent,
                              const skge_table_t* rel, int d, const int* pos, const int* neg,
                              const int4* rec, const int* rec_n1, long long start, int count,
                              float margin, void* workspace, size_t ws_bytes, int* nviol);
