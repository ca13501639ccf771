// The pipelined runner's plan (skge_pipeline.hip pipe_create, the
// skge_pipe_runner_plan export): its form, its launches and the bytes of every
// buffer it allocates, decided once from the tables' geometry.  Host code with
// no HIP header behind it: it compiles with the host compiler alone, and
// nothing here touches a device.  What lives in HIP headers or the
// environment comes in through PipeEnv.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/skge_hip.h"
#include "skge_epoch_batches.h"

namespace skge {

// hot rows (PipeTab::hot): replicas per row; a row is hot when its expected
// slots per batch are >= HOT_MIN and >= HOT_REL x the average row's; at most
// HOT_MAX rows.  WN18 Zipf(1.1), nb = 100, same box: HOT_MIN 16 / 8 / 4 ->
// 110.6 / 116.1 / 117.4 M triples/s (4 replicas); 16 replicas 108.2 M (the
// readers' fold: 97 VGPRs, 4 waves per SIMD; 4 replicas: 74 VGPRs, 6).  The
// relative bar keeps a uniform KG's rows at large batches out (WN18 nb = 2:
// ~3.5 slots per row and batch; hot rows there cost 531 / 519 vs 540 M).
// (HOT_MIN 2 / 3, HOT_REL 4: within noise of these, same box)
constexpr int HOT_REPS = 4, HOT_MIN = 4, HOT_REL = 8, HOT_MAX = 256;

// the fused kernel's slot records name a row and its buffer: row | buffer << 30
constexpr int SLOT_BUF = 1 << 30;

// large batches (owner marks, k_pipe_batch's GRP instances): 3-wave
// workgroups (WN18 nb = 2, same box: 508-510 -> 520 M triples/s; 128: 517 M;
// nb = 100 unchanged by either, so it keeps SKGE_PIPE_WG)
constexpr int PIPE_WG_GRP = 192;
#ifndef SKGE_PIPE_WG
#define SKGE_PIPE_WG 256   // threads per workgroup
#endif

constexpr int HPIPE_OCC = 2;   // HolE: scoring waves per SIMD the apply-workgroup cap assumes (direct form)

// What the plan takes from outside this header (skge_pipeline.hip pipe_env,
// the one place that reads the switches).
struct PipeEnv {
  int fused = -1;          // SKGE_PIPE_FUSED: -1 unset, else 0 / 1
  int rreps = 0;           // SKGE_HPIPE_RREPS: 0 unset
  bool hole_fft = false;   // hole_use_fft(d)
  bool hole_hot = true;    // SKGE_HPIPE_HOT: the HolE pair form looks for hub rows
  // HolE, dynamic LDS per workgroup: the FFT form with one wave's region (the
  // pair form) and with a workgroup's, the direct form
  size_t lds_fft_wave = 0, lds_fft_wg = 0, lds_direct_wg = 0;
  int shard_words = 0;     // NSHARD * SHARD_STRIDE: ints of one sharded counter
};

struct PipeLaunch {        // a batch launch (the last one: the flush, count 0)
  long long start;
  int count, prev_slots, pprev_slots, nwork, nA, grid;
};

// Bytes of the runner's buffers, one entry per kind of buffer; total() counts
// how many of each the form allocates (pipe_create compares its requests with
// it).
struct PipeBytes {
  size_t ent_rows = 0;   // a copy of the entity parameters / AdaGrad state (fused)
  size_t ent_sum = 0;    // one more copy of the entity sums
  size_t ent_word = 0;   // a word per entity row (count, done, pending, owner, hot index)
  size_t ent_meta = 0;   // fused: the meta words
  size_t slots = 0;      // a batch's slot records
  size_t rel_rows = 0;   // the relation parameters' / AdaGrad state's other buffer
  size_t rel_acc = 0;    // one copy of the relation sums (all replicas)
  size_t rec = 0, rec_n1 = 0, err = 0, key_copy = 0, stats = 0, viol = 0;
  // per hot row: one replica copy of its sums and counts, its value, its index
  size_t hot_sum = 0, hot_cnt = 0, hot_val = 0, hot_row = 0;
};

struct PipePlan {
  // the form
  bool hole = false;     // HolE pairwise (k_hole_pipe, fp32 sums)
  bool dp = false;       // data-parallel form (SKGE_PIPE_DP): driven launch by launch
  bool e8 = false;       // int8x4 entity sums (SKGE_ACC_I8X4: per-batch counts <= 127)
  bool w32 = false;      // int32x2 relation sums
  bool grouped = false;  // large batches: owner marks (k_pipe_batch's GRP instances)
  bool fused = false;    // TransE: k_pipe_fused (nothing waits; d <= 64 by default)
  bool fft = false;      // HolE: correlations in the frequency domain (skge_hole_fft.h)
  bool pair = false;     // HolE FFT, d = 200: two waves per positive (while 2 x B waves fit the chip)
  bool hot = false;      // hot rows are looked for (find_hot_rows)
  bool ent_ada = false, rel_ada = false;   // AdaGrad state beside the parameters
  int kq = 1;            // quads per lane (1, 2 or 4: the kernels' KQ)
  int reps = 1, rw = 0;  // relation sums: replicas, 8-B words per row
  bool rfold = false;    // replicas folded after each batch launch (k_rel_fold*)
  size_t lds = 0;        // HolE: dynamic LDS per workgroup
  int wpb = 0;           // waves per workgroup
  int hw = 0;            // hot rows: 8-B words per replica row
  // the geometry it was made for
  int N = 0, M = 0, d = 0, nb1 = 0;
  long long T = 0;
  int64_t bs = 0;
  EpochBatches batches;
  // the launches: nb1 batches and the flush
  std::vector<PipeLaunch> launch;
  PipeBytes bytes;

  int threads() const { return pair ? 128 : (grouped ? PIPE_WG_GRP : SKGE_PIPE_WG); }
  int nlaunch() const { return nb1 + 3; }   // the draw, the batches, the flush, the key advance
  int kernel() const { return hole ? 2 : (fused ? 1 : 0); }   // skge_pipe_runner_kernel's code

  // scoring workgroups of n positives (0: none; the pair form: one positive each)
  int score_groups(int n) const {
    if (n <= 0) return 0;
    return pair ? std::max(1, std::min(n, 2 * 16384))
                : std::max(1, std::min((n + wpb - 1) / wpb, 16384));
  }

  // bytes the runner allocates with nhot hot rows
  size_t total(int nhot) const {
    const PipeBytes& b = bytes;
    size_t n = b.rec + b.rec_n1 + b.err + b.key_copy + b.stats + b.viol;
    n += b.rel_rows * (rel_ada ? 2 : 1) + 3 * b.rel_acc;
    if (fused) {
      // the second row buffer, the other two accumulator copies, the meta words
      n += b.ent_rows * (ent_ada ? 2 : 1) + 2 * (b.ent_sum + b.ent_word + b.slots) + b.ent_meta;
    } else {
      // a second accumulator copy, slot records, done words, batch marks
      // (both parities; large batches: owner marks too)
      n += b.ent_sum + b.slots + (grouped ? 6 : 4) * b.ent_word;
    }
    if (nhot > 0)
      n += b.ent_word + (size_t)nhot * (b.hot_row + 3 * (b.hot_sum + b.hot_cnt) +
                                        (ent_ada ? 4 : 2) * b.hot_val);
    return n;
  }
  // the figure before the hot rows are known: an UPPER BOUND, HOT_MAX of them
  size_t device_bytes() const { return total(hot ? HOT_MAX : 0); }
};

// Grids and apply shares of the launches, for nhot hot rows (known only after
// find_hot_rows; pipe_plan fills them for none).
inline void pipe_plan_launches(PipePlan& p, int nhot) {
  const EpochBatches& batches = p.batches;
  const int nb1 = p.nb1, WPB = p.wpb;
  p.launch.clear();
  for (int b = 0; b <= nb1; ++b) {   // b == nb1: flush of the last batch (no scoring)
    PipeLaunch a = {};
    a.start = b < nb1 ? batches[b].first : 0;
    a.count = b < nb1 ? (int)batches[b].second : 0;
    const int cprev = b >= 1 ? (int)batches[b - 1].second : 0;
    a.prev_slots = 4 * cprev;
    if (p.fused) {
      // one kind of wave: relation rows, then max(this, the previous and the
      // pre-previous batch's positives) work items.  The epoch starts clean (the
      // flush zeroes both copies it leaves), so the first two launches have no
      // pre-previous slots to zero
      const int cpp = b >= 2 ? (int)batches[b - 2].second : 0;
      a.pprev_slots = 4 * cpp;
      a.nwork = a.count + std::max(cprev, cpp);   // scoring items, then slot groups
      a.nA = 0;
      a.grid = std::max(1, (p.M + a.nwork + WPB - 1) / WPB);
      p.launch.push_back(a);
      continue;
    }
    // A role: every relation row, then the previous batch's entity slots
    // (owner marks: 64-slot groups)
    const int a_items = p.M + nhot +
                        (p.hole ? 4 * cprev
                         : p.grouped ? (4 * cprev + 63) / 64 : 4 * cprev);
    // HolE: the apply waves loop over their items within the residency the
    // scoring waves leave (direct form: 2 waves per SIMD at ~180 VGPRs; FFT: 4
    // -- caps 150 / 250 / 400 / 600 / 800 / 1100 on WN18 d = 200: 74.7 / 77.6 /
    // 80.5 / 81.7 / 75.4 / 70.5 M triples/s; the flush has the chip to itself)
    // (pair: two waves per positive, one positive per workgroup)
    auto nBwaves = [&](long long cnt) { return p.pair ? 2 * cnt : (cnt + WPB - 1) / WPB * WPB; };
    const int occ = p.pair ? std::max(4, HPIPE_OCC) : p.fft ? 4 : HPIPE_OCC;
    int a_cap = p.hole && b < nb1 ? std::max(1, (occ * 4 * 256 - (int)nBwaves(batches[b].second)) / WPB - 8) : 16384;
    // (large batches: more scoring waves than the chip holds -- they run in
    // rounds anyway -- so the apply waves get a fixed share instead of the
    // residency left over, which would be none: nb = 2 on WN18 had 4 apply
    // waves for 283k slot records, 42 ms per epoch)
    if (p.hole && b < nb1 && (long long)nBwaves(batches[b].second) > occ * 4 * 256)
      a_cap = std::max(a_cap, 256);
    a.nA = std::max(1, std::min((a_items + WPB - 1) / WPB, std::min(a_cap, 16384)));
    a.grid = a.nA + p.score_groups(a.count);
    p.launch.push_back(a);
  }
}

// The plan of a runner over tables of ent's and rel's geometry (rows, width,
// acc_mode, opt and whether there is AdaGrad state; no pointer is
// dereferenced), already accepted by pipe_create's refusals.
inline PipePlan pipe_plan(const skge_table_t* ent, const skge_table_t* rel, int d, int64_t T,
                          int nbatches, int flags, bool hole, const PipeEnv& env) {
  PipePlan p;
  p.hole = hole;
  p.dp = (flags & SKGE_PIPE_DP) != 0;
  p.batches = epoch_batches(T, nbatches);
  p.nb1 = p.batches.size();
  p.bs = p.batches.bs;
  p.T = T;
  p.d = d;
  const int64_t bs = p.bs, maxb = p.batches.maxb;
  const int nq = d / 4;
  const int N = p.N = ent->rows, M = p.M = rel->rows;
  // HolE at d = 200 in the FFT form: two waves per positive (the pair form)
  // while the batch's 2 x B scoring waves fit the chip's 4-wave-per-SIMD
  // residency.  WN18 d = 200, same box: nb = 100 93.7 -> 106.7 M triples/s
  // (14.6 -> 12.8 us per launch); nb = 2 (70k positives per launch) 157 ->
  // 142 M, so off there
  p.fft = hole && env.hole_fft;
  p.pair = p.fft && d == 200 && 2 * maxb <= 4 * 4 * 256;
  p.e8 = !hole && ent->acc_mode == SKGE_ACC_I8X4;
  p.w32 = rel->acc_mode == SKGE_ACC_I32X2;
  p.kq = (nq + 63) / 64;
  // large batches (more than 16k slot records): owner marks, k_pipe_batch's A
  // role scans its slots 64 at a time
  p.grouped = !hole && 4 * bs > 4 * 4096;
  // TransE below that: k_pipe_fused for rows of up to 64 floats (WN18 d = 50
  // on its 64-wide padded tables: 10.52 -> 10.08 us per launch, same box),
  // k_pipe_batch above (d = 200: 8.48 vs 9.78 us -- at 800-B rows the fused
  // kernel's second-buffer loads and rotating copies cost more than its
  // waits save).  SKGE_PIPE_FUSED=0 / 1 forces either (d <= 256).
  {
    const bool ok = !hole && !p.grouped && nq <= 64 && (long long)N < SLOT_BUF;
    p.fused = ok && !p.dp && (env.fused >= 0 ? env.fused != 0 : nq <= 16);
  }
  // (the data-parallel form keeps every row in the tables: no hot rows;
  // HolE: the pair form only, fp32 sums of d floats per replica row)
  p.hot = !p.fused && !p.e8 && !p.dp && (!hole || (p.pair && env.hole_hot));
  p.hw = ((hole ? d / 2 : nq) + 15) / 16 * 16;   // 8-B words per replica row: whole 128-B lines
  p.ent_ada = ent->opt == SKGE_ADAGRAD && ent->state != nullptr;
  p.rel_ada = rel->opt == SKGE_ADAGRAD;
  // HolE (fp32 sums, float atomics): at large batches every relation row
  // takes thousands of adds per launch, which serialise on its addresses;
  // spread them over replicas (one per ~2k positives, <= 32; 1 at nb = 100)
  p.reps = 1;
  if (hole)
    while (p.reps < 32 && (long long)p.reps * 2048 < bs) p.reps *= 2;
  if (hole && env.rreps) p.reps = std::max(1, env.rreps);
  // TransE, large batches (the A role's owner-mark regime): the same spread,
  // one replica per ~256 expected adds into a row (bs / M), <= 16, folded by
  // k_rel_fold after every batch launch (WN18 nb = 2: 16; nb = 100: 1)
  if (p.grouped) {
    const long long per_row = bs / std::max(1, M);
    while (p.reps < 16 && (long long)p.reps * 256 < per_row) p.reps *= 2;
  }
  p.rfold = p.reps > 1;
  // 8-B words per relation row: sums + count, whole 128-B lines (HolE: d
  // floats, then the count as an int)
  p.rw = hole ? ((d + 2) / 2 + 15) / 16 * 16 : ((p.w32 ? 2 * nq : nq) + 1 + 15) / 16 * 16;
  p.lds = !hole ? 0 : p.pair ? env.lds_fft_wave : p.fft ? env.lds_fft_wg : env.lds_direct_wg;
  p.wpb = p.pair ? 2 : (p.grouped ? PIPE_WG_GRP : SKGE_PIPE_WG) / 64;

  PipeBytes& b = p.bytes;
  b.ent_rows = (size_t)N * d * 4;
  b.ent_sum = (size_t)N * nq * (hole ? 16 : (p.e8 ? 4 : 8));
  b.ent_word = (size_t)N * 4;
  b.ent_meta = (size_t)N * 16;
  b.slots = (size_t)4 * bs * 4;
  b.rel_rows = (size_t)M * d * 4;
  b.rel_acc = (size_t)p.reps * M * p.rw * 8;
  b.rec = (size_t)T * 16;
  b.rec_n1 = (size_t)T * 4;
  b.err = 4;
  b.key_copy = p.dp ? 0 : 8;
  b.stats = (size_t)(p.nb1 + 3) * 3 * env.shard_words * 4;
  b.viol = (size_t)env.shard_words * 4;
  b.hot_sum = (size_t)HOT_REPS * p.hw * 8;
  b.hot_cnt = (size_t)HOT_REPS * 4;
  b.hot_val = (size_t)d * 4;
  b.hot_row = 4;
  pipe_plan_launches(p, 0);
  return p;
}

}  // namespace skge
