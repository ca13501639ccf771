// The pipelined runner's plan header on its own: csrc/skge_pipe_plan.h
// compiled by the host compiler (no HIP header, no device) and run over the
// geometries of tests/test_pipe_plan.py under the sanitizers.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/pipe_plan_check.cpp -o pipe_plan_check && ./pipe_plan_check
// Prints one line per geometry; exits non-zero if a launch's figures leave
// their ranges or the bytes of a smaller hot-row count exceed the bound.
#include <cstdio>

#include "../scikit-kge_amd/csrc/skge_pipe_plan.h"

using namespace skge;

static skge_table_t table(int rows, int width, int mode, int slots) {
  skge_table_t t = {};
  t.rows = rows;
  t.width = width;
  t.acc_mode = mode;
  t.touched_cap = slots;
  t.opt = SKGE_ADAGRAD;
  t.state = (float*)&t;   // "has AdaGrad state": tested for NULL only
  return t;
}

static int check(const char* name, int d, long long T, int nb, int emode, int rmode, int M,
                 int flags, bool hole, PipeEnv env) {
  const int bs = (int)(T / nb);
  skge_table_t ent = table(300, d, emode, 4 * bs), rel = table(M, d, rmode, 0);
  env.shard_words = 64 * 32;
  env.lds_fft_wave = (size_t)(2 * d + 10 * d) * 4;
  env.lds_fft_wg = (size_t)(2 * d + 4 * 10 * d) * 4;
  env.lds_direct_wg = (size_t)4 * (10 * d + 28) * 4;
  PipePlan p = pipe_plan(&ent, &rel, d, T, nb, flags, hole, env);
  int bad = 0;
  for (int nhot : {0, 1, HOT_MAX}) {
    if (nhot && !p.hot) continue;
    pipe_plan_launches(p, nhot);
    long long covered = 0;
    for (const PipeLaunch& L : p.launch) {
      bad += L.grid < 1 || L.count < 0 || L.start != (L.count ? covered : 0);
      bad += !p.fused && (L.nA < 1 || L.grid != L.nA + p.score_groups(L.count));
      covered += L.count;
    }
    bad += covered != T || (int)p.launch.size() != p.nb1 + 1 || p.launch.back().count != 0;
    bad += p.total(nhot) > p.device_bytes();
  }
  printf("%-22s kernel %d grouped %d e8 %d w32 %d fft %d pair %d kq %d reps %d launches %d "
         "bytes %zu%s\n", name, p.kernel(), p.grouped, p.e8, p.w32, p.fft, p.pair, p.kq, p.reps,
         p.nlaunch(), p.device_bytes(), bad ? "  BAD" : "");
  return bad;
}

int main() {
  const int I16 = SKGE_ACC_I16X4, I8 = SKGE_ACC_I8X4, I32 = SKGE_ACC_I32X2, F32 = SKGE_ACC_F32;
  PipeEnv e, off, on, fft;
  off.fused = 0;
  on.fused = 1;
  fft.hole_fft = true;
  int bad = 0;
  bad += check("fused", 64, 1000, 3, I16, I16, 5, 0, false, e);
  bad += check("fused-off", 64, 1000, 3, I16, I16, 5, 0, false, off);
  bad += check("batch-kq1", 200, 1000, 3, I16, I16, 5, 0, false, e);
  bad += check("batch-kq2", 260, 1000, 3, I16, I16, 5, 0, false, e);
  bad += check("batch-kq4", 1024, 1000, 3, I16, I16, 5, 0, false, e);
  bad += check("w32", 200, 1000, 3, I16, I32, 5, 0, false, e);
  bad += check("e8", 200, 1000, 3, I8, I16, 5, 0, false, e);
  bad += check("grouped-reps", 200, 9000, 2, I16, I16, 5, 0, false, e);
  bad += check("dp", 200, 1000, 3, I16, I16, 5, SKGE_PIPE_DP, false, e);
  bad += check("dp-d64", 64, 1000, 3, I16, I16, 5, SKGE_PIPE_DP, false, on);
  bad += check("fused-forced", 200, 1000, 3, I16, I16, 5, 0, false, on);
  bad += check("one-triple", 4, 1, 1, I16, I16, 1, 0, false, e);
  bad += check("hole-pair", 200, 1000, 3, F32, F32, 5, 0, true, fft);
  bad += check("hole-no-pair", 200, 3000, 1, F32, F32, 5, 0, true, fft);
  bad += check("hole-large", 200, 141442, 2, F32, F32, 18, 0, true, fft);
  bad += check("hole-direct", 8, 1000, 3, F32, F32, 5, 0, true, e);
  return bad ? 1 : 0;
}
