"""Cost of the self-adversarial loss in the device loop, beside the margin loss.

WN18-shaped KG (40943 entities, 18 relations, 141442 random triples), d = 200,
AdaGrad, nb = 100, K = 2 n negatives per positive over modes [0, 1], K in
{2, 10, 20}.  Legs, interleaved in one process, every leg a fresh runner from
the same initial tables:

  * sadv_l1    the self-adversarial loss on TransE-L1 (SadvLoopRunner, k_sadv_pos);
  * sadv_rot   the same on RotatE;
  * margin_l1  TransE-L1's margin loss on k_transe_pos_multi (SKGE_TRANSE_PAIRS=0)
               with a margin so large that every pair violates: 3 + K row adds
               per positive, as the new loss makes (it reads 3 + 2K rows, the
               margin kernel 3 + K).  At K = 2 the pair loop runs (1, [0, 1]) on
               explicit pairs whatever the switch says: that line is labelled
               form = "pairs" and no ratio is formed from it;
  * per_batch  SelfAdversarialTrainer's per-batch path with the host sampler
               (two epochs, each wall-clocked).

Every device timing is HIP events around `rounds` single epochs after `warm`
warm-up epochs; a line holds the median of the turns' medians and the range of
all samples.  Writes one JSON line per (leg, K) to profiles/sadv/<tag>.jsonl
and prints them, then the sadv_l1 / margin_l1 ratio at K = 10 and 20.

  python tools/bench_sadv.py [--tag NAME] [--turns 3] [--rounds 7] [--no-per-batch]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scikit-kge_amd"))

N, M, T, D, NB = 40943, 18, 141442, 200, 100
BIG_MARGIN = 1e6   # every pair violates


def make_kg(seed=0):
    rs = np.random.RandomState(seed)
    t = np.stack([rs.randint(N, size=2 * T), rs.randint(N, size=2 * T), rs.randint(M, size=2 * T)], 1)
    t = np.unique(t, axis=0)
    rs.shuffle(t)
    return [tuple(int(v) for v in x) for x in t[:T]]


def model_of(S, leg):
    np.random.seed(42)
    m = S.RotatE((N, N, M), D) if leg == "sadv_rot" else S.TransE((N, N, M), D, l1=True)
    m.add_hyperparam("margin", BIG_MARGIN)
    m.add_hyperparam("gamma", 6.0)
    m.add_hyperparam("alpha", 1.0)
    return m


def time_device(S, DV, leg, kg, n, warm, rounds):
    os.environ["SKGE_TRANSE_PAIRS"] = "0"   # read at create: the per-positive kernel
    m = model_of(S, leg)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    cls = DV.PairLoopRunner if leg == "margin_l1" else DV.SadvLoopRunner
    r = cls(m, upd, kg, NB, seed=1, negatives=(n, [0, 1], None))
    ms = []
    with torch.cuda.stream(r.stream):
        r.run(warm)
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(r.stream)
            r.run(1)
            b.record(r.stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
    r.synchronize()
    return ms


def time_per_batch(S, xs, n, epochs=2):
    m = model_of(S, "sadv_l1")
    np.random.seed(1)
    marks = []

    def mark(t):
        torch.cuda.synchronize()
        marks.append(time.perf_counter())
        return True
    tr = S.SelfAdversarialTrainer(m, gamma=6.0, alpha=1.0, nbatches=NB, max_epochs=epochs,
                                  learning_rate=0.1,
                                  samplef=S.RandomModeSampler(n, [0, 1], xs, (N, N, M)).sample,
                                  post_epoch=[mark])
    torch.cuda.synchronize()
    marks.append(time.perf_counter())
    tr.fit(xs, [1] * len(xs))
    return [(b - a) * 1e3 for a, b in zip(marks, marks[1:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-per-batch", action="store_true")
    a = ap.parse_args()
    import skge_amd as S
    import skge_amd.device as DV
    xs = make_kg()
    kg = DV.DeviceKG(xs, torch.device("cuda", 0))
    cases = [(leg, n) for n in (1, 5, 10) for leg in ("sadv_l1", "margin_l1", "sadv_rot")]
    got, meds = {}, {}
    for turn in range(a.turns):            # every leg and K once per turn
        for leg, n in cases:
            ms = time_device(S, DV, leg, kg, n, a.warm, a.rounds)
            got.setdefault((leg, n), []).extend(ms)
            meds.setdefault((leg, n), []).append(float(np.median(ms)))
    if not a.no_per_batch:
        for n in (1, 5, 10):
            got[("per_batch", n)] = time_per_batch(S, xs, n)
    out = os.path.join(ROOT, "profiles", "sadv")
    os.makedirs(out, exist_ok=True)
    med_of = {}
    with open(os.path.join(out, a.tag + ".jsonl"), "w") as f:
        for (leg, n), ms in got.items():
            med = float(np.median(meds.get((leg, n), ms)))
            med_of[(leg, n)] = med
            form = ("per_batch" if leg == "per_batch" else
                    "pairs" if leg == "margin_l1" and n == 1 else "per_positive")
            line = {"leg": leg, "form": form, "n": n, "K": 2 * n, "d": D, "nb": NB, "T": T,
                    "ms_per_epoch": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                    "samples": len(ms), "turn_medians_ms": meds.get((leg, n)),
                    "positives_per_s": T / med * 1e3,
                    "device": torch.cuda.get_device_properties(0).gcnArchName}
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))
        for n in (5, 10):
            line = {"ratio": "sadv_l1 / margin_l1", "K": 2 * n,
                    "value": med_of[("sadv_l1", n)] / med_of[("margin_l1", n)]}
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))


if __name__ == "__main__":
    main()
