"""Cost of n negatives per positive in the device pair loop.

WN18-shaped KG (40943 entities, 18 relations, 141442 random triples), d = 200,
AdaGrad, nb = 100, K = 2 n negatives per positive over modes [0, 1].  Forms:

  * pairs      (a) the _multi pair loop on explicit pairs (SKGE_TRANSE_PAIRS=1):
               TransE-L1 at K = 2, 10, 20, HolE at K = 10 (its only form);
  * pos        (b) TransE's per-positive kernel k_transe_pos_multi
               (SKGE_TRANSE_PAIRS=0) at the same K;
  * per_batch  (c) the per-batch path with the host sampler (two epochs, each
               timed), the baseline the device loop replaces, at K = 2, 10, 20.

The device forms alternate a b a b within every turn (a turn builds a fresh
runner per case and form from the same initial tables).  Every device timing
is HIP events around `rounds` single epochs after `warm` warm-up epochs; the
line holds the median of the turns' medians and the range of all samples.
Writes one JSON line per (model, K, form) to profiles/negatives/<tag>.jsonl
and prints them.

  python tools/bench_negatives.py [--tag NAME] [--turns 4] [--rounds 7] [--no-per-batch]
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


def make_kg(seed=0):
    rs = np.random.RandomState(seed)
    t = np.stack([rs.randint(N, size=2 * T), rs.randint(N, size=2 * T), rs.randint(M, size=2 * T)], 1)
    t = np.unique(t, axis=0)
    rs.shuffle(t)
    return [tuple(int(v) for v in x) for x in t[:T]]


def model_of(S, kind):
    np.random.seed(42)
    m = S.TransE((N, N, M), D, l1=True) if kind == "transe_l1" else S.HolE((N, N, M), D)
    m.add_hyperparam("margin", 2.0 if kind == "transe_l1" else 0.2)
    return m


def time_device(S, DV, kind, kg, n, warm, rounds, form):
    os.environ["SKGE_TRANSE_PAIRS"] = "1" if form == "pairs" else "0"   # read at create
    m = model_of(S, kind)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    r = DV.PairLoopRunner(m, upd, kg, NB, seed=1, negatives=(n, [0, 1], None))
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


def time_per_batch(S, kind, xs, n, epochs=2):
    m = model_of(S, kind)
    np.random.seed(1)
    marks = []

    def mark(t):
        torch.cuda.synchronize()
        marks.append(time.perf_counter())
        return True
    tr = S.PairwiseStochasticTrainer(m, nbatches=NB, max_epochs=epochs, learning_rate=0.1,
                                     margin=float(m.margin),
                                     samplef=S.RandomModeSampler(n, [0, 1], xs, (N, N, M)).sample,
                                     file_grad=None, file_embed=None, post_epoch=[mark])
    torch.cuda.synchronize()
    marks.append(time.perf_counter())
    tr.fit(xs, [1] * len(xs))
    return [(b - a) * 1e3 for a, b in zip(marks, marks[1:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="negatives")
    ap.add_argument("--turns", type=int, default=4)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-per-batch", action="store_true")
    a = ap.parse_args()
    import skge_amd as S
    import skge_amd.device as DV
    xs = make_kg()
    kg = DV.DeviceKG(xs, torch.device("cuda", 0))
    cases = [("transe_l1", 1, "pairs"), ("transe_l1", 1, "pos"), ("transe_l1", 5, "pairs"),
             ("transe_l1", 5, "pos"), ("transe_l1", 10, "pairs"), ("transe_l1", 10, "pos"),
             ("hole", 5, "pairs")]
    got, meds = {}, {}
    for turn in range(a.turns):            # a b a b: every case and form once per turn
        for kind, n, form in cases:
            ms = time_device(S, DV, kind, kg, n, a.warm, a.rounds, form)
            got.setdefault((kind, n, form), []).extend(ms)
            meds.setdefault((kind, n, form), []).append(float(np.median(ms)))
    if not a.no_per_batch:
        for kind, n in (("transe_l1", 1), ("transe_l1", 5), ("transe_l1", 10)):
            got[(kind, n, "per_batch")] = time_per_batch(S, kind, xs, n)
    out = os.path.join(ROOT, "profiles", "negatives")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, a.tag + ".jsonl"), "w") as f:
        for (kind, n, form), ms in got.items():
            med = float(np.median(meds.get((kind, n, form), ms)))
            line = {"model": kind, "n": n, "K": 2 * n, "form": form, "d": D, "nb": NB, "T": T,
                    "ms_per_epoch": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                    "samples": len(ms),
                    "turn_medians_ms": meds.get((kind, n, form)), "positives_per_s": T / med * 1e3,
                    "pairs_per_s": 2 * n * T / med * 1e3,
                    "device": torch.cuda.get_device_properties(0).gcnArchName}
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))


if __name__ == "__main__":
    main()
