"""Throughput of the logistic trainer (StochasticTrainer: HolE under
--no-pairwise, RESCAL) on the WN18-shaped KG of bench.py (make_wn18_kg), d =
200, AdaGrad, nb = 100.

Default: whole epochs of the device logistic loop (LogisticLoopRunner), timed
with events on the runner's stream after warm-up epochs; the HolE form is the
runner's own choice (SKGE_HOLE_TRIPLES=1 in the environment selects the
explicit triples).  --per-batch: the per-batch path instead --
StochasticTrainer.fit with the host RandomModeSampler, one epoch, wall clock
(its host work is the cost being measured).

Prints one JSON line per model: positives (training triples) per second and
ms per epoch.

Usage: python tools/bench_logistic.py [--per-batch] [--epochs 5] [--warmup 2]
                                      [--models hole,rescal] [--nb 100] [--d 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scikit-kge_amd"))
sys.path.insert(0, ROOT)


def _model(S, kind, sz, d):
    np.random.seed(42)
    return S.HolE(sz, d) if kind == "hole" else S.RESCAL(sz, d)


def run_runner(S, torch, kind, xs, sz, d, nb, warmup, epochs):
    from skge_amd.device import DeviceKG, LogisticLoopRunner
    m = _model(S, kind, sz, d)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    kg = DeviceKG(xs, m.device)
    r = LogisticLoopRunner(m, upd, kg, nb, seed=1234)
    with torch.cuda.stream(r.stream):
        r.run(warmup)
        r.synchronize()
        ms = []
        for _ in range(epochs):   # one event pair per epoch: the spread is on record
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(r.stream)
            r.run(1)
            e1.record(r.stream)
            r.synchronize()
            ms.append(e0.elapsed_time(e1))
    loss = float(r.loss_total.item())
    assert np.isfinite(loss) and np.isfinite(m.E.data.sum().item())
    med = float(np.median(ms))
    return {"path": "runner", "hole_triples_env": os.environ.get("SKGE_HOLE_TRIPLES", ""),
            "ms_per_epoch": round(med, 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4), "epochs": epochs, "warmup": warmup,
            "graph_nodes": r.nlaunches, "triples_per_s": round(len(xs) / (med * 1e-3), 1)}


def run_per_batch(S, torch, kind, xs, sz, d, nb):
    m = _model(S, kind, sz, d)
    txs = [tuple(int(v) for v in x) for x in xs]
    np.random.seed(7)
    tr = S.StochasticTrainer(m, max_epochs=1, nbatches=nb, learning_rate=0.1,
                             samplef=S.RandomModeSampler(1, [0, 1], txs, sz).sample)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.fit(txs, [1] * len(txs))
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    assert np.isfinite(tr.loss)
    return {"path": "per_batch", "ms_per_epoch": round(sec * 1e3, 2), "epochs": 1, "warmup": 0,
            "triples_per_s": round(len(xs) / sec, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-batch", action="store_true")
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--models", default="hole,rescal")
    ap.add_argument("--nb", type=int, default=100)
    ap.add_argument("--d", type=int, default=200)
    args = ap.parse_args()
    import torch
    import skge_amd as S
    from bench import N_ENT, N_REL, make_wn18_kg
    xs = make_wn18_kg()
    sz = (N_ENT, N_ENT, N_REL)
    for kind in args.models.split(","):
        if args.per_batch:
            line = run_per_batch(S, torch, kind, xs, sz, args.d, args.nb)
        else:
            line = run_runner(S, torch, kind, xs, sz, args.d, args.nb, args.warmup, args.epochs)
        line.update({"model": kind, "d": args.d, "nb": args.nb, "opt": "adagrad",
                     "kg": "wn18-shaped uniform (%d, %d, %d)" % (N_ENT, N_REL, len(xs)),
                     "device": torch.cuda.get_device_name(0)})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
