#!/usr/bin/env python3
"""What the RotatE device pair loop costs, and whether the per-positive kernel
(k_rot_pos) beats the explicit pairs, on the WN18-shaped KG of bench.py
(make_wn18_kg: N = 40943, M = 18, T = 141442), d = 200, AdaGrad, nb = 100.

One process, interleaved legs (round r times every leg once, in order, before
round r + 1 starts, so drift hits all legs alike): epochs 1-2 warm up, epochs
3-9 are timed with HIP events around one graph replay each, median reported
with the raw times.

  rotate, form "pos"      the pair loop with k_rot_pos
  rotate, form "pairs"    the same with SKGE_ROT_PAIRS=1 (read when the runner
                          is created, so both forms live in one process)
  complex, transe_l1      the pair loop's own kernels for those models:
                          same-box yardsticks

One JSON line per leg, appended to --out when given.

Usage: python tools/bench_rotate.py [--rounds 7] [--warmup 2] [--d 200] [--nb 100]
           [--out profiles/rotate/runs.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--d", type=int, default=200)
    ap.add_argument("--nb", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "scikit-kge_amd"))
    sys.path.insert(0, ROOT)
    import torch
    import skge_amd as S
    from skge_amd.device import DeviceKG, PairLoopRunner
    from bench import N_ENT, N_REL, make_wn18_kg
    xs = make_wn18_kg()
    T = len(xs)
    sz = (N_ENT, N_ENT, N_REL)
    kg = DeviceKG(xs, torch.device("cuda", 0))
    base = {"d": args.d, "nb": args.nb, "updater": "adagrad",
            "kg": "wn18-shaped uniform (%d, %d, %d)" % (N_ENT, N_REL, T),
            "device": torch.cuda.get_device_name(0)}
    out = open(args.out, "a") if args.out else None

    def model(name):
        np.random.seed(42)
        if name == "transe_l1":
            m = S.TransE(sz, args.d, l1=True)
            m.add_hyperparam("margin", 2.0)
        elif name == "rotate":
            m = S.RotatE(sz, args.d)
            m.add_hyperparam("margin", 2.0)
        else:
            m = S.ComplEx(sz, args.d)
            m.add_hyperparam("margin", 0.2)
        return m, {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}

    legs = []
    for name, form in (("rotate", "pos"), ("rotate", "pairs"), ("complex", None),
                       ("transe_l1", None)):
        m, upd = model(name)
        if form is not None:
            os.environ["SKGE_ROT_PAIRS"] = "1" if form == "pairs" else "0"
        r = PairLoopRunner(m, upd, kg, args.nb, seed=1234)
        os.environ.pop("SKGE_ROT_PAIRS", None)
        legs.append((name, form, r, m, upd, []))   # (upd: the graph writes its state)
    for _, _, r, _, _, _ in legs:
        with torch.cuda.stream(r.stream):
            r.run(args.warmup)
        r.synchronize()
    for _ in range(args.rounds):
        for _, _, r, _, _, ms in legs:
            with torch.cuda.stream(r.stream):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record(r.stream)
                r.run(1)
                e1.record(r.stream)
                r.synchronize()
            ms.append(e0.elapsed_time(e1))
    bad = 0
    for name, form, r, m, _, ms in legs:
        nonfinite = {pid: int((~torch.isfinite(p.data)).sum().item()) for pid, p in m.params.items()}
        bad += sum(nonfinite.values())
        med = float(np.median(ms))
        s = json.dumps(dict(base, what="epoch", runner="pair", model=name, form=form,
                            ms_median=round(med, 4), ms=[round(v, 4) for v in ms],
                            graph_nodes=r.nlaunches, warmup=args.warmup,
                            triples_per_s=round(T / (med * 1e-3), 1), nonfinite=nonfinite,
                            violations=int(r.nviol_total.item())))
        print(s, flush=True)
        if out:
            out.write(s + "\n")
    if out:
        out.close()
    if bad:
        raise SystemExit("non-finite parameters after the timed epochs (see the lines)")


if __name__ == "__main__":
    main()
