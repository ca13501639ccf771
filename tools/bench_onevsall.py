#!/usr/bin/env python3
"""1vsAll step time on the WN18-shaped KG (|E| = 40943, 18 relations, d = 200):
skge_onevsall_step (AdaGrad, label smoothing 0.1, n3 = 0.05) for DistMult and
ComplEx at B = 128, 512, 1024 queries per batch, beside two yardsticks timed in
the same process:

  (a) skge_kvsall_step at the same B: the same three products with the
      element-wise BCE epilogue, no row reduction and no second pass over G;
  (b) the same 1vsAll step written with torch fp32 matmuls (logsumexp, the
      softmax gradient, three matmuls, index_add chain rule and N3, AdaGrad
      and normless1 on every E row).

One process; every round runs each leg once over the same NB batches (device
events around the leg); rounds 1-2 are warm-up, the medians of rounds 3-9 are
reported.  A step is three products of 2 B N d flops each; TF/s are set against
the 157.3 TF fp32 matrix peak.  G is B N floats: written by the forward, read
and rewritten by the combine, read by both backward products.
--kernels 1 runs every leg's batches twice for a kernel trace taken from
outside (rocprofv3 --kernel-trace --stats -- python tools/bench_onevsall.py
--kernels 1 --legs distmult:512); profiles/onevsall/README.md holds the record.

Usage: python tools/bench_onevsall.py [--out profiles/onevsall/bench_onevsall.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scikit-kge_amd")]

PEAK_TF = 157.3
NB = 8   # batches per leg and round
EPS, N3 = 0.1, 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--skip", type=int, default=2)
    ap.add_argument("--legs", default="distmult:128,distmult:512,distmult:1024,"
                                      "complex:128,complex:512,complex:1024")
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "onevsall",
                                                  "bench_onevsall.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import skge_amd as S
    from skge_amd import _lib as L
    from bench import make_wn18_kg, N_ENT, N_REL
    L.require_gpu()
    dev = torch.device("cuda:0")
    d, N = 200, N_ENT
    sz = (N_ENT, N_ENT, N_REL)
    kg = make_wn18_kg()
    q_ova = S.OneVsAllQueries.from_triples(kg, sz).to(dev)
    q_kv = S.KvsAllQueries.from_triples(kg, sz).to(dev)
    rng = np.random.RandomState(0)
    order_ova = rng.permutation(len(q_ova))
    order_kv = rng.permutation(len(q_kv))
    legs = {}

    def model(name):
        np.random.seed(42)
        return (S.DistMult if name == "distmult" else S.ComplEx)(sz, d)

    def ova_leg(name, B):
        m = model(name)
        m.add_hyperparam("label_smoothing", EPS)
        m.add_hyperparam("n3", N3)
        upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
        batches = [q_ova.batch(order_ova[i * B:(i + 1) * B]) for i in range(NB)]
        loss = torch.zeros(1, dtype=torch.float32, device=dev)

        def run():
            for b in batches:
                m._onevsall_step(b, upd, loss)
        return run, (m, upd, batches, loss)

    def kv_leg(name, B):
        m = model(name)
        m.add_hyperparam("label_smoothing", EPS)
        upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
        batches = [q_kv.batch(order_kv[i * B:(i + 1) * B]) for i in range(NB)]
        loss = torch.zeros(1, dtype=torch.float32, device=dev)

        def run():
            for b in batches:
                m._kvsall_step(b, upd, loss)
        return run, (m, upd, batches, loss)

    def torch_leg(name, B):
        m = model(name)
        E, R = m.E.data, m.R.data
        pE, pR = torch.zeros_like(E), torch.zeros_like(R)
        batches = []
        for i in range(NB):
            b = q_ova.batch(order_ova[i * B:(i + 1) * B])
            batches.append((b.anchor.long(), b.rel.long(), b.dir, b.target.long()))
        rows = torch.arange(B, device=dev)

        def cmul(x, y, conj_x=False):
            xr, xi, yr, yi = x[:, 0::2], x[:, 1::2], y[:, 0::2], y[:, 1::2]
            if conj_x:
                xi = -xi
            return torch.stack([xr * yr - xi * yi, xr * yi + xi * yr], dim=2).reshape(x.shape)

        def n3g(x):   # d |x|_3^3 / d x
            if name == "distmult":
                return 3.0 * x.abs() * x
            mod = (x[:, 0::2] ** 2 + x[:, 1::2] ** 2).sqrt()
            return 3.0 * mod.repeat_interleave(2, dim=1) * x

        def run():
            for a, p, t, g in batches:
                ea, rp, eg = E[a], R[p], E[g]
                tail = (t == 0)[:, None]
                if name == "distmult":
                    Q = ea * rp
                else:
                    Q = torch.where(tail, cmul(ea, rp), cmul(rp, ea, conj_x=True))
                z = Q @ E.t()
                lse = torch.logsumexp(z, dim=1, keepdim=True)
                G = torch.exp(z - lse) - EPS / N
                G[rows, g] -= 1.0 - EPS
                G /= B
                gE = G.t() @ Q
                dq = G @ E
                if name == "distmult":
                    ga, gr = dq * rp, dq * ea
                else:
                    ga = torch.where(tail, cmul(rp, dq, conj_x=True), cmul(dq, rp))
                    gr = torch.where(tail, cmul(ea, dq, conj_x=True), cmul(dq, ea, conj_x=True))
                c = N3 / B
                gE.index_add_(0, a, ga + c * n3g(ea))
                gE.index_add_(0, g, c * n3g(eg))
                gR = torch.zeros_like(R).index_add_(0, p, gr + c * n3g(rp))
                pE.add_(gE * gE)
                E.sub_(0.1 * gE / pE.sqrt().clamp_min(1e-7))
                ss = (E * E).sum(dim=1, keepdim=True)
                E.div_(torch.where(ss < 1, torch.ones_like(ss), ss))
                pR.add_(gR * gR)
                R.sub_(0.1 * gR / pR.sqrt().clamp_min(1e-7))
        return run, (m, batches)

    keep = []
    for leg in args.legs.split(","):
        name, B = leg.split(":")
        B = int(B)
        for key, mk in (("onevsall %s B%d" % (name, B), lambda: ova_leg(name, B)),
                        ("kvsall %s B%d" % (name, B), lambda: kv_leg(name, B)),
                        ("torch %s B%d" % (name, B), lambda: torch_leg(name, B))):
            run, k = mk()
            legs[key] = (run, B)
            keep.append(k)
    if args.kernels:   # two passes of every leg, for a trace taken from outside
        for _ in range(2):
            for run, _B in legs.values():
                run()
                torch.cuda.synchronize()
        return
    ms = {key: [] for key in legs}
    for r in range(args.rounds):
        for key, (run, B) in legs.items():   # interleaved: one of each per round
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            run()
            t1.record()
            t1.synchronize()
            ms[key].append(t0.elapsed_time(t1) / NB)
    lines = []
    for key, (run, B) in legs.items():
        v = ms[key][args.skip:]
        med = float(np.median(v))
        tf = 3 * 2.0 * B * N * d / (med * 1e-3) / 1e12
        lines.append({"leg": key, "B": B, "N": N, "d": d, "ms_per_batch": round(med, 4),
                      "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4),
                      "queries_per_s": round(B / (med * 1e-3)), "tflops": round(tf, 2),
                      "of_fp32_peak": round(tf / PEAK_TF, 4),
                      "rounds": "%d-%d" % (args.skip + 1, args.rounds),
                      "device": torch.cuda.get_device_name(0)})
    by = {r["leg"]: r for r in lines}
    for r in lines:
        if r["leg"].startswith("onevsall"):
            name = r["leg"].split()[1]
            r["label_smoothing"], r["n3"] = EPS, N3
            r["this_ms_over_kvsall_ms"] = round(
                r["ms_per_batch"] / by["kvsall %s B%d" % (name, r["B"])]["ms_per_batch"], 3)
            r["torch_ms_over_this"] = round(
                by["torch %s B%d" % (name, r["B"])]["ms_per_batch"] / r["ms_per_batch"], 3)
    text = "\n".join(json.dumps(r) for r in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
