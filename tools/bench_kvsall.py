#!/usr/bin/env python3
"""KvsAll step time on the WN18-shaped KG (|E| = 40943, 18 relations, d = 200):
skge_kvsall_step (AdaGrad) for DistMult and ComplEx at B = 128, 512, 1024
queries per batch, beside two yardsticks timed in the same process:

  (a) skge_neighbours at nq = B, k = 10, dot metric: the library's own fp32
      MFMA contraction of the forward's shape (the forward adds a
      transcendental epilogue and a B x N store);
  (b) the same step written with torch fp32 matmuls (dense labels by
      index_put, sigmoid, three matmuls, index_add chain rule, AdaGrad and
      normless1 on every E row).

One process; every round runs each leg once over the same NB batches (device
events around the leg); rounds 1-2 are warm-up, the medians of rounds 3-9 are
reported.  A step is three products of 2 B N d flops each; TF/s are set against
the 157.3 TF fp32 matrix peak.  G is B N floats, written once and read twice.
--kernels 1 runs one leg's batches once more for a kernel trace taken from
outside (rocprofv3 --kernel-trace --stats -- python tools/bench_kvsall.py
--kernels 1 --legs distmult:512); profiles/kvsall/README.md holds the record.

Usage: python tools/bench_kvsall.py [--out profiles/kvsall/bench_kvsall.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scikit-kge_amd")]

PEAK_TF = 157.3
NB = 8   # batches per leg and round


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--skip", type=int, default=2)
    ap.add_argument("--legs", default="distmult:128,distmult:512,distmult:1024,"
                                      "complex:128,complex:512,complex:1024")
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kvsall", "bench_kvsall.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import skge_amd as S
    from skge_amd import _lib as L
    from bench import make_wn18_kg, N_ENT, N_REL
    L.require_gpu()
    lib = L.lib()
    dev = torch.device("cuda:0")
    d, N = 200, N_ENT
    q_all = S.KvsAllQueries.from_triples(make_wn18_kg(), (N_ENT, N_ENT, N_REL)).to(dev)
    rng = np.random.RandomState(0)
    order = rng.permutation(len(q_all))
    legs = {}

    def kv_leg(name, B):
        np.random.seed(42)
        m = (S.DistMult if name == "distmult" else S.ComplEx)((N_ENT, N_ENT, N_REL), d)
        upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
        batches = [q_all.batch(order[i * B:(i + 1) * B]) for i in range(NB)]
        loss = torch.zeros(1, dtype=torch.float32, device=dev)

        def run():
            for b in batches:
                m._kvsall_step(b, upd, loss)
        return run, (m, upd, batches, loss)

    def nb_leg(B):
        np.random.seed(42)
        m = S.DistMult((N_ENT, N_ENT, N_REL), d)
        E = m.params["E"]
        rows = torch.as_tensor(order[:B].astype(np.int32) % N, device=dev)
        nbytes = lib.skge_neighbours_workspace_bytes(B, N, d, 10)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        io = torch.empty((B, 10), dtype=torch.int32, device=dev)
        so = torch.empty((B, 10), dtype=torch.float32, device=dev)

        def run():
            for _ in range(NB):
                L.check(lib.skge_neighbours(L.stream_ptr(), L.ptr(E.data), N, d, None, L.ptr(rows),
                                            B, 1, 10, L.ptr(ws), nbytes, L.ptr(io), L.ptr(so)),
                        "neighbours")
        return run, (m, rows, ws, io, so)

    def torch_leg(name, B):
        np.random.seed(42)
        m = (S.DistMult if name == "distmult" else S.ComplEx)((N_ENT, N_ENT, N_REL), d)
        E, R = m.E.data, m.R.data
        pE, pR = torch.zeros_like(E), torch.zeros_like(R)
        batches = []
        for i in range(NB):
            b = q_all.batch(order[i * B:(i + 1) * B])
            lens = (b.off[1:] - b.off[:-1]).long()
            rowid = torch.repeat_interleave(torch.arange(B, device=dev), lens)
            batches.append((b.anchor.long(), b.rel.long(), b.dir, rowid, b.ans.long()))

        def cmul(x, y, conj_x=False):
            xr, xi, yr, yi = x[:, 0::2], x[:, 1::2], y[:, 0::2], y[:, 1::2]
            if conj_x:
                xi = -xi
            return torch.stack([xr * yr - xi * yi, xr * yi + xi * yr], dim=2).reshape(x.shape)

        def run():
            for a, p, t, rowid, ans in batches:
                ea, rp = E[a], R[p]
                tail = (t == 0)[:, None]
                if name == "distmult":
                    Q = ea * rp
                else:
                    Q = torch.where(tail, cmul(ea, rp), cmul(rp, ea, conj_x=True))
                z = Q @ E.t()
                y = torch.zeros_like(z)
                y[rowid, ans] = 1.0
                G = (torch.sigmoid(z) - y) / B
                gE = G.t() @ Q
                dq = G @ E
                if name == "distmult":
                    ga, gr = dq * rp, dq * ea
                else:
                    ga = torch.where(tail, cmul(rp, dq, conj_x=True), cmul(dq, rp))
                    gr = torch.where(tail, cmul(ea, dq, conj_x=True), cmul(dq, ea, conj_x=True))
                gE.index_add_(0, a, ga)
                gR = torch.zeros_like(R).index_add_(0, p, gr)
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
        for key, mk in (("kvsall %s B%d" % (name, B), lambda: kv_leg(name, B)),
                        ("torch %s B%d" % (name, B), lambda: torch_leg(name, B)),
                        ("neighbours B%d" % B, lambda: nb_leg(B))):
            if key not in legs:
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
        nprod = 1 if key.startswith("neighbours") else 3
        tf = nprod * 2.0 * B * N * d / (med * 1e-3) / 1e12
        rec = {"leg": key, "B": B, "N": N, "d": d, "ms_per_batch": round(med, 4),
               "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4),
               "queries_per_s": round(B / (med * 1e-3)), "products": nprod,
               "tflops": round(tf, 2), "of_fp32_peak": round(tf / PEAK_TF, 4),
               "rounds": "%d-%d" % (args.skip + 1, args.rounds),
               "device": torch.cuda.get_device_name(0)}
        if key.startswith("kvsall"):
            rec["G_bytes"] = 4 * B * ((N + 3) // 4 * 4)
            rec["G_traffic_GBps_if_all_time"] = round(3 * rec["G_bytes"] / (med * 1e-3) / 1e9, 1)
        lines.append(rec)
    by = {r["leg"]: r for r in lines}
    for r in lines:
        if r["leg"].startswith("kvsall"):
            name = r["leg"].split()[1]
            r["torch_ms_over_this"] = round(by["torch %s B%d" % (name, r["B"])]["ms_per_batch"] /
                                            r["ms_per_batch"], 3)
            r["step_tflops_over_neighbours_tflops"] = round(
                r["tflops"] / by["neighbours B%d" % r["B"]]["tflops"], 3)
    text = "\n".join(json.dumps(r) for r in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
