#!/usr/bin/env python3
"""Link-prediction evaluation time: skge_score and skge_curve_stats with their
yardsticks timed in the same process, interleaved, medians and spread.

  scores   n labelled triples on the WN18-shaped KG (N = 40943, d = 200), TransE,
           HolE (M = 18) and RESCAL (M = 18 and M = 1345, W = 215 MB): skge_score
           against skge_pair_grad with the positives as negatives (the only
           route before; for RESCAL a one-wave-per-triple kernel), both on device
           triples; and Model.score against Model._scores from the same host
           array (upload and id check included).
           TransE / HolE: GB/s of gathered rows (3 rows of 4 d bytes per triple).
           RESCAL: TFLOP/s = 2 n d (d + 1) / time against the 157.3 TF fp32 peak.
  curves   skge_curve_stats (one segment, and M segments) against torch.sort +
           cumsum on the same GPU and against sklearn on the host.

Device events around each call, warm-up first, the calls interleaved over the
rounds.  Usage: python tools/bench_linkpred.py [--n 100000 10000000]
[--rounds 7] [--out profiles/linkpred/bench_linkpred.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scikit-kge_amd")]

PEAK_TF = 157.3
N_ENT, D = 40943, 200


def timed(calls, rounds, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {key: [] for key in calls}
    for _ in range(rounds):          # interleaved: one of each per round
        for key, fn in calls.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ms[key].append(t0.elapsed_time(t1))
    return {key: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4),
                  "max_ms": round(max(v), 4)} for key, v in ms.items()}


def bench_scores(n, rounds, out):
    import numpy as np
    import torch
    import skge_amd as S
    rs = np.random.RandomState(1)
    for name, cls, M in (("transe", S.TransE, 18), ("hole", S.HolE, 18), ("rescal", S.RESCAL, 18),
                         ("rescal", S.RESCAL, 1345)):
        np.random.seed(3)
        m = cls((N_ENT, N_ENT, M), D)
        trip = np.stack([rs.randint(0, N_ENT, n), rs.randint(0, N_ENT, n), rs.randint(0, M, n)],
                        axis=1).astype(np.int32)
        tt = torch.as_tensor(trip, device=m.device)
        # _scores takes host columns (its upload is part of that route)
        ss, oo, pp = (np.ascontiguousarray(trip[:, j]) for j in range(3))
        # the entry point itself, buffers allocated once (Model.score adds the
        # host's id check and the allocations)
        from skge_amd import _lib as L
        lib = L.lib()
        rel = m.params[m.rel_id]
        nb = int(lib.skge_score_workspace_bytes(m._kernel_model(), n, M, D))
        ws = torch.empty(nb, dtype=torch.uint8, device=m.device)
        sc = torch.empty(n, dtype=torch.float32, device=m.device)

        def raw(m=m, rel=rel, ws=ws, sc=sc, nb=nb, tt=tt, M=M):
            L.check(lib.skge_score(L.stream_ptr(), m._kernel_model(), L.ptr(m.params["E"].data),
                                   L.ptr(rel.data), N_ENT, M, D, L.ptr(tt), n, L.ptr(ws), nb,
                                   L.ptr(sc)), "score")
        # the route before, two ways: its kernel alone (skge_pair_grad with the
        # positives as negatives, the triples already on the device, as for
        # skge_score; it scores every triple twice and builds the table structs per
        # call, which is that route), and Model._scores as a user calls it, from host
        # columns -- beside Model.score from the same host array
        out_old = torch.empty(n, dtype=torch.float32, device=m.device)

        def old_kernel(m=m, tt=tt, out_old=out_old):
            te, tr = m._tables("pairwise")
            L.check(lib.skge_pair_grad(L.stream_ptr(), m._kernel_model(), m._af_code(), te, tr, D,
                                       L.ptr(tt), L.ptr(tt), n, float("-inf"), L.ptr(out_old),
                                       None, None, None), "scores")
        calls = {"skge_score": raw, "pair_grad_device": old_kernel,
                 "Model.score_host": lambda: m.score(trip),
                 "Model._scores_host": lambda: m._scores(ss, pp, oo)}
        r = timed(calls, rounds, 2)
        t = r["skge_score"]["median_ms"] * 1e-3
        rec = {"what": "score", "model": name, "M": M, "n": n, "d": D, **r}
        if name == "rescal":
            tf = 2.0 * n * D * (D + 1) / t / 1e12
            rec.update({"tflops": round(tf, 2), "fraction_of_fp32_peak": round(tf / PEAK_TF, 4)})
        else:
            rec["gather_GBps"] = round(3.0 * 4 * D * n / t / 1e9, 1)
        print(json.dumps(rec))
        out.append(rec)
        del m
        torch.cuda.empty_cache()


def bench_curves(n, rounds, out):
    import numpy as np
    import torch
    from skge_amd import linkpred as LP
    rs = np.random.RandomState(2)
    y = (rs.rand(n) < 0.5).astype(np.int8)
    s = (rs.randn(n) + y).astype(np.float32)
    st, yt = torch.as_tensor(s, device="cuda:0"), torch.as_tensor(y, device="cuda:0")

    def torch_route():
        srt, idx = torch.sort(st, descending=True)
        lab = yt[idx].to(torch.int64)
        tp = torch.cumsum(lab, 0)
        fp = torch.cumsum(1 - lab, 0)
        return tp, fp
    for nseg in (1, 18, 1345):
        seg = None if nseg == 1 else torch.as_tensor(rs.randint(0, nseg, n).astype(np.int32),
                                                     device="cuda:0")
        calls = {"skge_curve_stats": lambda: LP.curve_stats(st, yt, seg=seg, nseg=nseg)}
        if nseg == 1:
            calls["torch_sort_cumsum"] = torch_route
        rec = {"what": "curve", "n": n, "nseg": nseg, **timed(calls, rounds, 2)}
        if nseg == 1:
            from sklearn.metrics import auc, precision_recall_curve, roc_auc_score
            t0 = time.perf_counter()
            p, r, _ = precision_recall_curve(y, s)
            auc(r, p)
            roc_auc_score(y, s)
            rec["sklearn_host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        print(json.dumps(rec))
        out.append(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 10000000])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linkpred",
                                                  "bench_linkpred.json"))
    args = ap.parse_args()
    out = []
    for n in args.n:
        bench_scores(n, args.rounds, out)
        bench_curves(n, args.rounds, out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
