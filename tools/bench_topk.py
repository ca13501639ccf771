#!/usr/bin/env python3
"""Top-k link prediction time at the WN18 geometry (5000 queries, |E| = 40943,
|R| = 18, d = 200): skge_topk for tails and heads at k = 10 and k = 100, with
skge_rank_known (both directions of the same 5000 triples in one call) timed
in the same process for scale.

Device events around each call, warm-up first, the five timed calls
interleaved over the repeats, medians reported; host-side set-up (the
exclusion lists, the known-answer CSR, the buffers) is outside the timed
window.  Usage: python tools/bench_topk.py [--models transe,hole]
[--repeats 20] [--out profiles/topk/bench_topk.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scikit-kge_amd")]

KS = (10, 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="transe,hole")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk", "bench_topk.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import skge_amd as S
    from skge_amd import _lib as L
    from skge_amd.eval import _model_code
    from bench import make_wn18_kg, N_ENT, N_REL
    L.require_gpu()
    trip = make_wn18_kg()
    test = trip[:5000]
    lib = L.lib()
    out = {"queries": len(test), "n_ent": N_ENT, "n_rel": N_REL, "d": 200,
           "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "models": {}}
    for name in args.models.split(","):
        np.random.seed(42)
        m = {"transe": S.TransE, "hole": S.HolE, "rescal": S.RESCAL}[name]((N_ENT, N_ENT, N_REL), 200)
        code, rel = _model_code(m)
        E, dev, d = m.params["E"], m.device, m.d
        lp = S.LinkPredictor(m, trip)
        ev = S.FilteredRankingEval(test, trip)
        order = np.asarray([(s, o, p) for p, sos in ev.idx.items() for (s, o) in sos], dtype=np.int32)
        calls = {}

        def topk_call(direction, k):
            a = order[:, 1 if direction else 0].astype(np.int64)
            r = order[:, 2].astype(np.int64)
            csr = lp._exclusions(a, r, direction, True, None, N_ENT)
            off, ent = (torch.as_tensor(x, device=dev) for x in csr)
            q = torch.as_tensor(np.stack([a, r], axis=1).astype(np.int32), device=dev)
            n = len(a)
            nbytes = lib.skge_topk_workspace_bytes(n, d, k, N_ENT)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            eo = torch.empty((n, k), dtype=torch.int32, device=dev)
            so = torch.empty((n, k), dtype=torch.float32, device=dev)
            keep = (off, ent, q, ws, eo, so)
            return lambda: L.check(lib.skge_topk(
                L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), N_ENT, d, L.ptr(q), n,
                direction, k, L.ptr(off), L.ptr(ent), L.ptr(ws), nbytes, L.ptr(eo), L.ptr(so)),
                "topk") or keep

        for k in KS:
            calls["tails_k%d" % k] = topk_call(0, k)
            calls["heads_k%d" % k] = topk_call(1, k)
        toff, tent, hoff, hent = ev._known_answers(order.tolist(), dev)
        rq = torch.as_tensor(order, device=dev)
        rbytes = lib.skge_rank_known_workspace_bytes(len(order), d)
        rws = torch.empty(rbytes, dtype=torch.uint8, device=dev)
        rout = torch.empty((len(order), 4), dtype=torch.int32, device=dev)
        calls["rank_known"] = lambda: L.check(lib.skge_rank_known(
            L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), N_ENT, d, L.ptr(rq), len(order),
            L.ptr(toff), L.ptr(tent), L.ptr(hoff), L.ptr(hent), L.ptr(rws), rbytes, L.ptr(rout)),
            "rank")
        for _ in range(args.warmup):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        ms = {key: [] for key in calls}
        for _ in range(args.repeats):          # interleaved: one of each per repeat
            for key, fn in calls.items():
                t0 = torch.cuda.Event(enable_timing=True)
                t1 = torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                ms[key].append(t0.elapsed_time(t1))
        res = {key: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
                     "max_ms": round(float(np.max(v)), 4)} for key, v in ms.items()}
        rank = res["rank_known"]["median_ms"]
        for k in KS:     # both directions of top-k against the one call that ranks both
            both = res["tails_k%d" % k]["median_ms"] + res["heads_k%d" % k]["median_ms"]
            res["topk_both_k%d_over_rank_known" % k] = round(both / rank, 3)
        out["models"][name] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
