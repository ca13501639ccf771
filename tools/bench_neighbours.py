#!/usr/bin/env python3
"""Nearest-neighbour time at the WN18 geometry (|E| = 40943, d = 200, a
nunif-initialised E): skge_neighbours for every row against every other row
by cosine at k = 10 and k = 100, and for 5000 rows at k = 10.

The yardstick is skge_topk's dot form -- the VALU register micro-tile
selection -- timed in the same process: the k = 10 tails of 5000 queries of a
HolE model of the same N and d, nothing excluded.  Both do one fp32 fma per
(query, table row, dim) and then select, so the time per (query x row) is
compared; the achieved TFLOP/s (2 nq N d / time, the norms, the selection and
the merge all inside the timed call) is set against the 157.3 TF fp32 peak.

Device events around each call, warm-up first, the timed calls interleaved
over the repeats, medians reported; buffers are made outside the timed
window.  Usage: python tools/bench_neighbours.py [--repeats 10]
[--out profiles/neighbours/bench_neighbours.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scikit-kge_amd")]

PEAK_TF = 157.3
NQ_SOME = 5000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbours",
                                                  "bench_neighbours.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import skge_amd as S
    from skge_amd import _lib as L
    from skge_amd.eval import _model_code
    from bench import make_wn18_kg, N_ENT, N_REL
    L.require_gpu()
    lib = L.lib()
    np.random.seed(42)
    m = S.HolE((N_ENT, N_ENT, N_REL), 200)
    code, rel = _model_code(m)
    E, dev, d = m.params["E"], m.device, m.d
    trip = make_wn18_kg()[:NQ_SOME]
    calls, work = {}, {}

    def nb_call(nq, k, rows):
        nbytes = lib.skge_neighbours_workspace_bytes(nq, N_ENT, d, k)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        io = torch.empty((nq, k), dtype=torch.int32, device=dev)
        so = torch.empty((nq, k), dtype=torch.float32, device=dev)
        keep = (ws, io, so, rows)
        return lambda: L.check(lib.skge_neighbours(
            L.stream_ptr(), L.ptr(E.data), N_ENT, d, None, L.ptr(rows), nq, 0, k, L.ptr(ws),
            nbytes, L.ptr(io), L.ptr(so)), "neighbours") or keep

    some = torch.as_tensor(np.ascontiguousarray(trip[:, 0]).astype(np.int32), device=dev)
    for key, nq, k, rows in (("all_rows_k10", N_ENT, 10, None), ("all_rows_k100", N_ENT, 100, None),
                             ("rows5000_k10", NQ_SOME, 10, some)):
        calls[key] = nb_call(nq, k, rows)
        work[key] = nq

    def topk_call(k):
        q = torch.as_tensor(np.ascontiguousarray(trip[:, [0, 2]]).astype(np.int32), device=dev)
        n = len(trip)
        nbytes = lib.skge_topk_workspace_bytes(n, d, k, N_ENT)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        eo = torch.empty((n, k), dtype=torch.int32, device=dev)
        so = torch.empty((n, k), dtype=torch.float32, device=dev)
        keep = (q, ws, eo, so)
        return lambda: L.check(lib.skge_topk(
            L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), N_ENT, d, L.ptr(q), n, 0, k,
            None, None, L.ptr(ws), nbytes, L.ptr(eo), L.ptr(so)), "topk") or keep

    calls["topk_hole_tails5000_k10"] = topk_call(10)
    work["topk_hole_tails5000_k10"] = NQ_SOME
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
    res = {}
    for key, v in ms.items():
        med = float(np.median(v))
        pairs = float(work[key]) * N_ENT
        tf = 2.0 * pairs * d / (med * 1e-3) / 1e12
        res[key] = {"median_ms": round(med, 4), "min_ms": round(float(np.min(v)), 4),
                    "max_ms": round(float(np.max(v)), 4),
                    "ps_per_query_row": round(med * 1e9 / pairs, 3),
                    "tflops": round(tf, 2), "of_fp32_peak": round(tf / PEAK_TF, 4)}
    ref = res["topk_hole_tails5000_k10"]["ps_per_query_row"]
    for key in ("all_rows_k10", "all_rows_k100", "rows5000_k10"):
        res[key]["topk_valu_over_this_per_query_row"] = round(ref / res[key]["ps_per_query_row"], 3)
    out = {"n_ent": N_ENT, "d": d, "repeats": args.repeats, "peak_tf": PEAK_TF,
           "device": torch.cuda.get_device_name(0), "jobs": res}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
