#!/usr/bin/env python3
"""Subgraph embedding and ranking time at the WN18 geometry (|E| = 40943,
|R| = 18, d = 200): the subgraphs of the whole KG at mincard 10, both kinds,
and 5000 test queries.  The KG is bench.py's Zipf(1.1)-skewed one (--kg zipf,
the default): the uniform one has no group above 5 members.

Timed with device events after warm-up, the calls interleaved over the
repeats, medians reported; the host-side set-up (grouping, the CSR and its
inverse, the skip ids, the buffers) is outside the timed window:
  embed       skge_subgraph_embed, SA only
  embed_var   skge_subgraph_embed, SA and SV
  rank        skge_subgraph_rank over SA, both directions of the 5000 queries
  rank_known  skge_rank_known over E for the same queries, for scale
Beside them: embed's own traffic, 4d (members + 2S) bytes (SA only: + S),
against the measured streaming gather rate (skge_roofline_gather, bench.py's
measured_roofline), rank's and rank_known's time per query and row, and the
time of the NumPy restatement (tests/subgraph_ref.py) on the CPU: embed over
every subgraph, ranks over --cpu-queries queries, scaled to the 5000.
Usage: python tools/bench_subgraphs.py [--models transe,hole] [--repeats 20]
[--out profiles/subgraphs/bench_subgraphs.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scikit-kge_amd"), os.path.join(ROOT, "tests")]

MINCARD, D, NQ = 10, 200, 5000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="transe,hole")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-queries", type=int, default=20)
    ap.add_argument("--kg", choices=("zipf", "uniform"), default="zipf")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subgraphs",
                                                  "bench_subgraphs.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import skge_amd as S
    import subgraph_ref as G
    from skge_amd import _lib as L
    from skge_amd.eval import _model_code
    from bench import make_wn18_kg, make_zipf_kg, measured_roofline, N_ENT, N_REL
    L.require_gpu()
    # the uniform WN18-shaped KG has no group above 5 members, so nothing
    # passes mincard 10; the Zipf(1.1) variant (bench.py --skew zipf) has
    # hubs, as WN18 itself: 2892 subgraphs, the largest of 671 members
    trip = make_zipf_kg() if args.kg == "zipf" else make_wn18_kg()
    test = trip[:NQ]
    lib = L.lib()
    t0 = time.perf_counter()
    sg = S.Subgraphs.from_triples(trip, MINCARD)
    t_group = time.perf_counter() - t0
    n_sub, members = sg.get_Nsubgraphs(), int(sg.mem_off[-1])
    if n_sub == 0:
        raise SystemExit("no group of the %s KG has more than %d members" % (args.kg, MINCARD))
    dev = torch.device("cuda:0")
    _, _, gather_gbs = measured_roofline(dev, N_ENT, D, 262144, 5, 0, 0, launches=10, reps=3)
    out = {"kg": args.kg, "queries": len(test), "n_ent": N_ENT, "n_rel": N_REL, "d": D, "mincard": MINCARD,
           "subgraphs": n_sub, "spo": int((sg.kind == 0).sum()), "pos": int((sg.kind == 1).sum()),
           "members": members, "largest": int(sg.size.max()), "grouping_host_s": round(t_group, 3),
           "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "streaming_gather_GB_s": round(gather_gbs, 1), "models": {}}
    for name in args.models.split(","):
        np.random.seed(42)
        m = {"transe": S.TransE, "hole": S.HolE, "rescal": S.RESCAL}[name]((N_ENT, N_ENT, N_REL), D)
        code, rel = _model_code(m)
        E, d = m.params["E"], m.d
        off, ent, ans_off, ans_sub = sg.device_arrays(dev, N_ENT)
        SA = torch.empty((n_sub, d), dtype=torch.float32, device=dev)
        SV = torch.empty_like(SA)
        ebytes = lib.skge_subgraph_embed_workspace_bytes(n_sub, d, members)
        ews = torch.empty(ebytes, dtype=torch.uint8, device=dev)

        def embed(var):
            return lambda: L.check(lib.skge_subgraph_embed(
                L.stream_ptr(), L.ptr(E.data), N_ENT, d, L.ptr(off), L.ptr(ent), n_sub, L.ptr(SA),
                L.ptr(SV) if var else None, L.ptr(ews), ebytes), "embed")

        ev = S.SubgraphRankingEval(test, sg)
        order = np.asarray(ev._queries(), dtype=np.int32)
        n = len(order)
        skip_t = torch.as_tensor(np.array([sg.subgraph_id(0, s, p) for s, o, p in order.tolist()],
                                          dtype=np.int32), device=dev)
        skip_h = torch.as_tensor(np.array([sg.subgraph_id(1, o, p) for s, o, p in order.tolist()],
                                          dtype=np.int32), device=dev)
        rq = torch.as_tensor(order, device=dev)
        sbytes = lib.skge_subgraph_rank_workspace_bytes(n, d)
        sws = torch.empty(sbytes, dtype=torch.uint8, device=dev)
        sout = torch.empty((n, 2), dtype=torch.int32, device=dev)
        sfound = torch.empty((n, 2), dtype=torch.int32, device=dev)
        fe = S.FilteredRankingEval(test, trip)
        toff, tent, hoff, hent = fe._known_answers(order.tolist(), dev)
        rbytes = lib.skge_rank_known_workspace_bytes(n, d)
        rws = torch.empty(rbytes, dtype=torch.uint8, device=dev)
        rout = torch.empty((n, 4), dtype=torch.int32, device=dev)
        calls = {
            "embed": embed(False),
            "embed_var": embed(True),
            "rank": lambda: L.check(lib.skge_subgraph_rank(
                L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), N_ENT, d, L.ptr(SA), n_sub,
                L.ptr(rq), n, L.ptr(skip_t), L.ptr(skip_h), L.ptr(ans_off), L.ptr(ans_sub),
                L.ptr(sws), sbytes, L.ptr(sout), L.ptr(sfound)), "subgraph rank"),
            "rank_known": lambda: L.check(lib.skge_rank_known(
                L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), N_ENT, d, L.ptr(rq), n,
                L.ptr(toff), L.ptr(tent), L.ptr(hoff), L.ptr(hent), L.ptr(rws), rbytes,
                L.ptr(rout)), "rank"),
        }
        for _ in range(args.warmup):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        ms = {key: [] for key in calls}
        for _ in range(args.repeats):          # interleaved: one of each per repeat
            for key, fn in calls.items():
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[key].append(e0.elapsed_time(e1))
        res = {key: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
                     "max_ms": round(float(np.max(v)), 4)} for key, v in ms.items()}
        for key, rows_out in (("embed", 1), ("embed_var", 2)):
            # every member row once (SV's second pass over a group's members
            # follows its first at once: not counted again) + the rows written
            nbytes = 4.0 * d * (members + rows_out * n_sub)
            gbs = nbytes / (res[key]["median_ms"] * 1e-3) / 1e9
            res[key].update({"bytes": int(nbytes), "GB_s": round(gbs, 1),
                             "frac_of_streaming_gather": round(gbs / gather_gbs, 4)})
        per_sub = res["rank"]["median_ms"] * 1e6 / (2.0 * n * n_sub)
        per_ent = res["rank_known"]["median_ms"] * 1e6 / (2.0 * n * N_ENT)
        res["rank"]["ns_per_query_row"] = round(per_sub, 5)
        res["rank_known"]["ns_per_query_row"] = round(per_ent, 5)
        res["rank_over_rank_known_per_query_row"] = round(per_sub / per_ent, 3)
        res["found_tail"] = int(sfound[:, 0].sum().item())
        res["found_head"] = int(sfound[:, 1].sum().item())
        # the NumPy restatement on the CPU
        Eh = E.data.cpu().numpy().astype(np.float64)
        Rh = rel.data.cpu().numpy().astype(np.float64).reshape(N_REL, -1)
        t0 = time.perf_counter()
        groups = G.group(trip, MINCARD)
        t_g = time.perf_counter() - t0
        t0 = time.perf_counter()
        SA64, _ = G.embed(Eh, groups)
        t_e = time.perf_counter() - t0
        nc = max(1, min(args.cpu_queries, n))
        t0 = time.perf_counter()
        want = G.ranks(lambda s, o, p, dr: G.scores(name, Eh, Rh, SA64, s, o, p, dr), groups,
                       order[:nc])
        t_r = time.perf_counter() - t0
        got = torch.cat([sout, sfound], dim=1)[:nc].cpu().numpy()
        res["cpu_restatement"] = {"group_s": round(t_g, 3), "embed_s": round(t_e, 3),
                                  "rank_s_per_query": round(t_r / nc, 5),
                                  "rank_s_5000_scaled": round(t_r / nc * n, 1),
                                  "queries_timed": nc,
                                  "ranks_equal_fp64": int((got == want).all(axis=1).sum())}
        out["models"][name] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
