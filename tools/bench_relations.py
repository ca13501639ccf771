#!/usr/bin/env python3
"""Relation prediction time (skge_relrank, skge_reltopk at k = 10) at two
geometries, with its yardsticks timed in the same process:

  wn18   N = 40943, M = 18, d = 200, 5000 test triples, TransE / HolE / RESCAL
  many   M = 1345, d = 200, the same 5000 (s, o) pairs (RESCAL's W: 215 MB)

TransE / HolE: skge_rank_known over E on the same triples, per (query x row).
RESCAL: TFLOP/s = 2 nq M d (d + 1) / time against the 157.3 TF fp32 peak, and
torch's own fp32 path for the same score matrix, ((E_S @ W[j]) * E_O).sum(1)
per relation.

Then the number the feature exists to produce: a TransE trained on a KG whose
relations can be told from (s, o) (18 clusters on a line, p = the clusters'
distance), twice from the same init under device_negatives=True, with
modes [0, 1] and with [0, 1, 2]; the filtered relation MRR on held-out triples
of each.

Device events around each call, warm-up first, the timed calls interleaved
over the rounds, medians reported.  Usage: python tools/bench_relations.py
[--rounds 10] [--epochs 20] [--out profiles/relations/bench_relations.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scikit-kge_amd")]

PEAK_TF = 157.3
D = 200
NQ = 5000


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
    return {key: round(float(np.median(v)), 4) for key, v in ms.items()}


def geometry(name, M, models, test, trip, rounds, warmup):
    import numpy as np
    import torch
    import skge_amd as S
    from skge_amd import _lib as L
    from skge_amd.eval import _model_code
    from bench import N_ENT
    lib = L.lib()
    res = {}
    for mname in models:
        np.random.seed(42)
        m = {"transe": S.TransE, "hole": S.HolE, "rescal": S.RESCAL}[mname]((N_ENT, N_ENT, M), D)
        code, rel = _model_code(m)
        E, dev = m.params["E"], m.device
        ev = S.FilteredRankingEval(test, trip)
        order = np.asarray([(s, o, p) for p, sos in ev.idx.items() for (s, o) in sos],
                           dtype=np.int32)
        nq = len(order)
        q = torch.as_tensor(order, device=dev)
        pairs = torch.as_tensor(np.ascontiguousarray(order[:, :2]), device=dev)
        off, krel = ev._known_relations(order.tolist(), dev)
        rb = lib.skge_relrank_workspace_bytes(nq, D, M, code)
        rws = torch.empty(rb, dtype=torch.uint8, device=dev)
        rout = torch.empty((nq, 2), dtype=torch.int32, device=dev)
        tb = lib.skge_reltopk_workspace_bytes(nq, D, 10, M, code)
        tws = torch.empty(tb, dtype=torch.uint8, device=dev)
        tid = torch.empty((nq, 10), dtype=torch.int32, device=dev)
        tsc = torch.empty((nq, 10), dtype=torch.float32, device=dev)
        calls = {
            "relrank": lambda: L.check(lib.skge_relrank(
                L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), N_ENT, M, D, L.ptr(q), nq,
                L.ptr(off), L.ptr(krel), L.ptr(rws), rb, L.ptr(rout)), "relrank"),
            "reltopk_k10": lambda: L.check(lib.skge_reltopk(
                L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), N_ENT, M, D, L.ptr(pairs),
                nq, 10, None, None, L.ptr(tws), tb, L.ptr(tid), L.ptr(tsc)), "reltopk"),
        }
        if mname == "rescal":
            ES, EO = E.data[q[:, 0].long()], E.data[q[:, 1].long()]
            W = rel.data.view(M, D, D)
            sc = torch.empty((M, nq), dtype=torch.float32, device=dev)

            def torch_scores():
                for j in range(M):
                    sc[j] = ((ES @ W[j]) * EO).sum(1)
            calls["torch_scores"] = torch_scores
        else:
            toff, tent, hoff, hent = ev._known_answers(order.tolist(), dev)
            kb = lib.skge_rank_known_workspace_bytes(nq, D)
            kws = torch.empty(kb, dtype=torch.uint8, device=dev)
            kout = torch.empty((nq, 4), dtype=torch.int32, device=dev)
            calls["rank_known"] = lambda: L.check(lib.skge_rank_known(
                L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), N_ENT, D, L.ptr(q), nq,
                L.ptr(toff), L.ptr(tent), L.ptr(hoff), L.ptr(hent), L.ptr(kws), kb, L.ptr(kout)),
                "rank")
        r = timed(calls, rounds, warmup)
        r["relrank_ps_per_query_row"] = round(r["relrank"] * 1e9 / (nq * M), 2)
        r["reltopk_ps_per_query_row"] = round(r["reltopk_k10"] * 1e9 / (nq * M), 2)
        if mname == "rescal":
            flop = 2.0 * nq * M * D * (D + 1)
            for key in ("relrank", "reltopk_k10", "torch_scores"):
                r[key + "_tflops"] = round(flop / (r[key] * 1e-3) / 1e12, 2)
            r["relrank_of_peak"] = round(r["relrank_tflops"] / PEAK_TF, 3)
            r["torch_over_relrank"] = round(r["torch_scores"] / r["relrank"], 3)
            # the kernel's matrix against torch's, on the device's own numbers
            S1 = rws[:nq * M * 4].view(torch.float32).view(nq, M)
            calls["relrank"]()
            torch_scores()
            ref = sc.t().double()
            r["max_abs_diff_vs_torch_over_max_abs"] = float(
                ((S1.double() - ref).abs().max() / ref.abs().max()).item())
        else:
            r["rank_known_ps_per_query_row"] = round(r["rank_known"] * 1e9 / (2 * nq * N_ENT), 2)
            r["relrank_over_rank_known_per_query_row"] = round(
                r["relrank_ps_per_query_row"] / r["rank_known_ps_per_query_row"], 2)
        res[mname] = r
        del m
        torch.cuda.empty_cache()
    return {"n_ent": N_ENT, "n_rel": M, "d": D, "queries": len(test), "models": res}


def cluster_kg(rs, n_ent, n_rel, n):
    """Triples whose relation is the distance between the clusters of s and o
    (n_rel clusters on a line): what a translation model can learn."""
    import numpy as np
    cl = rs.randint(n_rel, size=n_ent)
    members = [np.flatnonzero(cl == c) for c in range(n_rel)]
    p = rs.randint(n_rel, size=n)
    cs = (rs.rand(n) * (n_rel - p)).astype(np.int64)
    s = np.array([members[c][rs.randint(len(members[c]))] for c in cs.tolist()])
    o = np.array([members[c][rs.randint(len(members[c]))] for c in (cs + p).tolist()])
    return np.unique(np.stack([s, o, p], axis=1), axis=0).astype(np.int32)


def training(epochs):
    import numpy as np
    import torch
    import skge_amd as S
    from bench import N_ENT, N_REL
    rs = np.random.RandomState(7)
    kg = cluster_kg(rs, N_ENT, N_REL, 141442 + NQ)
    kg = kg[rs.permutation(len(kg))]
    test, train = kg[:NQ], kg[NQ:]
    sz = (N_ENT, N_ENT, N_REL)
    out = {"train": len(train), "held_out": len(test), "epochs": epochs, "nbatches": 100, "d": 50,
           "kg": "18 clusters on a line, p = cluster(o) - cluster(s)"}
    ev = S.FilteredRankingEval(test, kg)
    for modes in ([0, 1], [0, 1, 2]):
        np.random.seed(42)
        m = S.TransE(sz, 50)
        if not out.get("mrr_untrained"):
            out["mrr_untrained"] = round(S.relation_ranking_scores(*ev.relation_positions(m))[1][0], 4)
        tr = S.PairwiseStochasticTrainer(
            m, nbatches=100, max_epochs=epochs, learning_rate=0.1, margin=2.0, device_loop=True,
            device_negatives=True, seed=11, file_grad=None, file_embed=None,
            samplef=S.RandomModeSampler(1, modes, train, sz).sample)
        tr.fit(train, [1] * len(train))
        torch.cuda.synchronize()
        raw, filt = S.relation_ranking_scores(*ev.relation_positions(m))
        ent = S.ranking_scores(*ev.positions(m))[1]
        out["modes_" + "".join(map(str, modes))] = {
            "relation_mrr_filtered": round(filt[0], 4), "relation_hits1_filtered": round(filt[2], 2),
            "relation_mrr_raw": round(raw[0], 4), "entity_mrr_filtered": round(ent[0], 4)}
        print("modes %s: filtered relation MRR %.4f (hits@1 %.1f%%), entity MRR %.4f"
              % (modes, filt[0], filt[2], ent[0]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--many", type=int, default=1345)
    ap.add_argument("--skip", default="", help="comma list of wn18, many, training")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relations",
                                                  "bench_relations.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from skge_amd import _lib as L
    from bench import make_wn18_kg, N_REL
    L.require_gpu()
    skip = set(args.skip.split(","))
    trip = make_wn18_kg()
    test = trip[:NQ]
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "peak_fp32_tf": PEAK_TF}
    if "wn18" not in skip:
        out["wn18"] = geometry("wn18", N_REL, ("transe", "hole", "rescal"), test, trip,
                               args.rounds, args.warmup)
        print(json.dumps(out["wn18"]), flush=True)
    if "many" not in skip:
        rs = np.random.RandomState(3)
        many = np.array(trip)
        many[:, 2] = rs.randint(args.many, size=len(many))
        out["many"] = geometry("many", args.many, ("transe", "hole", "rescal"), many[:NQ], many,
                               args.rounds, args.warmup)
        print(json.dumps(out["many"]), flush=True)
    if "training" not in skip:
        out["training"] = training(args.epochs)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        with open(os.path.join(os.path.dirname(args.out), "README.md"), "w") as f:
            f.write(readme(out))


def readme(out):
    lines = ["# Relation prediction: measured", "",
             "Written by `tools/bench_relations.py` on %s: device events, medians of %d "
             "interleaved rounds.  `bench_relations.json` holds every figure." % (
                 out["device"], out["rounds"]), ""]
    for g in ("wn18", "many"):
        if g not in out:
            lines += ["%s: not measured in this run." % g, ""]
            continue
        r = out[g]
        lines += ["## %s: N = %d, M = %d, d = %d, %d queries" % (g, r["n_ent"], r["n_rel"], r["d"],
                                                                  r["queries"]), "",
                  "| model | relrank ms | reltopk k=10 ms | ps per (query x row) | yardstick |",
                  "|---|---|---|---|---|"]
        for name, m in r["models"].items():
            if name == "rescal":
                y = ("%.2f TF = %.3f of peak; torch %.3f ms = %.2f TF, torch / relrank %.2f"
                     % (m["relrank_tflops"], m["relrank_of_peak"], m["torch_scores"],
                        m["torch_scores_tflops"], m["torch_over_relrank"]))
            else:
                y = ("rank_known %.3f ms = %.2f ps per (query x row); relrank / rank_known %.2f"
                     % (m["rank_known"], m["rank_known_ps_per_query_row"],
                        m["relrank_over_rank_known_per_query_row"]))
            lines.append("| %s | %.4f | %.4f | %.2f | %s |" % (
                name, m["relrank"], m["reltopk_k10"], m["relrank_ps_per_query_row"], y))
        lines.append("")
    if "training" in out:
        t = out["training"]
        lines += ["## Training with and without relation corruption", "",
                  "TransE d = %d, %d epochs of %d batches, %d training and %d held-out triples "
                  "(%s), device_negatives=True, same init.  Untrained filtered relation MRR %.4f."
                  % (t["d"], t["epochs"], t["nbatches"], t["train"], t["held_out"], t["kg"],
                     t["mrr_untrained"]), "",
                  "| modes | filtered relation MRR | hits@1 % | raw relation MRR | filtered entity MRR |",
                  "|---|---|---|---|---|"]
        for key in ("modes_01", "modes_012"):
            m = t[key]
            lines.append("| %s | %.4f | %.2f | %.4f | %.4f |" % (
                key[6:], m["relation_mrr_filtered"], m["relation_hits1_filtered"],
                m["relation_mrr_raw"], m["entity_mrr_filtered"]))
        lines.append("")
    else:
        lines += ["Training comparison: not measured in this run.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
