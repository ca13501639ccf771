#!/usr/bin/env python3
"""Type-constrained ranking time (skge_rank_pools) against its yardstick
skge_rank_known, timed in the same process:

  wn18   the WN18-shaped KG of bench.py, N = 40943, M = 18, d = 200
  zipf   its Zipf(1.1) variant (skewed entities: a few large typed pools)

5000 test triples, TransE / HolE / RESCAL, three calls per model: rank_known
(every entity), rank_pools with the typed pools of the KG (tail -> range of p,
head -> domain), rank_pools with every vector on pool -1 (the same rows as
rank_known through the grouped, gathered path).  Per call milliseconds, and
nanoseconds per (query vector x candidate row) -- the rows being N for
rank_known and -1, and the vector's pool size for typed.  The baseline is
rank_known itself, whose code is unchanged; its run-to-run spread (min .. max
over the rounds) is the margin.

Then what the protocol is for: a TransE trained with typed negatives
(CorruptedSampler, device_negatives=True) on a KG with planted types, its
filtered MRR over all entities and over typed pools.

Device events around each call, warm-up first, the timed calls interleaved
over the rounds, medians reported.  Usage: python tools/bench_typed_eval.py
[--rounds 10] [--epochs 20] [--out profiles/typed_eval/bench_typed_eval.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scikit-kge_amd")]

D = 200
NQ = 5000


def timed(calls, rounds, warmup):
    """{key: (median, min, max) ms}: interleaved, one of each per round."""
    import numpy as np
    import torch
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {key: [] for key in calls}
    for _ in range(rounds):
        for key, fn in calls.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ms[key].append(t0.elapsed_time(t1))
    return {key: (float(np.median(v)), float(min(v)), float(max(v))) for key, v in ms.items()}


def geometry(name, trip, rounds, warmup):
    import numpy as np
    import torch
    import skge_amd as S
    from skge_amd import _lib as L
    from skge_amd.eval import _model_code
    from bench import N_ENT, N_REL
    lib = L.lib()
    test = trip[:NQ]
    lines = []
    for mname in ("transe", "hole", "rescal"):
        np.random.seed(42)
        m = {"transe": S.TransE, "hole": S.HolE, "rescal": S.RESCAL}[mname](
            (N_ENT, N_ENT, N_REL), D)
        code, rel = _model_code(m)
        E, dev = m.params["E"], m.device
        ev = S.FilteredRankingEval(test, trip)
        order = np.asarray([(s, o, p) for p, sos in ev.idx.items() for (s, o) in sos],
                           dtype=np.int32)
        nq = len(order)
        q = torch.as_tensor(order, device=dev)
        toff, tent, hoff, hent = ev._known_answers(order.tolist(), dev)
        pools, tp, hp = ev.typed_pools(N_REL)
        off, ent = S.pool_csr(pools, N_ENT)
        n_pools = len(off) - 1
        d_off, d_ent = torch.as_tensor(off, device=dev), torch.as_tensor(ent, device=dev)
        typed = np.stack([tp, hp], axis=1).reshape(-1).astype(np.int32)
        vp = {"typed": torch.as_tensor(typed, device=dev),
              "minus1": torch.full((2 * nq,), -1, dtype=torch.int32, device=dev)}
        kb = lib.skge_rank_known_workspace_bytes(nq, D)
        kws = torch.empty(kb, dtype=torch.uint8, device=dev)
        pb = lib.skge_rank_pools_workspace_bytes(nq, D, n_pools)
        pws = torch.empty(pb, dtype=torch.uint8, device=dev)
        out = {key: torch.empty((nq, 4), dtype=torch.int32, device=dev)
               for key in ("rank_known", "typed", "minus1")}

        def pool_call(key):
            return lambda: L.check(lib.skge_rank_pools(
                L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), N_ENT, D, L.ptr(q), nq,
                L.ptr(d_off), L.ptr(d_ent), n_pools, L.ptr(vp[key]), L.ptr(toff), L.ptr(tent),
                L.ptr(hoff), L.ptr(hent), L.ptr(pws), pb, L.ptr(out[key])), "rank (pools)")
        calls = {
            "rank_known": lambda: L.check(lib.skge_rank_known(
                L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), N_ENT, D, L.ptr(q), nq,
                L.ptr(toff), L.ptr(tent), L.ptr(hoff), L.ptr(hent), L.ptr(kws), kb,
                L.ptr(out["rank_known"])), "rank"),
            "typed": pool_call("typed"), "minus1": pool_call("minus1")}
        t = timed(calls, rounds, warmup)
        same = bool((out["minus1"] == out["rank_known"]).all().item())
        sizes = np.diff(off)
        rows = {"rank_known": 2.0 * nq * N_ENT, "minus1": 2.0 * nq * N_ENT,
                "typed": float(sizes[typed].sum())}
        line = {"kg": name, "model": mname, "n_ent": N_ENT, "n_rel": N_REL, "d": D, "queries": nq,
                "rounds": rounds, "minus1_equals_rank_known": same,
                "typed_rows_share": round(rows["typed"] / rows["rank_known"], 4),
                "typed_pool_sizes_min_median_max": [int(sizes.min()), int(np.median(sizes)),
                                                    int(sizes.max())]}
        for key, (med, lo, hi) in t.items():
            line[key + "_ms"] = round(med, 4)
            line[key + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
            line[key + "_ns_per_vector_row"] = round(med * 1e6 / rows[key], 5)
        base = line["rank_known_ns_per_vector_row"]
        line["rank_known_spread"] = round((t["rank_known"][2] - t["rank_known"][1])
                                          / t["rank_known"][0], 4)
        line["minus1_over_rank_known"] = round(line["minus1_ms"] / line["rank_known_ms"], 4)
        line["typed_per_row_over_rank_known"] = round(line["typed_ns_per_vector_row"] / base, 3)
        line["rank_known_over_typed_ms"] = round(line["rank_known_ms"] / line["typed_ms"], 2)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del m
        torch.cuda.empty_cache()
    return lines


def planted_kg(rs, n_ent, n_rel, n, n_types=6):
    """Triples with planted types: entities fall into n_types classes, relation
    p joins class p % n_types to class (p // n_types + p + 1) % n_types, and the
    object is the subject's position in its class shifted by p (plus a little
    noise): a translation along the class, which TransE can learn."""
    import numpy as np
    cl = rs.randint(n_types, size=n_ent)
    members = [np.flatnonzero(cl == c) for c in range(n_types)]
    p = rs.randint(n_rel, size=n)
    a, b = p % n_types, (p // n_types + p + 1) % n_types
    s_pos = np.array([rs.randint(len(members[c])) for c in a.tolist()])
    s = np.array([members[c][i] for c, i in zip(a.tolist(), s_pos.tolist())])
    o_pos = s_pos + 37 * p + rs.randint(3, size=n)
    o = np.array([members[c][i % len(members[c])] for c, i in zip(b.tolist(), o_pos.tolist())])
    return np.unique(np.stack([s, o, p], axis=1), axis=0).astype(np.int32)


def training(epochs):
    import numpy as np
    import torch
    import skge_amd as S
    from bench import N_ENT, N_REL
    rs = np.random.RandomState(7)
    kg = planted_kg(rs, N_ENT, N_REL, 141442 + NQ)
    kg = kg[rs.permutation(len(kg))]
    test, train = kg[:NQ], kg[NQ:]
    sz = (N_ENT, N_ENT, N_REL)
    np.random.seed(42)
    m = S.TransE(sz, 50)
    tr = S.PairwiseStochasticTrainer(
        m, nbatches=100, max_epochs=epochs, learning_rate=0.1, margin=2.0, device_loop=True,
        device_negatives=True, seed=11, file_grad=None, file_embed=None,
        samplef=S.CorruptedSampler(1, train, S.type_index(train.tolist()), modes=[0, 1]).sample)
    tr.fit(train, [1] * len(train))
    torch.cuda.synchronize()
    ev = S.FilteredRankingEval(test, kg)
    raw, filt = S.ranking_scores(*ev.positions(m))
    traw, tfilt = S.ranking_scores(*ev.typed_positions(m, train))
    cand = ev.last_typed_candidates
    line = {"kg": "planted types: 6 classes, relation p joins two of them", "model": "transe",
            "d": 50, "epochs": epochs, "nbatches": 100, "train": len(train), "held_out": len(test),
            "sampler": "CorruptedSampler modes [0, 1], device_negatives",
            "untyped": {"mrr_raw": round(raw[0], 4), "mrr_filtered": round(filt[0], 4),
                        "hits10_filtered": round(filt[2], 2)},
            "typed": {"mrr_raw": round(traw[0], 4), "mrr_filtered": round(tfilt[0], 4),
                      "hits10_filtered": round(tfilt[2], 2),
                      "candidates_median": int(np.median(cand)), "of_entities": N_ENT}}
    print(json.dumps(line), flush=True)
    return line


def readme(device, lines, train):
    out = ["# Type-constrained ranking: measured", "",
           "Written by `tools/bench_typed_eval.py` on %s: device events, medians of interleaved "
           "rounds.  `bench_typed_eval.jsonl` holds every figure (one line per KG and model, "
           "then the trained model)." % device, "",
           "`rank_known` scores every entity; `typed` ranks over the range / domain pools of the "
           "KG; `minus1` sends every vector through the pool path with pool -1 (the same rows as "
           "`rank_known`).  ns = nanoseconds per (query vector x candidate row); spread = "
           "rank_known's (max - min) / median over the rounds.", "",
           "| KG | model | rank_known ms (spread) | minus1 ms (/ rank_known) | typed ms | typed rows "
           "share | ns rank_known | ns typed (/ rank_known) | minus1 == rank_known |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in lines:
        out.append("| %s | %s | %.3f (%.3f) | %.3f (%.3f) | %.3f | %.4f | %.5f | %.5f (%.2f) | %s |" % (
            r["kg"], r["model"], r["rank_known_ms"], r["rank_known_spread"], r["minus1_ms"],
            r["minus1_over_rank_known"], r["typed_ms"], r["typed_rows_share"],
            r["rank_known_ns_per_vector_row"], r["typed_ns_per_vector_row"],
            r["typed_per_row_over_rank_known"], r["minus1_equals_rank_known"]))
    out.append("")
    if train:
        out += ["## A model trained with typed negatives", "",
                "TransE d = %d, %d epochs of %d batches, %s; %d training and %d held-out triples "
                "(%s).  Typed pools from the training triples; median %d candidates of %d." % (
                    train["d"], train["epochs"], train["nbatches"], train["sampler"],
                    train["train"], train["held_out"], train["kg"],
                    train["typed"]["candidates_median"], train["typed"]["of_entities"]), "",
                "| protocol | raw MRR | filtered MRR | filtered hits@10 % |", "|---|---|---|---|"]
        for key in ("untyped", "typed"):
            t = train[key]
            out.append("| %s | %.4f | %.4f | %.2f |" % (key, t["mrr_raw"], t["mrr_filtered"],
                                                        t["hits10_filtered"]))
        out.append("")
    else:
        out += ["Trained-model comparison: not measured in this run.", ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--skip", default="", help="comma list of wn18, zipf, training")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "typed_eval",
                                                  "bench_typed_eval.jsonl"))
    args = ap.parse_args()
    import torch
    from skge_amd import _lib as L
    from bench import make_wn18_kg, make_zipf_kg
    L.require_gpu()
    skip = set(args.skip.split(","))
    lines = []
    if "wn18" not in skip:
        lines += geometry("wn18", make_wn18_kg(), args.rounds, args.warmup)
    if "zipf" not in skip:
        lines += geometry("zipf", make_zipf_kg(), args.rounds, args.warmup)
    train = None if "training" in skip else training(args.epochs)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines + ([train] if train else []):
                f.write(json.dumps(r) + "\n")
        with open(os.path.join(os.path.dirname(args.out), "README.md"), "w") as f:
            f.write(readme(torch.cuda.get_device_name(0), lines, train))


if __name__ == "__main__":
    main()
