#!/usr/bin/env python3
"""What the negative sampler's kind costs in the device epochs: RANDOM
(RandomModeSampler), TYPED (CorruptedSampler over type_index(xs)) and LCWA
(LCWASampler), on the WN18-shaped KG of bench.py (make_wn18_kg: N = 40943,
M = 18, T = 141442; |subj(p)| ~ 0.175 N, so an LCWA s-corruption takes ~6
tries), d = 200, AdaGrad, nb = 100.

Measured, interleaved in one process (round r times every case once, in
order, before round r + 1 starts, so drift hits all cases alike):

  * the sampling launch alone (skge_epoch_sample_ex) per kind: HIP events
    around each of --launches warmed-up launches, median and min/max, and the
    mean of one batch of back-to-back launches between two events;
  * whole epochs of the pair loop (PairLoopRunner) for TransE-L1 and HolE and
    of the logistic loop (LogisticLoopRunner) for HolE, per kind: events
    around one epoch per round, median over the rounds.

--runner pipe times, instead of the three loops above, the pair loop and the
throughput runner of device_runner="pipe" (EpochRunner / HolePipeRunner with
sampler=) side by side for TransE-L1 and HolE, per kind, in the same
interleaved rounds; a pipe line also carries the draw launch's own time
(profile()'s first entry, median of three eager epochs after the timed
rounds).  --hot-ab times the pipelined TransE-L1 runner with TYPED draws on a
small-pool KG (64 relations of 700 triples whose object pools hold two
entities: 350 occurrences each, below the hot-row bar of 4 per batch, 700
with their expected corruptions) with the hot rows chosen by occurrences
only (SKGE_PIPE_HOT_NEG=0) and with the corruption weight (1), interleaved.

One JSON line per case (the rounds' raw times included), appended to --out
when given.  --tree DIR measures another checkout's package instead (its
scikit-kge_amd/ must be built); a tree from before the typed / LCWA samplers
has only today's entry points and gets RANDOM alone, through them -- the
comparison side of the RANDOM gate: run this tool on both trees in
alternating processes on the same box and compare the RANDOM lines with the
spread of the older tree's own repeated runs.

Usage: python tools/bench_samplers.py [--tree DIR] [--label NAME] [--rounds 7]
           [--kinds random,typed,lcwa] [--launches 200] [--runner pairs|pipe] [--hot-ab]
           [--out profiles/samplers/runs.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"random": 0, "typed": 1, "lcwa": 2}


def _events(torch):
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--d", type=int, default=200)
    ap.add_argument("--nb", type=int, default=100)
    ap.add_argument("--kinds", default="random,typed,lcwa",
                    help="sampler kinds measured in this process (their runners are alive "
                         "together)")
    ap.add_argument("--runner", default="pairs", choices=["pairs", "pipe"])
    ap.add_argument("--hot-ab", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, os.path.join(tree, "scikit-kge_amd"))
    sys.path.insert(0, ROOT)
    import torch
    import skge_amd as S
    from skge_amd import _lib as L
    from skge_amd.device import (DeviceKG, EpochRunner, HolePipeRunner, LogisticLoopRunner,
                                 PairLoopRunner)
    from bench import N_ENT, N_REL, make_wn18_kg
    has_ex = "skge_epoch_sample_ex" in L.SIGNATURES
    kinds = {k: KINDS[k] for k in args.kinds.split(",")} if has_ex else {"random": 0}
    label = args.label or ("this" if tree == ROOT else os.path.basename(tree))
    xs = make_wn18_kg()
    T = len(xs)
    sz = (N_ENT, N_ENT, N_REL)
    dev = torch.device("cuda", 0)
    kg = DeviceKG(xs, dev)
    lib = L.lib()
    base = {"tree": label, "entry": "_ex" if has_ex else "plain", "d": args.d, "nb": args.nb,
            "kg": "wn18-shaped uniform (%d, %d, %d)" % (N_ENT, N_REL, T),
            "device": torch.cuda.get_device_name(0)}
    out = open(args.out, "a") if args.out else None

    def emit(**kw):
        s = json.dumps(dict(base, **kw))
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    if args.hot_ab:
        return hot_ab(args, torch, S, DeviceKG, EpochRunner, emit)

    # ---- the sampling launch ----
    rec = torch.empty((T, 4), dtype=torch.int32, device=dev)
    n1 = torch.empty(T, dtype=torch.int32, device=dev)
    ek = torch.zeros(1, dtype=torch.int64, device=dev)
    smps = {k: (kg.sampler(c, N_REL) if has_ex else None) for k, c in kinds.items()}
    st = torch.cuda.current_stream()

    def launch(k):
        a = (L.stream_ptr(st), L.ptr(kg.trip), kg.T, L.ptr(kg.slots), kg.capacity, N_ENT, 1234,
             L.ptr(ek), 100, L.ptr(rec), L.ptr(n1))
        L.check(lib.skge_epoch_sample_ex(*a, smps[k]) if has_ex else lib.skge_epoch_sample(*a),
                "epoch sample")

    per = {k: [] for k in kinds}
    for k in kinds:
        for _ in range(20):
            launch(k)
    torch.cuda.synchronize()
    for _ in range(args.launches):          # interleaved: one launch of every kind per turn
        for k in kinds:
            e0, e1 = _events(torch)
            e0.record(st)
            launch(k)
            e1.record(st)
            e1.synchronize()
            per[k].append(1e3 * e0.elapsed_time(e1))
    for k in kinds:
        e0, e1 = _events(torch)
        e0.record(st)
        for _ in range(args.launches):
            launch(k)
        e1.record(st)
        e1.synchronize()
        found = [int((rec[:, 3] >= 0).sum().item()), int((n1 >= 0).sum().item())]
        emit(what="sample_launch", kind=k, launches=args.launches,
             us_median=round(float(np.median(per[k])), 3), us_min=round(min(per[k]), 3),
             us_max=round(max(per[k]), 3),
             us_back_to_back=round(1e3 * e0.elapsed_time(e1) / args.launches, 3),
             negatives_found=found)

    # ---- whole epochs ----
    def model(name):
        np.random.seed(42)
        if name == "transe_l1":
            m = S.TransE(sz, args.d, l1=True)
            m.add_hyperparam("margin", 2.0)
        else:
            m = S.HolE(sz, args.d)
            m.add_hyperparam("margin", 0.2)
        return m, {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}

    cases = []
    legs = (("pair", "transe_l1"), ("pair", "hole"), ("triple", "hole"))
    if args.runner == "pipe":
        legs = (("pair", "transe_l1"), ("pipe", "transe_l1"), ("pair", "hole"), ("pipe", "hole"))
    for runner, name in legs:
        for k, code in kinds.items():
            m, upd = model(name)
            kw = {"sampler": code} if has_ex else {}
            cls = {"pair": PairLoopRunner, "triple": LogisticLoopRunner,
                   "pipe": EpochRunner if name == "transe_l1" else HolePipeRunner}[runner]
            r = cls(m, upd, kg, args.nb, seed=1234, **kw)
            # (upd stays referenced with its runner: the graph writes its state)
            cases.append((runner, name, k, r, m, [], upd))
    for _, _, _, r, _, _, _ in cases:
        with torch.cuda.stream(r.stream):
            r.run(args.warmup)
        r.synchronize()
    for _ in range(args.rounds):
        for _, _, _, r, _, ms, _ in cases:
            with torch.cuda.stream(r.stream):
                e0, e1 = _events(torch)
                e0.record(r.stream)
                r.run(1)
                e1.record(r.stream)
                r.synchronize()
            ms.append(e0.elapsed_time(e1))
    bad = 0
    for runner, name, k, r, m, ms, _ in cases:
        # (a table that left the finite range is reported, not hidden: the line
        # says so and the tool exits non-zero after the last line)
        nonfinite = {pid: int((~torch.isfinite(p.data)).sum().item()) for pid, p in m.params.items()}
        bad += sum(nonfinite.values())
        total = r.loss_total if runner == "triple" else r.nviol_total
        med = float(np.median(ms))
        extra = {}
        if runner == "pipe":   # the draw launch's own time, from three eager epochs
            draws = []
            for _ in range(3):
                with torch.cuda.stream(r.stream):
                    us, _ = r.profile()
                r.synchronize()
                draws.append(float(us[0]))
            extra = {"kernel": getattr(r, "kernel", "k_hole_pipe"), "hot_rows": r.hot_rows,
                     "draw_us": round(float(np.median(draws)), 2),
                     "draw_share": round(float(np.median(draws)) / (med * 1e3), 4)}
            if name == "transe_l1":
                extra["ent_i8"] = bool(r.ent_i8)
        emit(what="epoch", **extra, runner=runner, model=name, kind=k, ms_median=round(med, 4),
             ms=[round(v, 4) for v in ms], graph_nodes=r.nlaunches, warmup=args.warmup,
             triples_per_s=round(T / (med * 1e-3), 1), nonfinite=nonfinite,
             total=float(total.item()))
    if out:
        out.close()
    if bad:
        raise SystemExit("non-finite parameters after the timed epochs (see the lines)")


def hot_ab(args, torch, S, DeviceKG, EpochRunner, emit):
    from bench import N_ENT
    n_small, per, n_rel = 64, 700, 65
    rs = np.random.RandomState(7)
    xs = []
    for p in range(n_small):        # subjects spread wide, two objects per relation
        subj = rs.choice(N_ENT - 2 * n_small, size=per, replace=False)
        xs += [(int(s), N_ENT - 2 * n_small + 2 * p + (i & 1), p) for i, s in enumerate(subj)]
    seen = set()
    while len(xs) < 141442:         # filler: one broad relation over the other entities
        t = (int(rs.randint(N_ENT - 2 * n_small)), int(rs.randint(N_ENT - 2 * n_small)), n_small)
        if t not in seen:
            seen.add(t)
            xs.append(t)
    kg = DeviceKG(xs, torch.device("cuda", 0))
    cases = []
    for flag in ("0", "1"):
        os.environ["SKGE_PIPE_HOT_NEG"] = flag
        np.random.seed(42)
        m = S.TransE((N_ENT, N_ENT, n_rel), args.d, l1=True)
        m.add_hyperparam("margin", 2.0)
        upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
        r = EpochRunner(m, upd, kg, args.nb, seed=1234, pipelined=True, sampler=KINDS["typed"])
        cases.append((flag, r, m, upd, []))
    os.environ.pop("SKGE_PIPE_HOT_NEG")
    for _, r, _, _, _ in cases:
        r.run(args.warmup)
        r.synchronize()
    for _ in range(args.rounds):
        for _, r, _, _, ms in cases:
            with torch.cuda.stream(r.stream):
                e0, e1 = _events(torch)
                e0.record(r.stream)
                r.run(1)
                e1.record(r.stream)
                r.synchronize()
            ms.append(e0.elapsed_time(e1))
    same = all(torch.equal(cases[0][2].params[pid].data, cases[1][2].params[pid].data)
               for pid in ("E", "R"))
    for flag, r, m, _, ms in cases:
        med = float(np.median(ms))
        emit(what="hot_ab", hot_neg=int(flag), kind="typed", model="transe_l1", kernel=r.kernel,
             ent_i8=bool(r.ent_i8), hot_rows=r.hot_rows, ms_median=round(med, 4),
             ms=[round(v, 4) for v in ms], triples_per_s=round(len(xs) / (med * 1e-3), 1),
             kg="small pools: %d relations x %d triples, two-entity object pools" % (n_small, per),
             params_equal_other_leg=same, total=int(r.nviol_total.item()))


if __name__ == "__main__":
    main()
