#!/usr/bin/env python3
"""Digests of the evaluation entry points' outputs on fixed-seed float tables.

One line per output buffer: a SHA-256 prefix of the bytes that skge_rank_known,
skge_rank_pools, skge_topk, skge_topk_pools, skge_neighbours, skge_relrank,
skge_reltopk and skge_subgraph_rank return (through the package's facade) for
TransE, TransE with squared-L2 scoring, HolE and RESCAL at d = 33, 64 and 200
(700 entities, 40 relations, 150 test triples).  Run once under each of two
builds of the library (SKGE_LIB_PATH picks one, tools/build_rev.sh builds a
revision's) and compare the two outputs line for line: a refactor of the
kernels must not move a bit.  Prints to stdout; --out FILE also writes there.
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scikit-kge_amd")]

N, M, NQ = 700, 40, 150
DIMS = (33, 64, 200)
SCORERS = [("transe", "transe", False), ("transe-l2", "transe", True), ("hole", "hole", False),
           ("rescal", "rescal", False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import skge_amd as S
    from skge_amd import _lib as L
    L.require_gpu()
    lines = []

    def digest(tag, *arrays):
        for i, a in enumerate(arrays):
            a = np.ascontiguousarray(a)
            lines.append("%s[%d] %s %s %s" % (tag, i, a.dtype, "x".join(map(str, a.shape)),
                                             hashlib.sha256(a.tobytes()).hexdigest()[:16]))

    for name, model, l2 in SCORERS:
        for d in DIMS:
            rs = np.random.RandomState(1000 * d + len(name))
            cls = {"transe": S.TransE, "hole": S.HolE, "rescal": S.RESCAL}[model]
            m = cls((N, N, M), d, init="device_nunif", **({"l1": False} if l2 else {}))
            for pid in ("E", "W" if model == "rescal" else "R"):
                shape = tuple(m.params[pid].shape)
                bnd = np.sqrt(6.0 / (shape[0] + shape[1]))
                m.params[pid].data.copy_(torch.from_numpy(
                    rs.uniform(-bnd, bnd, size=shape).astype(np.float32)))
            test = np.stack([rs.randint(N, size=NQ), rs.randint(N, size=NQ),
                             rs.randint(M, size=NQ)], axis=1)
            pick = test[rs.randint(NQ, size=8 * NQ)]
            known = np.concatenate([
                test, np.stack([pick[:, 0], rs.randint(N, size=len(pick)), pick[:, 2]], axis=1),
                np.stack([rs.randint(N, size=len(pick)), pick[:, 1], pick[:, 2]], axis=1),
                np.stack([pick[:, 0], pick[:, 1], rs.randint(M, size=len(pick))], axis=1)])
            known = sorted(set(tuple(t) for t in known.tolist()))
            tests = [tuple(t) for t in test.tolist()]
            pools = [np.sort(rs.choice(N, n, replace=False)) for n in (500, 130, 7)]
            qpool = rs.randint(-1, len(pools), size=NQ)
            tag = "%s d=%d" % (name, d)
            lp = S.LinkPredictor(m, known, scoring="model" if l2 else "eval")
            for k in (10, 100):
                for fn, anchor in ((lp.tails, test[:, 0]), (lp.heads, test[:, 1])):
                    digest("%s topk %s k=%d" % (tag, fn.__name__, k),
                           *fn(anchor, test[:, 2], k=k))
                    digest("%s topk_pools %s k=%d" % (tag, fn.__name__, k),
                           *fn(anchor, test[:, 2], k=k, candidates=(pools, qpool)))
                digest("%s reltopk k=%d" % (tag, k),
                       *lp.relations(test[:, 0], test[:, 1], k=min(k, M + 5)))
            if l2:
                continue   # the ranking entry points score both TransE codes as L1
            ev = S.FilteredRankingEval(tests, known)
            digest(tag + " rank_known", ev.ranks(m))
            digest(tag + " rank_pools", ev.candidate_ranks(m, pools, qpool, qpool[::-1]))
            digest(tag + " relrank", ev.relation_ranks(m))
            sg = S.Subgraphs.from_triples(known, 2)
            for dist in ("avg", "var"):
                digest("%s subgraph_rank %s" % (tag, dist),
                       *S.SubgraphRankingEval(tests, sg).ranks(m, dist))
    carrier = S.TransE((4, 4, 2), 4, init="device_nunif")   # the device the tables are put on
    for d in DIMS:
        table = np.random.RandomState(77 + d).uniform(-1, 1, size=(N, d)).astype(np.float32)
        for metric in ("cosine", "dot"):
            nn = S.Neighbours(carrier, table=table, metric=metric)
            for k in (10, 20, 100):
                digest("neighbours %s d=%d k=%d" % (metric, d, k),
                       *nn.topk(k=k, rows=np.arange(2 * NQ)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
