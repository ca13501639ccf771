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
--onen digests the 1-N training entry points instead (onen_digest).
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


ONEN_SHAPES = ((300, 33, 200), (129, 129, 2), (128, 33, 50))   # (N, B, d); M = B


def onen_digest(S, L, digest):
    """--onen: the 1-N training entry points (skge_kvsall_* / skge_onevsall_*)
    for DistMult and ComplEx, label smoothing 0.1, 1vsAll at n3 = 0 and 0.05.
    The queries name every anchor and every relation at most once (M = B, rel a
    permutation, anchors drawn without replacement), so every gradient element
    takes at most one atomic add and the sums have one order: the workspace
    sizes, z, lse, the loss, the gradients, the marked relations and the tables
    after an SGD and an AdaGrad step must all keep their bits."""
    import numpy as np
    import torch
    from skge_amd.kvsall import KvsAllQueries
    from skge_amd.onevsall import OneVsAllQueries
    for cls in (S.DistMult, S.ComplEx):
        for N, B, d in ONEN_SHAPES:
            rs = np.random.RandomState(7 * N + B + d)
            tables = {pid: rs.uniform(-0.5, 0.5, size=(n, d)).astype(np.float32)
                      for pid, n in (("E", N), ("R", B))}
            anchor = rs.choice(N, B, replace=False).astype(np.int32)
            rel = rs.permutation(B).astype(np.int32)
            dirn = (rs.permutation(B) % 2).astype(np.int32)
            lens = rs.randint(0, min(N, 5) + 1, size=B)
            off = np.zeros(B + 1, dtype=np.int32)
            off[1:] = np.cumsum(lens)
            ans = np.concatenate([np.sort(rs.choice(N, n, replace=False)) for n in lens]
                                 + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
            target = rs.randint(N, size=B).astype(np.int32)
            kv = KvsAllQueries(anchor, rel, dirn, off, ans, N, B)
            ova = OneVsAllQueries(anchor, rel, dirn, target, N, B)

            def model(n3):
                m = cls((N, N, B), d, init="device_nunif")
                for pid in ("E", "R"):
                    m.params[pid].data.copy_(torch.from_numpy(tables[pid]))
                m.add_hyperparam("label_smoothing", 0.1)
                m.add_hyperparam("n3", n3)
                return m

            for regime, q, n3 in (("kvsall", kv, 0.0), ("onevsall", ova, 0.0),
                                  ("onevsall", ova, 0.05)):
                tag = "%s %s N=%d B=%d d=%d n3=%g" % (regime, cls.__name__, N, B, d, n3)
                nbytes = getattr(L.lib(), "skge_%s_workspace_bytes" % regime)(
                    model(n3)._kernel_model(), B, N, B, d)
                digest(tag + " workspace_bytes", np.array([nbytes], dtype=np.int64))
                m = model(n3)
                g = getattr(m, "_%s_gradients" % regime)(q, scores=True)
                digest(tag + " grad gE gR touched loss z",
                       g["E"][0].cpu().numpy(), g["R"][0].cpu().numpy(), g["R"][1].cpu().numpy(),
                       np.array([m.loss], dtype=np.float32), m._score.cpu().numpy())
                if regime == "onevsall":
                    digest(tag + " grad lse", m._lse.cpu().numpy())
                for opt in (S.SGD, S.AdaGrad):
                    m = model(n3)
                    upd = {pid: opt(p, 0.1) for pid, p in m.params.items()}
                    loss = torch.zeros(1, dtype=torch.float32, device=m.device)
                    getattr(m, "_%s_step" % regime)(q, upd, loss)
                    digest("%s step %s E R loss" % (tag, opt.__name__),
                           m.params["E"].data.cpu().numpy(), m.params["R"].data.cpu().numpy(),
                           loss.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--onen", action="store_true",
                    help="digest the 1-N training entry points instead (see onen_digest)")
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

    for name, model, l2 in ([] if args.onen else SCORERS):
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
    if args.onen:
        onen_digest(S, L, digest)
    carrier = S.TransE((4, 4, 2), 4, init="device_nunif")   # the device the tables are put on
    for d in ([] if args.onen else DIMS):
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
