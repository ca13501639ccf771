#!/usr/bin/env python3
"""Subgraph fixture made by the reference's own Experiment.make_subgraphs
(skge/base.py:122-202), as subgraphs_create calls it (skge/base.py:392-399):
once over the triples sorted by (p, s) for SUBTYPE.SPO, once sorted by (p, o)
for SUBTYPE.POS, sub_algo "transe", for mincard 0 and 2.

Runs ONLY in the build container (imports the reference with the shims of
tools/gen_golden.py).  The Experiment is made without its argument parser and
given a stand-in ``args`` (ncomp) and a stand-in model (E).

Writes tests/golden/subgraphs/subgraphs_transe.npz (a directory of its own:
the fixtures directly under tests/golden/ are all read as training fixtures):
E (float64 holding fp32 values), the triples, and per mincard m the reference's avg_embeddings (m<m>_avg),
var_embeddings (m<m>_var) and Metadata (m<m>_kind 0 SPO / 1 POS, _ent, _rel,
_size, and the members as _mem_off / _mem_ent).  Data only.

The reference's loop closes its LAST group after the loop, and there takes
that group's variance around the previous kept group's ``mean``
(base.py:188-197).  The KG is built so that, for mincard 2, the last group of
both sort orders has count <= mincard (never kept) while earlier groups are
kept: asserted below.  For mincard 0 every group is kept, the last one too,
so the branch cannot be avoided: m0_stale lists the two subgraph ids (the
last SPO and the last POS) whose var rows come from that branch.
Usage:  python tools/gen_golden_subgraphs.py [--out tests/golden/subgraphs]
"""
import argparse
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import import_reference  # noqa: E402

N_ENT, N_REL, D = 48, 4, 8


def make_kg():
    """Unique triples over entities 0 .. 39 with group sizes from 1 up, plus
    (47, 5, 3) and (6, 46, 3): the last groups of the (p, s) and the (p, o)
    order, one member each."""
    rs = np.random.RandomState(7)
    seen, out = set(), []
    while len(out) < 90:
        # few subjects per relation, so that some groups reach 3 and more
        t = (int(rs.randint(12)), int(rs.randint(40)), int(rs.randint(N_REL)))
        if t not in seen:
            seen.add(t)
            out.append(t)
    out += [(47, 5, 3), (6, 46, 3)]
    rs.shuffle(out)
    return [tuple(t) for t in out]


def run_reference(R, E, triples, mincard):
    exp = object.__new__(R.base.Experiment)
    exp.args = types.SimpleNamespace(ncomp=D)
    exp.subgraphs = R.base.Subgraphs()
    exp.avg_embeddings = []
    exp.var_embeddings = []
    model = types.SimpleNamespace(E=E)
    T = R.base.SUBTYPE
    exp.make_subgraphs(T.SPO, sorted(triples, key=lambda l: (l[2], l[0])), mincard, model,
                       "transe")
    exp.make_subgraphs(T.POS, sorted(triples, key=lambda l: (l[2], l[1])), mincard, model,
                       "transe")
    subs = exp.subgraphs.subgraphs
    assert len(subs) == exp.subgraphs.get_Nsubgraphs() == len(exp.avg_embeddings)
    return {
        "avg": np.array(exp.avg_embeddings, dtype=np.float64),
        "var": np.array(exp.var_embeddings, dtype=np.float64),
        "kind": np.array([0 if m.subType == T.SPO else 1 for m in subs], dtype=np.int64),
        "ent": np.array([m.ent for m in subs], dtype=np.int64),
        "rel": np.array([m.rel for m in subs], dtype=np.int64),
        "size": np.array([m.size for m in subs], dtype=np.int64),
        "mem_off": np.concatenate([[0], np.cumsum([len(m.entities) for m in subs])]).astype(
            np.int64),
        "mem_ent": np.array([e for m in subs for e in m.entities], dtype=np.int64),
    }


def last_group_count(triples, col):
    last = max((t[2], t[col]) for t in triples)
    return sum(1 for t in triples if (t[2], t[col]) == last)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "tests", "golden", "subgraphs"))
    args = ap.parse_args()
    out = os.path.abspath(args.out)
    R = import_reference()
    triples = make_kg()
    assert max(max(t[0], t[1]) for t in triples) < N_ENT <= 64
    E = np.random.RandomState(11).uniform(-1, 1, (N_ENT, D)).astype(np.float32).astype(np.float64)
    res = {}
    os.chdir(tempfile.mkdtemp())    # make_subgraphs writes a log into the cwd
    for mincard in (0, 2):
        r = run_reference(R, E, triples, mincard)
        for k, v in r.items():
            res["m%d_%s" % (mincard, k)] = v
        kinds = r["kind"]
        assert (kinds == 0).any() and (kinds == 1).any()      # groups of both kinds are kept
        if mincard == 2:
            # the stale-`mean` tail branch must not have run
            assert last_group_count(triples, 0) <= mincard
            assert last_group_count(triples, 1) <= mincard
    sizes0 = set(res["m0_size"].tolist())
    assert {1, 2, 3} <= sizes0, sizes0        # both sides of count > 2 and of count > mincard
    assert 3 in set(res["m2_size"].tolist())
    n_spo = int((res["m0_kind"] == 0).sum())
    res["m0_stale"] = np.array([n_spo - 1, len(res["m0_kind"]) - 1], dtype=np.int64)
    path = os.path.join(out, "subgraphs_transe.npz")
    np.savez_compressed(path, E=E, triples=np.array(triples, dtype=np.int64), **res)
    print("wrote %s (%d bytes): %d / %d subgraphs" % (path, os.path.getsize(path),
                                                       len(res["m0_kind"]), len(res["m2_kind"])))


if __name__ == "__main__":
    main()
