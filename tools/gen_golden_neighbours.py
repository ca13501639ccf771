#!/usr/bin/env python3
"""Nearest-neighbour fixture made by the reference's own eval-embeddings.py:
``cosTheta`` of every pair of rows of a small table, and for a train and a
test graph the relation "j is in incoming_neighbours(i) or in
outgoing_neighbours(i)" that its ``similarity`` tags neighbours with.

Runs ONLY on the development machine: the reference script is imported by
path with importlib (its name has a hyphen).  ``cosineMatrix`` is NOT used:
it fills ``numpy.full((N, N), 2)``, an integer matrix, so every cosine it
stores is truncated to an int; the fixture holds ``cosTheta``'s own values.

Writes tests/golden/neighbours/neighbours_ref.npz (a directory of its own:
the fixtures directly under tests/golden/ are all read as training fixtures):
T (float64 holding fp32 values) [40, 8], train / test triples (s, o, p)
int64, cos float64 [40, 40], role_train / role_test bool [40, 40].  Data only.
Usage:  python tools/gen_golden_neighbours.py [--out tests/golden/neighbours]
"""
import argparse
import importlib.util
import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import REF  # noqa: E402

N_ENT, N_REL, D = 40, 3, 8


def import_eval_embeddings():
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("eval_embeddings",
                                                  os.path.join(REF, "eval-embeddings.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    logging.disable(logging.CRITICAL)
    return mod


def make_kg(seed, n, n_subj, n_obj):
    """n unique triples; entities >= 36 take no part, relation 2 is rare."""
    rs = np.random.RandomState(seed)
    seen, out = set(), []
    while len(out) < n:
        p = int(rs.choice(N_REL, p=[0.5, 0.4, 0.1]))
        t = (int(rs.randint(n_subj)), int(rs.randint(n_obj)), p)
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def role_matrix(mod, triples):
    graph = mod.make_graph(triples, N_ENT, N_REL)
    out = np.zeros((N_ENT, N_ENT), dtype=bool)
    for i in range(N_ENT):
        for j in mod.incoming_neighbours(i, graph) + mod.outgoing_neighbours(i, graph):
            out[i, j] = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "tests", "golden", "neighbours"))
    args = ap.parse_args()
    out = os.path.abspath(args.out)
    mod = import_eval_embeddings()
    T = np.random.RandomState(13).uniform(-1, 1, (N_ENT, D)).astype(np.float32).astype(np.float64)
    T[17] = 2.0 * T[4]          # cosine 1 (up to rounding) with another row
    train = make_kg(5, 45, 20, 36)
    test = make_kg(6, 12, 36, 20)
    cos = np.array([[mod.cosTheta(T[i], T[j]) for j in range(N_ENT)] for i in range(N_ENT)],
                   dtype=np.float64)
    role_train, role_test = role_matrix(mod, train), role_matrix(mod, test)
    for r in (role_train, role_test):
        assert r.any() and not r.all() and (r == r.T).all()
        assert not r[36:].any()                # entities without a role
    assert (role_train != role_test).any()
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "neighbours_ref.npz")
    np.savez_compressed(path, T=T, train=np.array(train, dtype=np.int64),
                        test=np.array(test, dtype=np.int64), cos=cos, role_train=role_train,
                        role_test=role_test)
    print("wrote %s (%d bytes): %d / %d tagged pairs" % (path, os.path.getsize(path),
                                                         role_train.sum(), role_test.sum()))


if __name__ == "__main__":
    main()
