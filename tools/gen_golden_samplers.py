#!/usr/bin/env python3
"""Generate the host samplers' golden fixtures from the scikit-kge reference.

Runs only where the reference tree is (tools/gen_golden.py's REF, or
--reference): it loads the reference's skge/sample.py unmodified, by path (the
module imports nothing but copy, collections and numpy.random), and records
what LCWASampler and CorruptedSampler return for one pass over a small KG
from a seeded numpy global RNG.

  * KG: 40 entities, 3 relations, 80 distinct triples (RandomState(7));
    relation 2 has two subjects and ten objects only, so its LCWA mode-0
    draws are mostly rejected, and where an object is known with both
    subjects no s-corruption exists (the sampler returns None for it after
    ntries draws).
  * LCWASampler(1, [0, 1], xs, sz): constructed as the reference does.
  * CorruptedSampler: its constructor calls Sampler.__init__(n) without
    ``modes`` and raises, so the object is made with object.__new__ and given
    the attributes the constructor would set (n, modes = [0, 1], ntries = 100,
    xs, type_index = type_index(xs)).
  * np.random.seed(42), then ``sample(xys)`` once over all triples.

Output: tests/golden/samplers/sampler_{lcwa,corrupted}.npz -- inputs and
recorded outputs only, no code (a directory of their own: every *.npz directly
under tests/golden/ is a training fixture to tests/golden_util.py).
type_index(xs) builds its lists from sets; the fixture stores the lists as
the reference returned them (CSR over 2 * n_rel lists), so the test feeds the
facade the same order.

Usage:  python tools/gen_golden_samplers.py [--reference DIR]
                                           [--out tests/golden/samplers]
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

N_ENT, N_REL, T = 40, 3, 80


def make_kg():
    rs = np.random.RandomState(7)
    seen, out = set(), []
    while len(out) < T:
        p = int(rs.randint(N_REL))
        s = int(rs.randint(2)) if p == 2 else int(rs.randint(N_ENT))
        t = (s, int(rs.randint(10 if p == 2 else N_ENT)), p)
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def load_reference_sample(ref):
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("reference_skge_sample",
                                                  os.path.join(ref, "skge", "sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def index_csr(index):
    off, ent = [0], []
    for p in range(N_REL):
        for side in (0, 1):
            ent += [int(v) for v in index.get(p, {0: [], 1: []})[side]]
            off.append(len(ent))
    return np.asarray(off, dtype=np.int64), np.asarray(ent, dtype=np.int64)


def record(sampler, xs):
    xys = list(zip(xs, [1.0] * len(xs)))
    np.random.seed(42)
    res = sampler.sample(xys)
    return (np.asarray([t for t, _ in res], dtype=np.int64).reshape(-1, 3),
            np.asarray([y for _, y in res], dtype=np.float64))


def main():
    from gen_golden import REF
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=REF)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "tests", "golden",
                                                  "samplers"))
    a = ap.parse_args()
    R = load_reference_sample(a.reference)
    xs = make_kg()
    sz = (N_ENT, N_ENT, N_REL)
    common = dict(xs=np.asarray(xs, dtype=np.int64), sz=np.asarray(sz, dtype=np.int64), seed=42)

    neg, ys = record(R.LCWASampler(1, [0, 1], xs, sz), xs)
    np.savez(os.path.join(a.out, "sampler_lcwa.npz"), neg=neg, ys=ys, **common)
    print("lcwa: %d negatives of %d draws" % (len(neg), 2 * len(xs)))

    index = R.type_index(xs)
    c = object.__new__(R.CorruptedSampler)
    c.n, c.modes, c.ntries = 1, [0, 1], 100
    c.xs, c.type_index = set(xs), index
    neg, ys = record(c, xs)
    off, ent = index_csr(index)
    np.savez(os.path.join(a.out, "sampler_corrupted.npz"), neg=neg, ys=ys, index_off=off,
             index_ent=ent, **common)
    print("corrupted: %d negatives of %d draws" % (len(neg), 2 * len(xs)))


if __name__ == "__main__":
    main()
