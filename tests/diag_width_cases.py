"""The widths at which the DistMult and ComplEx kernels are compared with
tests/diag_ref.py so that every register layout is reached
(tests/test_gpu_diag_widths.py), as data: a table of (model, d, KM, what) and
the inputs of each case.  In the spirit of width_cases.py.

A row of width d lives in KM = km_for(d) registers per lane, element e in
lane e mod 64 of register e / 64.  k_pair_grad, k_triple_grad and k_score_diag
are instantiated for KM = 1, 2, 3, 4, 8, 16, k_diag_pos for KM = 1 .. 4 (d <=
256, diag_pos_ok).  ComplEx finds a component's other half in lane l ^ 1, which
is right only because d is even and the fill past the row is zero: the widths
66, 130, 194, 258 and 514 end the row one complex component into a register.

Every case carries its own table scale, margin and seed.  They are chosen on
the CPU, by tests/test_diag_width_cases.py, never from a device result:

scale   the largest of SCALES at which the worst-case fp32 error of a score,
        (KM + 10) 2^-24 max_i A_i, stays at or under 5e-6, half the parity bar
        (score_error_bound);
margin  a round number for which between 20% and 80% of the P pairs violate
        in fp64 and no pair's f(n) + margin - f(p) is within 1e-5 of zero;
seed    the first of case_seed + 0, 1, 2 ... for which such a margin exists.
"""
from collections import namedtuple

import numpy as np

import diag_ref as DR
from eval_ref import case_seed
from width_cases import km_for

N, M, P = 300, 7, 200
NSCORE = 500               # random triples of the score comparison
SCALES = (0.5, 0.4, 0.3, 0.25, 0.2, 0.15, 0.1)
MARGINS = (0.05, 0.02, 0.01, 0.1)
ERR_BAR = 5e-6             # half of parity_util's 1e-5
GAP = 1e-5

CLS = {"distmult": "DistMult", "complex": "ComplEx"}
MODEL_CODE = {"distmult": 5, "complex": 6}

# (d, what); loop: the forms of the pair-loop epoch run at this width
_DISTMULT = ((65, "KM 2, one element in the second register"),
             (100, "KM 2"),
             (128, "KM 2, full lanes"),
             (129, "KM 3, one element in the third register"),
             (192, "KM 3, full lanes"),
             (255, "KM 4, the last lane empty"),
             (256, "KM 4, full lanes; the last width of k_diag_pos"),
             (257, "KM 8, one element in the fifth register; past k_diag_pos"),
             (512, "KM 8, full lanes"),
             (513, "KM 16, one element in the ninth register"),
             (1024, "KM 16, full lanes"))
_COMPLEX = ((66, "KM 2, one component in the second register"),
            (100, "KM 2"),
            (128, "KM 2, full lanes"),
            (130, "KM 3, one component in the third register"),
            (192, "KM 3, full lanes"),
            (194, "KM 4, one component in the fourth register"),
            (254, "KM 4, the last component's lanes empty"),
            (256, "KM 4, full lanes; the last width of k_diag_pos"),
            (258, "KM 8, one component in the fifth register; past k_diag_pos"),
            (512, "KM 8, full lanes"),
            (514, "KM 16, one component in the ninth register"),
            (1024, "KM 16, full lanes"))
# pair-loop epochs: k_diag_pos<*, 2>, and both sides of the d <= 256 edge
LOOP_D = {"distmult": (100, 128, 256, 257), "complex": (66, 100, 128, 256, 258)}
DIAG_POS_MAX_D = 256

# (model, d) -> (scale, margin, seed offset): tests/test_diag_width_cases.py
# holds each triple to the rules of the module docstring
_CHOSEN = {
    ("distmult", 65): (0.4, 0.05, 0),
    ("distmult", 100): (0.3, 0.05, 0),
    ("distmult", 128): (0.3, 0.05, 0),
    ("distmult", 129): (0.3, 0.05, 0),
    ("distmult", 192): (0.3, 0.05, 0),
    ("distmult", 255): (0.25, 0.05, 0),
    ("distmult", 256): (0.3, 0.05, 0),
    ("distmult", 257): (0.25, 0.05, 0),
    ("distmult", 512): (0.2, 0.05, 0),
    ("distmult", 513): (0.15, 0.02, 0),
    ("distmult", 1024): (0.15, 0.02, 0),
    ("complex", 66): (0.3, 0.05, 0),
    ("complex", 100): (0.3, 0.05, 0),
    ("complex", 128): (0.3, 0.05, 0),
    ("complex", 130): (0.3, 0.02, 0),
    ("complex", 192): (0.25, 0.05, 0),
    ("complex", 194): (0.2, 0.02, 0),
    ("complex", 254): (0.2, 0.05, 0),
    ("complex", 256): (0.2, 0.02, 0),
    ("complex", 258): (0.2, 0.05, 0),
    ("complex", 512): (0.15, 0.02, 0),
    ("complex", 514): (0.15, 0.02, 0),
    ("complex", 1024): (0.1, 0.01, 1),
}

Case = namedtuple("Case", "id model cls d km what scale margin seed loop")


def _build():
    out = []
    for model, widths in (("distmult", _DISTMULT), ("complex", _COMPLEX)):
        for d, what in widths:
            scale, margin, off = _CHOSEN[model, d]
            out.append(Case("%s-d%d" % (model, d), model, CLS[model], d, km_for(d), what, scale,
                            margin, (case_seed("diag-width", model, d) + off) % (2 ** 31),
                            d in LOOP_D[model]))
    return out


CASES = _build()
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
LOOP_IDS = [c.id for c in CASES if c.loop]


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def tables(c):
    return DR.tables(c.model, N, M, c.d, c.seed, scale=c.scale)


def pairs(c):
    return DR.forced_pairs(N, M, P, c.seed + 1)


def labelled(c):
    """the logistic batch: the pairs' positives (+1), then their negatives (-1)"""
    pos, neg = pairs(c)
    return np.concatenate([pos, neg]), np.concatenate([np.ones(P), -np.ones(P)])


def score_triples(c):
    rs = np.random.RandomState(c.seed + 2)
    return np.stack([rs.randint(N, size=NSCORE), rs.randint(N, size=NSCORE),
                     rs.randint(M, size=NSCORE)], axis=1).astype(np.int32)


def abs_scores(model, E, R, trip):
    """A_i = sum_k |s_k| absprod(|r|, |o|)_k: the sum of the absolute values of
    the terms of triple i's score"""
    trip = np.asarray(trip)
    s, o, p = trip[:, 0], trip[:, 1], trip[:, 2]
    return np.sum(np.abs(E[s]) * DR._abs_prod(model, R[p], E[o]), axis=1)


def score_error_bound(c, E, R):
    """(KM + 10) u max_i A_i over every triple the case scores: KM chained
    fmas per lane, the 6 levels of wave_sum and the products (one rounding for
    DistMult's, a product and an fma for ComplEx's) each carry at most u A_i to
    first order."""
    pos, neg = pairs(c)
    trip = np.concatenate([pos, neg, score_triples(c)])
    return (c.km + 10) * DR.U32 * float(abs_scores(c.model, E, R, trip).max())


def margin_gaps(c, E, R, margin=None):
    """f(n) + margin - f(p) of the P pairs in fp64 (Sigmoid, the models'
    default): positive where the pair violates"""
    from oracle import skge_oracle as O
    pos, neg = pairs(c)
    pf = O.Sigmoid.f(DR.scores(c.model, E, R, pos))
    nf = O.Sigmoid.f(DR.scores(c.model, E, R, neg))
    return nf + (c.margin if margin is None else margin) - pf


def loop_kg(T):
    """T distinct triples over (N, M) with forced duplicates, as
    test_gpu_diag.loop_kg: a hub subject, some s == o, one relation on a third
    of them."""
    rs = np.random.RandomState(17)
    seen, out = set(), []
    while len(out) < T:
        s, o, p = int(rs.randint(N)), int(rs.randint(N)), int(rs.randint(M))
        k = len(out)
        if k % 7 == 0:
            s = 3
        elif k % 11 == 0:
            o = s
        if k % 3 == 0:
            p = 1
        if (s, o, p) not in seen:
            seen.add((s, o, p))
            out.append((s, o, p))
    return np.array(out, dtype=np.int32)


# ---------------------------------------------------------------------------
# the dense KG of the undrawn corruptions: N = 8, M = 2
# ---------------------------------------------------------------------------
DENSE_N, DENSE_M = 8, 2


def dense_kg():
    """Every (s, o=0, p=0), every (s=1, o, p=1) and four other triples.  A
    subject corruption of (s, 0, 0) and an object corruption of (1, o, 1) is
    always a training triple, so no sampler can draw it: the record holds -1
    whatever the seed and the number of tries."""
    t = [(s, 0, 0) for s in range(DENSE_N)] + [(1, o, 1) for o in range(DENSE_N)]
    t += [(2, 3, 0), (4, 5, 1), (6, 7, 0), (3, 3, 1)]
    assert len(set(t)) == len(t)
    return np.array(t, dtype=np.int32)


def undrawn(rec, n1):
    """(records whose s-corruption cannot exist, records whose o-corruption
    cannot exist) as boolean masks over the epoch's records"""
    rec = np.asarray(rec)
    return (rec[:, 1] == 0) & (rec[:, 2] == 0), (rec[:, 0] == 1) & (rec[:, 2] == 1)
