"""References for the link-prediction statistics and explicit-triple scores
(tests/test_linkpred_ref.py on the CPU, tests/test_gpu_linkpred.py on the GPU).

Curve statistics are EXACT: Python integers for P, Nneg, 2U and best_correct,
``fractions.Fraction`` for the two areas, an fp32 value for the threshold.

Scores: integer tables (eval_ref.make_int_case's pattern: entries so small
that every fp32 sum the kernels can form is an exact integer, whatever its
order) give the exact score; float tables are compared with the oracle.

The areas' bound
----------------
skge_curve_stats adds a segment's terms t_k = (dTP_k / P) * (prec_k +
prec_k-1) / 2 (all >= 0) in this tree: thread t of part y of Y = parts(nseg)
takes groups 256 y + t + 256 Y j in ascending j, the 256 threads are added by
a binary tree (8 levels), the Y parts one after another.  Each term carries at
most 4 roundings (prec_k and prec_k-1 one each, but their errors do not add
in a sum of positives: the sum has relative error <= 2 u, then the division
dTP / P and the product; the halving is exact), and a term passes through at
most ceil(G / (256 Y)) + 8 + Y additions, G <= n groups.  All terms being
non-negative, the relative error of the sum is at most
    (4 + ceil(n / (256 Y)) + 8 + Y) u (1 + small),   u = 2^-53,
for the average precision likewise (3 roundings per term).  An fma in place
of a product and a sum only removes a rounding.  ``area_rel_bound`` returns
that figure with 1 % for the second-order terms; it is a condition of the
tests that it stays below 1e-12 for every case they run.
"""
import math
from fractions import Fraction

import numpy as np

U53 = 2.0 ** -53


def parts(nseg):
    """k_cs_reduce's parts per segment (csrc/skge_curve.hip cs_parts)."""
    return max(1, min(256, (2048 + nseg - 1) // nseg))


def area_rel_bound(n, nseg):
    y = parts(nseg)
    b = (4 + math.ceil(max(n, 1) / (256.0 * y)) + 8 + y) * U53 * 1.01
    assert b < 1e-12, (n, nseg, b)
    return b


def canon(scores):
    """fp32 scores with -0.0 folded into +0.0."""
    s = np.asarray(scores, dtype=np.float32).copy()
    s[s == 0] = 0.0
    return s


def _tree_sum(terms):
    """Exact sum of Fractions, pairwise: the large denominators appear only
    near the root, which keeps 70001 terms within a second."""
    terms = list(terms) or [Fraction(0)]
    while len(terms) > 1:
        terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i]
                 for i in range(0, len(terms), 2)]
    return terms[0]


def curve_ref(scores, labels):
    """Exact statistics of one segment.  Returns a dict: P, Nneg, twoU,
    best_correct (int), thresh (np.float32), pr_auc, average_precision
    (Fraction, or None where P == 0 or Nneg == 0)."""
    s = canon(scores)
    y = np.asarray(labels) > 0
    assert not np.isnan(s).any()
    n = len(s)
    P = int(y.sum())
    N = n - P
    out = {"P": P, "Nneg": N, "twoU": 0, "best_correct": N, "thresh": np.float32(np.inf),
           "pr_auc": None, "average_precision": None}
    if n == 0:
        return out
    vals, inv = np.unique(s, return_inverse=True)      # ascending
    tp_g = np.bincount(inv, weights=y, minlength=len(vals)).astype(np.int64)[::-1]
    ct_g = np.bincount(inv, minlength=len(vals)).astype(np.int64)[::-1]
    vals = vals[::-1]                                   # descending
    defined = P > 0 and N > 0
    tp = fp = 0
    twoU, best, thr = 0, N, np.float32(np.inf)
    pr_t, ap_t, prec_prev = [], [], Fraction(1)
    for k in range(len(vals)):
        tpk = tp + int(tp_g[k])
        fpk = fp + int(ct_g[k]) - int(tp_g[k])
        twoU += (fpk - fp) * (tpk + tp)
        prec = Fraction(tpk, tpk + fpk)
        if defined and tpk > tp:
            w = Fraction(tpk - tp, P)
            pr_t.append(w * (prec + prec_prev) / 2)
            ap_t.append(w * prec)
        c = tpk + (N - fpk)
        if c > best:                                    # the smallest k among equal maxima
            best, thr = c, np.float32(vals[k])
        tp, fp, prec_prev = tpk, fpk, prec
    out.update({"twoU": twoU, "best_correct": best, "thresh": thr})
    if defined:
        out["pr_auc"], out["average_precision"] = _tree_sum(pr_t), _tree_sum(ap_t)
    return out


def curve_ref_segments(scores, labels, seg, nseg):
    scores, labels = np.asarray(scores), np.asarray(labels)
    if seg is None:
        return [curve_ref(scores, labels)]
    seg = np.asarray(seg)
    order = np.argsort(seg, kind="stable")
    cuts = np.searchsorted(seg[order], np.arange(nseg + 1))
    return [curve_ref(scores[order[cuts[i]:cuts[i + 1]]], labels[order[cuts[i]:cuts[i + 1]]])
            for i in range(nseg)]


def best_correct_brute(scores, labels):
    """max over EVERY threshold rule score >= t (t any score, or +inf) of the
    number of correct predictions, and the largest such t among the maxima."""
    s = canon(scores)
    y = np.asarray(labels) > 0
    best, thr = int((~y).sum()), np.float32(np.inf)
    for t in sorted(set(s.tolist()), reverse=True):
        c = int(((s >= np.float32(t)) == y).sum())
        if c > best:
            best, thr = c, np.float32(t)
    return best, thr


def roc_auc_ref(r):
    return Fraction(r["twoU"], 2 * r["P"] * r["Nneg"])


# ---- curve cases: (name, scores fp32, labels int8) ----
def curve_case(kind, n, seed):
    rs = np.random.RandomState(seed)
    y = (rs.rand(n) < 0.4).astype(np.int8)
    if kind == "equal":
        s = np.full(n, 0.25, dtype=np.float32)
    elif kind == "levels8":
        s = (rs.randint(0, 8, size=n) / 8.0).astype(np.float32)
    elif kind == "distinct":
        s = rs.permutation(n).astype(np.float32) / np.float32(4.0)
    elif kind == "zeros":
        s = rs.choice(np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32), size=n)
    elif kind == "inf":
        s = rs.randn(n).astype(np.float32)
        s[rs.rand(n) < 0.2] = np.inf
        s[rs.rand(n) < 0.2] = -np.inf
    elif kind == "one_label":
        s = rs.randn(n).astype(np.float32)
        y[:] = 1 if seed % 2 else 0
    elif kind == "informative":
        s = (rs.randn(n) + 1.5 * y).astype(np.float32)
    else:
        raise ValueError(kind)
    return s.astype(np.float32), y


CURVE_KINDS = ("equal", "levels8", "distinct", "zeros", "inf", "one_label", "informative")
CURVE_SIZES = (0, 1, 2, 255, 256, 257, 4097, 70001)


def segment_ids(n, nseg, seed):
    """Segment ids with empty segments, single-element segments and, when n
    allows, one segment longer than a scan tile (2048)."""
    rs = np.random.RandomState(seed)
    if nseg == 1:
        return np.zeros(n, dtype=np.int32)
    live = np.arange(0, nseg, 2)                        # odd segments stay empty
    seg = np.empty(n, dtype=np.int32)
    k = min(n, len(live) // 2)
    seg[:k] = live[1:1 + k]                             # one element each
    rest = n - k
    big = rest * 3 // 4
    seg[k:k + big] = live[0]                            # the long segment
    seg[k + big:] = rs.choice(live[1 + k:] if len(live) > 1 + k else live, size=rest - big)
    return seg[rs.permutation(n)] if n else seg


# ---- scores ----
MODELS = ("transe_l1", "transe_l2", "hole", "rescal")
MODEL_CODE = {"transe_l1": 0, "transe_l2": 1, "hole": 2, "rescal": 3}


def int_tables(model, d, N, M, seed):
    """eval_ref.make_int_case's tables: entries in [-3, 3], [-2, 2] from d = 789."""
    rs = np.random.RandomState(seed)
    lim = 3 if 27 * d * d < 2 ** 24 else 2
    assert (lim ** 3) * d * d < 2 ** 24 and (3 * lim) ** 2 * d < 2 ** 24
    E = rs.randint(-lim, lim + 1, size=(N, d)).astype(np.float64)
    shape = (M, d, d) if model == "rescal" else (M, d)
    R = rs.randint(-lim, lim + 1, size=shape).astype(np.float64)
    return E, R


def ccorr_direct(a, b):
    """sum_j a_j b_{(j + k) mod d}, by the definition (one pair)."""
    d = len(a)
    idx = (np.arange(d)[:, None] + np.arange(d)[None, :]) % d      # [j][k]
    return a @ b[idx]


def scores_f64(model, E, R, trip, integer=False):
    """float64 scores of (s, o, p) triples, RESCAL relation by relation.
    integer: the tables are int_tables' -- HolE's correlation (an FFT in
    float64, off by ~1e-11 on integers below 10^4) is rounded to the integer
    it is, so the result is the exact score (test_linkpred_ref checks the FFT
    form against ccorr_direct)."""
    trip = np.asarray(trip, dtype=np.int64).reshape(-1, 3)
    s, o, p = trip[:, 0], trip[:, 1], trip[:, 2]
    if model.startswith("transe"):
        v = E[s] + R[p] - E[o]
        return -np.abs(v).sum(1) if model == "transe_l1" else -(v * v).sum(1)
    if model == "hole":
        d = E.shape[1]
        c = np.fft.irfft(np.conj(np.fft.rfft(E[s], axis=1)) * np.fft.rfft(E[o], axis=1), n=d, axis=1)
        if integer:
            c = np.rint(c)
        return (R[p] * c).sum(1)
    out = np.zeros(len(trip))
    for r in np.unique(p):
        m = p == r
        out[m] = ((E[s[m]] @ R[r]) * E[o[m]]).sum(1)
    return out


def repeated_triples(rs, N, M, n, rel_counts=None):
    """n triples drawn from few entities (rows repeat); rel_counts: exact
    number of triples per relation (sums to n), else uniform relations."""
    ent = rs.randint(0, N, size=max(2, min(N, 1 + n // 3)))
    t = np.empty((n, 3), dtype=np.int32)
    t[:, 0] = rs.choice(ent, size=n)
    t[:, 1] = rs.choice(ent, size=n)
    if rel_counts is None:
        t[:, 2] = rs.randint(0, M, size=n)
    else:
        assert sum(rel_counts) == n and len(rel_counts) == M
        t[:, 2] = rs.permutation(np.repeat(np.arange(M), rel_counts))
    return t
