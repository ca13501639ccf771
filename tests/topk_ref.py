"""References for top-k link prediction (csrc/skge_topk.hip,
skge_amd/predict.py).  numpy only: no torch, no GPU.

The contract: a query is (anchor a, relation p) and a direction -- 'tail'
scores every entity j as the object of (a, p, j), 'head' as the subject of
(j, p, a) -- with the evaluators' scores (oracle.entity_scores; squared L2
for TransE under l2=True).  The result is the k best entities not on the
query's exclusion list, by descending score, then ascending id among exactly
equal scores, padded with id -1 and score -inf.

exact_topk      integer-valued tables scored in int64 (eval_ref's argument:
                fp32, fp64 and int64 agree bit for bit), so a device result
                must EQUAL it, ids and scores, ties included.
topk_envelope   float tables scored in fp64 with eval_ref's derived bound
                tau_j on any sequential fp32 evaluation: which entities a
                correct kernel must return (forced) and may return (allowed).
"""
import numpy as np

import eval_ref as X
from oracle import skge_oracle as O

DIRECTIONS = ("tail", "head")


def _queries(queries):
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 2)
    return q[:, 0], q[:, 1]


def _excl_lists(excl, n):
    if excl is None:
        return [np.zeros(0, dtype=np.int64)] * n
    assert len(excl) == n
    return [np.asarray(e, dtype=np.int64).reshape(-1) for e in excl]


def known_answers(queries, known, direction):
    """Per query (a, p) its known answers: every o with (a, o, p) known
    ('tail'), every s with (s, a, p) known ('head'); sorted id arrays."""
    kn = np.asarray(known, dtype=np.int64).reshape(-1, 3)
    fix, var = (kn[:, 0], kn[:, 1]) if direction == "tail" else (kn[:, 1], kn[:, 0])
    table = {}
    for f, v, p in zip(fix.tolist(), var.tolist(), kn[:, 2].tolist()):
        table.setdefault((f, p), set()).add(v)
    a, p = _queries(queries)
    return [np.array(sorted(table.get(key, ())), dtype=np.int64)
            for key in zip(a.tolist(), p.tolist())]


# ----------------------------------------------------------------------------
# integer tables: the exact result
# ----------------------------------------------------------------------------

def int_query_scores(model, E, R, queries, direction, l2=False):
    """[nq, N] int64 scores of every entity under every query."""
    Ei, Ri = X._int_tables(E, R)
    a, p = _queries(queries)
    N, d = Ei.shape
    per = N * d if model == "transe" else max(N, d * d)
    step = max(1, X._CHUNK_ELEMS // per)
    out = np.zeros((len(a), N), dtype=np.int64)
    for i0 in range(0, len(a), step):
        sl = slice(i0, i0 + step)
        if l2:
            assert model == "transe"
            q = X._int_query_vectors(model, Ei, Ri, a[sl], a[sl], p[sl], direction)
            out[sl] = -((q[:, None, :] - Ei[None, :, :]) ** 2).sum(axis=2)
        else:
            out[sl] = X._int_scores_batch(model, Ei, Ri, a[sl], a[sl], p[sl], direction)
    return out


def topk_of_scores(scores, k, excl=None):
    """(ids [nq, k] int64, scores [nq, k] float64) from a score matrix: a
    stable sort of the eligible entities on (-score, id), padded with -1 and
    -inf."""
    scores = np.asarray(scores)
    nq, N = scores.shape
    ids = np.full((nq, k), -1, dtype=np.int64)
    out = np.full((nq, k), -np.inf)
    for i, ex in enumerate(_excl_lists(excl, nq)):
        ok = np.ones(N, dtype=bool)
        ok[ex] = False
        cand = np.flatnonzero(ok)                      # ascending ids
        order = cand[np.argsort(-scores[i, cand], kind="stable")][:k]
        ids[i, :len(order)] = order
        out[i, :len(order)] = scores[i, order]
    return ids, out


def exact_topk(model, E, R, queries, direction, k, excl, l2=False):
    """The contract's result on integer-valued tables."""
    return topk_of_scores(int_query_scores(model, E, R, queries, direction, l2), k, excl)


# ----------------------------------------------------------------------------
# float tables: the fp32 envelope
# ----------------------------------------------------------------------------

def float_query_scores(model, E, R, queries, direction, l2=False):
    """(sc, tau), each [nq, N] float64: the fp64 scores and eval_ref's bound
    tau_j = 2 (d + 2) 2^-24 A_j on a sequential fp32 evaluation's error, A_j
    the scoring formula on absolute values (for squared L2: the same sum of
    absolute values, squared termwise)."""
    E = np.asarray(E, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    N, d = E.shape
    a, p = _queries(queries)
    sc = np.zeros((len(a), N))
    A = np.zeros((len(a), N))
    for i, (ai, pi) in enumerate(zip(a.tolist(), p.tolist())):
        if l2:
            assert model == "transe"
            q = E[ai] + R[pi] if direction == "tail" else E[ai] - R[pi]
            sc[i] = -np.sum((q - E) ** 2, axis=1)
            A[i] = np.sum((np.abs(E[ai]) + np.abs(R[pi]) + np.abs(E)) ** 2, axis=1)
        else:
            sc[i] = O.entity_scores(model, E, R, ai, ai, pi, direction)
            A[i] = X._abs_scores(model, E, R, ai, ai, pi, direction)
    return sc, 2.0 * (d + 2) * X.U32 * A


def topk_envelope(model, E, R, queries, direction, k, excl, l2=False):
    """(sc, tau, forced, allowed): fp64 scores and bounds [nq, N], and two
    bool masks [nq, N].  With every fp32 score within tau_j of sc_j, entity j
    is FORCED into the result when fewer than k other eligible entities i can
    reach it (sc_i + tau_i >= sc_j - tau_j), and ALLOWED in it when fewer than
    k other eligible i certainly beat it (sc_i - tau_i > sc_j + tau_j).
    Excluded entities are neither."""
    sc, tau = float_query_scores(model, E, R, queries, direction, l2)
    nq, N = sc.shape
    forced = np.zeros((nq, N), dtype=bool)
    allowed = np.zeros((nq, N), dtype=bool)
    for i, ex in enumerate(_excl_lists(excl, nq)):
        ok = np.ones(N, dtype=bool)
        ok[ex] = False
        lo, hi = (sc[i] - tau[i])[ok], (sc[i] + tau[i])[ok]
        reach = (hi[None, :] >= lo[:, None]).sum(axis=1) - 1      # minus j itself
        beat = (lo[None, :] > hi[:, None]).sum(axis=1)            # never j itself
        forced[i, ok] = reach < k
        allowed[i, ok] = beat < k
    return sc, tau, forced, allowed
