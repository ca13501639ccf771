"""References for nearest neighbours in embedding space
(csrc/skge_neighbours.hip, skge_amd/neighbours.py).  numpy only: no torch,
no GPU.

The contract (include/skge_hip.h): query i is row rows[i] of the table T
[N, d] (that id is then never returned) or an external vector (nothing is
excluded); sim is the dot product, or the cosine (dot * r_q) * r_j with
r = 1 / sqrt(n2), 0 for a zero row, every step one correctly rounded fp32
operation and every sum a sequential fp32 fma chain.  The result is the k
best eligible rows by descending similarity, then ascending id among exactly
equal values, padded with id -1 and -inf (topk_ref.topk_of_scores).

exact_neighbours      integer-valued tables with every sum below 2^24: the
                      dots and squared norms are exact in int64, fp32 and
                      fp64 alike; for the cosine the same numbers go through
                      np.float32's 1 / sqrt and the contract's two multiplies,
                      which NumPy rounds correctly, so a device result must
                      EQUAL it, ids and values, ties included.
neighbours_envelope   float tables in fp64 with a derived per-pair bound on
                      the fp32 evaluation: which rows a correct kernel must
                      return (forced) and may return (allowed).
chain32               the contract's arithmetic restated in NumPy, to show on
                      the CPU that the bound holds and is not vacuous.
"""
import numpy as np

import topk_ref as T

U32 = 2.0 ** -24          # fp32 unit roundoff
METRICS = ("cosine", "dot")


def _queries(table, vectors, rows):
    """(query vectors, per-query excluded id lists or None)."""
    assert vectors is None or rows is None
    if vectors is not None:
        return np.asarray(vectors), None
    ids = np.arange(len(table)) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    return np.asarray(table)[ids], [np.array([i], dtype=np.int64) for i in ids.tolist()]


# ----------------------------------------------------------------------------
# integer tables: the exact result
# ----------------------------------------------------------------------------

def _int(a):
    a = np.asarray(a)
    i = np.rint(a).astype(np.int64)
    assert (i == a).all()
    return i


def int_scores(table, metric, vectors=None, rows=None):
    """([nq, N] scores, excl): int64 dots, or the float32 cosines of the
    contract (returned as float32)."""
    q, excl = _queries(table, vectors, rows)
    Ti, Qi = _int(table), _int(q)
    dot = Qi @ Ti.T
    n2t, n2q = (Ti * Ti).sum(axis=1), (Qi * Qi).sum(axis=1)
    amax = max((np.abs(Qi) @ np.abs(Ti).T).max(initial=0), n2t.max(initial=0),
               n2q.max(initial=0))
    assert amax < 2 ** 24          # every partial sum is exact in fp32
    if metric == "dot":
        return dot, excl
    assert metric == "cosine"

    def recip(n2):
        n2 = n2.astype(np.float32)
        with np.errstate(divide="ignore"):
            r = np.float32(1.0) / np.sqrt(n2)
        return np.where(n2 == 0, np.float32(0.0), r).astype(np.float32)

    rq, rt = recip(n2q), recip(n2t)
    cos = (dot.astype(np.float32) * rq[:, None]) * rt[None, :]
    assert cos.dtype == np.float32
    return cos, excl


def exact_neighbours(table, metric, k, vectors=None, rows=None):
    """The contract's (ids int64 [nq, k], sims float64 [nq, k]) on an
    integer-valued table."""
    sc, excl = int_scores(table, metric, vectors, rows)
    return T.topk_of_scores(sc.astype(np.float64), k, excl)


# ----------------------------------------------------------------------------
# float tables: fp64 values and the fp32 bound
# ----------------------------------------------------------------------------

def cosines64(table, vectors=None):
    """fp64 cosine of every query (default: every row) with every row; 0
    where either vector is zero."""
    t = np.asarray(table, dtype=np.float64)
    q = t if vectors is None else np.asarray(vectors, dtype=np.float64)
    nt, nq = np.sqrt((t * t).sum(axis=1)), np.sqrt((q * q).sum(axis=1))
    den = nq[:, None] * nt[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == 0, 0.0, (q @ t.T) / den)


def float_scores(table, metric, vectors=None, rows=None):
    """(sc, tau, excl): the fp64 similarities [nq, N] and a bound tau on
    |fp32 result - sc| for the contract's arithmetic, u = 2^-24, barring
    overflow and underflow.

    dot: a sequential fp32 chain of d terms, fused or not, is within
    tau_dot = 2 (d + 2) u A of the exact sum, A = sum |q_k| |t_k| (eval_ref's
    bound, as topk_ref.float_query_scores uses it).

    cosine: the squared norm is such a chain of non-negative terms, so its
    relative error is at most 2 (d + 2) u; the square root halves that and
    adds u, the divide adds u: r_fp32 = r (1 + e), |e| <= (d + 2) u + 2 u =
    (d + 4) u to first order.  The two multiplies add u each, so
    cos_fp32 = dot_fp32 r_q r_j (1 + h) with |h| <= eta = 1.01 (2 (d + 4) +
    2) u -- the 1.01 covers the products of these terms, which are below
    eta^2 < 1e-3 eta for d <= 2^12 -- and
    |cos_fp32 - cos| <= r_q r_j (tau_dot (1 + eta) + |dot| eta)."""
    q, excl = _queries(table, vectors, rows)
    t = np.asarray(table, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    d = t.shape[1]
    dot = q @ t.T
    tau_dot = 2.0 * (d + 2) * U32 * (np.abs(q) @ np.abs(t).T)
    if metric == "dot":
        return dot, tau_dot, excl
    assert metric == "cosine"
    with np.errstate(divide="ignore"):
        rt = 1.0 / np.sqrt((t * t).sum(axis=1))
        rq = 1.0 / np.sqrt((q * q).sum(axis=1))
    rt[~np.isfinite(rt)] = 0.0
    rq[~np.isfinite(rq)] = 0.0
    rr = rq[:, None] * rt[None, :]
    eta = 1.01 * (2 * (d + 4) + 2) * U32
    return dot * rr, rr * (tau_dot * (1.0 + eta) + np.abs(dot) * eta), excl


def envelope_of(sc, tau, k, excl):
    """topk_ref.topk_envelope's masks from given scores and bounds: row j is
    FORCED into query i's result when fewer than k other eligible rows can
    reach it (sc + tau >= sc_j - tau_j), ALLOWED when fewer than k certainly
    beat it (sc - tau > sc_j + tau_j).  Excluded rows are neither."""
    nq, N = sc.shape
    forced = np.zeros((nq, N), dtype=bool)
    allowed = np.zeros((nq, N), dtype=bool)
    for i, ex in enumerate(T._excl_lists(excl, nq)):
        ok = np.ones(N, dtype=bool)
        ok[ex] = False
        lo, hi = (sc[i] - tau[i])[ok], (sc[i] + tau[i])[ok]
        reach = (hi[None, :] >= lo[:, None]).sum(axis=1) - 1      # minus j itself
        beat = (lo[None, :] > hi[:, None]).sum(axis=1)            # never j itself
        forced[i, ok] = reach < k
        allowed[i, ok] = beat < k
    return forced, allowed


def neighbours_envelope(table, metric, k, vectors=None, rows=None):
    """(sc, tau, forced, allowed, excl) for a float table."""
    sc, tau, excl = float_scores(table, metric, vectors, rows)
    forced, allowed = envelope_of(sc, tau, k, excl)
    return sc, tau, forced, allowed, excl


def chain32(table, metric, vectors=None, rows=None):
    """The contract's arithmetic in NumPy, float32 [nq, N]: the sequential
    chain acc = fl32(acc + q_k t_k) over k (the product is exact in fp64, the
    sum is rounded to fp64 and then to fp32: an fma up to a rare double
    rounding, which the bound covers like any sequential evaluation), the
    fp32 1 / sqrt and the two multiplies."""
    q, _ = _queries(table, vectors, rows)
    t = np.asarray(table, dtype=np.float32)
    q = np.asarray(q, dtype=np.float32)

    def chain(a, b):        # a [n, d], b [m, d] -> [n, m]
        acc = np.zeros((len(a), len(b)), dtype=np.float32)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        for kk in range(a.shape[1]):
            acc = (acc.astype(np.float64) + a64[:, kk, None] * b64[None, :, kk]).astype(np.float32)
        return acc

    def norm2(a):
        acc = np.zeros(len(a), dtype=np.float32)
        a64 = a.astype(np.float64)
        for kk in range(a.shape[1]):
            acc = (acc.astype(np.float64) + a64[:, kk] * a64[:, kk]).astype(np.float32)
        return acc

    def recip(n2):
        with np.errstate(divide="ignore"):
            r = np.float32(1.0) / np.sqrt(n2)
        return np.where(n2 == 0, np.float32(0.0), r).astype(np.float32)

    dot = chain(q, t)
    if metric == "dot":
        return dot
    return (dot * recip(norm2(q))[:, None]) * recip(norm2(t))[None, :]


# ----------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------

def make_int_table(N, d, seed, lo=-3, hi=3):
    """Integer values in lo .. hi: sums stay far below 2^24 for d <= 1024."""
    return np.random.RandomState(seed).randint(lo, hi + 1, size=(N, d)).astype(np.float64)


def make_float_table(N, d, seed):
    """A nunif-initialised table (param.init_nunif's range), rounded to fp32."""
    bnd = np.sqrt(6) / np.sqrt(N + d)
    return np.random.RandomState(seed).uniform(-bnd, bnd, size=(N, d)).astype(np.float32)


# the float cases of the GPU tests: (N, d, seed)
FLOAT_CASES = [(300, 50, 501), (300, 200, 502)]
FLOAT_KS = (1, 10, 64)


def float_query_forms(table, seed):
    """The three query forms the float tests ask: every row, some rows (one
    repeated), external vectors (two of them rows of the table)."""
    rs = np.random.RandomState(seed)
    N, d = table.shape
    rows = rs.randint(N, size=40)
    rows[7] = rows[3]
    bnd = np.sqrt(6) / np.sqrt(N + d)
    vec = rs.uniform(-bnd, bnd, size=(33, d)).astype(np.float32)
    vec[0], vec[5] = table[2], table[N - 1]
    return {"all": {}, "rows": {"rows": rows}, "query": {"vectors": vec}}


# ----------------------------------------------------------------------------
# eval-embeddings.py's connected-neighbour tag
# ----------------------------------------------------------------------------

def shared_role_matrix(triples, N):
    """bool [N, N]: j is in incoming_neighbours(i) or outgoing_neighbours(i)
    of eval-embeddings.py's graph of ``triples`` (s, o, p): both objects of a
    common relation, or both subjects of one."""
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    M = int(t[:, 2].max(initial=-1)) + 1
    heads = np.zeros((N, max(M, 1)), dtype=np.int64)
    tails = np.zeros((N, max(M, 1)), dtype=np.int64)
    heads[t[:, 0], t[:, 2]] = 1
    tails[t[:, 1], t[:, 2]] = 1
    return (heads @ heads.T + tails @ tails.T) > 0
