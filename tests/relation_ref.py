"""References for relation prediction (csrc/skge_relation.hip,
FilteredRankingEval.relation_ranks, LinkPredictor.relations).

numpy only: no torch, no GPU.  Every relation j of 0 .. M - 1 is scored for a
pair (s, o): TransE -sum|E_s + R_j - E_o|, HolE R_j . ccorr(E_s, E_o), RESCAL
E_s W_j E_o.  The rules are the project's: a position is 1 + the number of
relations scoring strictly higher than the true one; the filtered position
skips every p' != p with (s, o, p') known; a top-k list is ordered by
descending score, then ascending id, and padded with (-1, -inf).

exact_relation_ranks / exact_relation_topk
    integer-valued tables scored in int64.  With eval_ref.make_int_case's
    ranges (entries in [-3, 3], [-2, 2] from d = 789) every partial sum of
    every model's score, in any order, is an integer below 2^24, so fp32, fp64
    and int64 agree bit for bit and a device result must EQUAL the reference.
relation_rank_envelope
    float tables: the interval [lo, hi] of ranks a correct fp32 kernel may
    return (derivation in its docstring).
"""
import numpy as np

import eval_ref as X
import topk_ref as T
from oracle.skge_oracle import hole_scores, rescal_scores, transe_scores

MODELS = ("transe", "hole", "rescal")
_ORACLE = {"transe": transe_scores, "hole": hole_scores, "rescal": rescal_scores}


# ----------------------------------------------------------------------------
# scores
# ----------------------------------------------------------------------------

def oracle_relation_scores(model, E, R, s, o, **kw):
    """[M] float64: the oracle's score of (s, o, j) for every relation j."""
    M = np.asarray(R).shape[0]
    trip = np.stack([np.full(M, s), np.full(M, o), np.arange(M)], axis=1)
    return _ORACLE[model](np.asarray(E, dtype=np.float64), np.asarray(R, dtype=np.float64), trip,
                          **kw)


def int_relation_scores(model, E, R, pairs, l2=False):
    """[n, M] int64 scores of every relation for the pairs (s, o) on
    integer-valued tables (direct sums, no FFT)."""
    Ei, Ri = X._int_tables(E, R)
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    es, eo = Ei[pr[:, 0]], Ei[pr[:, 1]]
    n, d = es.shape
    M = Ri.shape[0]
    if model == "transe":
        q = eo - es
        out = np.zeros((n, M), dtype=np.int64)
        step = max(1, X._CHUNK_ELEMS // (M * d))
        for i0 in range(0, n, step):
            diff = q[i0:i0 + step, None, :] - Ri[None, :, :]
            out[i0:i0 + step] = -(diff * diff).sum(axis=2) if l2 else -np.abs(diff).sum(axis=2)
        return out
    if model == "hole":
        # ccorr(E_s, E_o)_k = sum_j E_s[j] E_o[(j + k) mod d]
        k, j = np.arange(d)[:, None], np.arange(d)[None, :]
        idx = (j + k) % d
        q = np.zeros((n, d), dtype=np.int64)
        step = max(1, X._CHUNK_ELEMS // (d * d))
        for i0 in range(0, n, step):
            q[i0:i0 + step] = np.einsum("nj,nkj->nk", es[i0:i0 + step], eo[i0:i0 + step][:, idx])
        return q @ Ri.T
    if model == "rescal":
        return np.stack([((es @ Ri[j]) * eo).sum(axis=1) for j in range(M)], axis=1)
    if model in ("distmult", "complex"):
        # R_j . (conj(E_s) * E_o)  (diag_ref.q_rel; eval_ref.int_diag_mul's bound)
        return X.int_diag_mul(model, es, eo, True) @ Ri.T
    raise ValueError("unknown model %r" % (model,))


def known_mask(queries, known, M):
    """[nq, M] bool: mask[i, j] = (s_i, o_i, j) is known and j != p_i."""
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    kn = np.asarray(known, dtype=np.int64).reshape(-1, 3)
    big = int(max(q[:, :2].max(initial=0), kn[:, :2].max(initial=0))) + 1
    ukeys, grp = np.unique(q[:, 0] * big + q[:, 1], return_inverse=True)
    kkeys = kn[:, 0] * big + kn[:, 1]
    pos = np.searchsorted(ukeys, kkeys)
    pos[pos == len(ukeys)] = 0
    hit = ukeys[pos] == kkeys
    gmask = np.zeros((len(ukeys), M), dtype=bool)
    gmask[pos[hit], kn[hit, 2]] = True
    mask = gmask[grp.reshape(-1)]
    mask[np.arange(len(q)), q[:, 2]] = False
    return mask


def known_relations(queries, known, M=None):
    """Per query (s, o, p) the ascending ids p' != p with (s, o, p') known."""
    if M is None:
        M = int(np.asarray(known).reshape(-1, 3)[:, 2].max()) + 1
    return [np.flatnonzero(row) for row in known_mask(queries, known, M)]


def pair_relations(pairs, known):
    """Per pair (s, o) the ascending ids of every known relation."""
    rels = {}
    for s, o, p in np.asarray(known).reshape(-1, 3).tolist():
        rels.setdefault((s, o), set()).add(p)
    return [np.array(sorted(rels.get((s, o), ())), dtype=np.int64)
            for s, o in np.asarray(pairs).reshape(-1, 2).tolist()]


def ranks_of_scores(sc, queries, known):
    """[nq, 2] int64 (raw, filtered) from a score matrix [nq, M]."""
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    rows = np.arange(len(q))
    higher = sc > sc[rows, q[:, 2]][:, None]
    out = np.zeros((len(q), 2), dtype=np.int64)
    out[:, 0] = 1 + higher.sum(axis=1)
    out[:, 1] = out[:, 0]
    if known is not None:
        out[:, 1] -= (higher & known_mask(q, known, sc.shape[1])).sum(axis=1)
    return out


def exact_relation_ranks(model, E, R, queries, known):
    """[nq, 2] int64 (raw, filtered) for queries (s, o, p) on integer-valued
    tables; known None: no filter."""
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    return ranks_of_scores(int_relation_scores(model, E, R, q[:, :2]), q, known)


def exact_relation_topk(model, E, R, pairs, k, excl=None, l2=False):
    """(ids [nq, k] int64, scores [nq, k] float64): the contract's result on
    integer-valued tables; excl: per pair the relation ids never returned."""
    return T.topk_of_scores(int_relation_scores(model, E, R, pairs, l2), k, excl)


# ----------------------------------------------------------------------------
# the fp32 envelope
# ----------------------------------------------------------------------------

def _abs_relation_scores(model, E, R, s, o):
    """A_j: the score formula on absolute values."""
    aE, aR = np.abs(E), np.abs(R)
    if model == "transe":
        return np.sum(aE[s] + aR + aE[o], axis=1)
    return oracle_relation_scores(model, aE, aR, s, o)


def relation_rank_envelope(model, E, R, queries, known):
    """(lo, hi), each [nq, 2] int64 (raw, filtered): the ranks any correct fp32
    evaluation may return for float tables holding fp32 values.

    Every relation's score sc_j is computed in fp64 (the oracle's *_scores).
    Its fp32 counterpart differs from it by at most

        tau_j = 2 (d + 2) u A_j,      u = 2^-24,

    A_j the same formula on absolute values.  The bound holds for ANY order of
    a d-term fp32 sum nested in a d-term fp32 sum: a d-term sum carries at most
    (d - 1) u sum|t| to first order whatever the order of its adds (each add
    rounds a partial sum that is itself bounded by sum|t|); each term of the
    outer sum is a product (one rounding, u) with an inner d-term sum of
    rounded products ((d - 1) u + u), so the nested sum carries at most
    (2 d + 1) u A_j to first order -- RESCAL's reduction over b may take any
    order, and HolE's correlation and dot are such a nest.  TransE has one
    rounded subtract for q, one for q - R_j, and a d-term sum: (d + 1) u A_j.
    The remaining 3 u A_j and more covers the second-order terms (d^2 u^2 A_j,
    below 4 u A_j for d <= 1024).  So relation j certainly outscores the true
    relation t when sc_j - sc_t > tau_j + tau_t and certainly does not when
    sc_j - sc_t < -(tau_j + tau_t):

        lo = 1 + #{j : sc_j - sc_t > tau_j + tau_t}
        hi = 1 + #{j != t : sc_j - sc_t >= -(tau_j + tau_t)}

    and the filtered bounds are the same counts over the relations that are
    not filtered out (as eval_ref.rank_envelope computes its own)."""
    E = np.asarray(E, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    d = E.shape[1]
    M = R.shape[0]
    q = np.asarray(queries).reshape(-1, 3)
    kr = known_relations(q, known, M)
    lo = np.zeros((len(q), 2), dtype=np.int64)
    hi = np.zeros((len(q), 2), dtype=np.int64)
    rel = np.arange(M)
    for i, (s, o, p) in enumerate(q.tolist()):
        sc = oracle_relation_scores(model, E, R, s, o)
        tau = 2.0 * (d + 2) * X.U32 * _abs_relation_scores(model, E, R, s, o)
        diff = sc - sc[p]
        slack = tau + tau[p]
        above = diff > slack
        maybe = (diff >= -slack) & (rel != p)
        filt = np.zeros(M, dtype=bool)
        filt[kr[i]] = True
        lo[i] = 1 + above.sum(), 1 + (above & ~filt).sum()
        hi[i] = 1 + maybe.sum(), 1 + (maybe & ~filt).sum()
    return lo, hi


# ----------------------------------------------------------------------------
# seeded cases
# ----------------------------------------------------------------------------

def relation_triples(rs, N, M, nq):
    """nq test triples and a known set holding them plus, for three in four of
    the test triples, (s, o, p') for a random half of the other relations."""
    test = np.stack([rs.randint(N, size=nq), rs.randint(N, size=nq), rs.randint(M, size=nq)],
                    axis=1).astype(np.int32)
    dense = rs.rand(nq) < 0.75
    extra = rs.rand(nq, M) < 0.5
    extra &= dense[:, None]
    extra[np.arange(nq), test[:, 2]] = False
    qi, pj = np.nonzero(extra)
    more = np.stack([test[qi, 0], test[qi, 1], pj], axis=1)
    both = np.concatenate([test, more]).astype(np.int64)
    key = np.unique((both[:, 0] * N + both[:, 1]) * M + both[:, 2])     # sorted, as rows
    known = np.stack([key // M // N, key // M % N, key % M], axis=1).astype(np.int32)
    return test, known


def make_int_case(model, d, N, M, nq, seed):
    """Integer tables in eval_ref.make_int_case's ranges; test and known
    triples from relation_triples."""
    rs = np.random.RandomState(seed)
    lim = 3 if 27 * d * d < 2 ** 24 else 2
    assert (lim * lim * lim) * d * d < 2 ** 24
    E = rs.randint(-lim, lim + 1, size=(N, d)).astype(np.float64)
    R = rs.randint(-lim, lim + 1, size=X.rel_shape(model, M, d)).astype(np.float64)
    test, known = relation_triples(rs, N, M, nq)
    return E, R, test, known


def make_float_case(model, d, scale, seed, N=300, M=40, nq=120):
    """fp32 tables at init scale times `scale` (eval_ref.make_float_case's
    draw), widened to float64."""
    rs = np.random.RandomState(seed)

    def unif(shape):
        bnd = scale * np.sqrt(6.0) / np.sqrt(shape[0] + shape[1])
        return rs.uniform(-bnd, bnd, size=shape).astype(np.float32).astype(np.float64)
    E = unif((N, d))
    R = unif(X.rel_shape(model, M, d))
    test, known = relation_triples(rs, N, M, nq)
    return E, R, test, known


# (d, N, M, nq): every edge of the new code at least once per model -- d < 4,
# the scalar tail (d & 3), the 32-dim chunk and 32-column tile boundaries
# (31 / 32 / 33, 64 / 65: waves of the RESCAL kernel without a column), a
# ragged second 128-column pass of W_j (d = 130), eight full ones at d = 1024;
# M = 1, 2, around the 64-lane row pass and the 128-row tile, 300; nq at the
# RESCAL query blocks (32 / 64 / 128) and the 64-vector counting block;
# nq = 2048 with M = 129: two relations per RESCAL workgroup, the last group
# with one
_COMMON = [(1, 50, 1, 31), (3, 50, 2, 1), (31, 50, 63, 32), (32, 50, 64, 33), (33, 50, 65, 64),
           (64, 50, 127, 65), (65, 50, 128, 31), (5, 50, 129, 2048), (7, 50, 300, 33),
           (130, 40, 4, 33), (1024, 40, 3, 33)]
# TransE / HolE: ragged multi-tile relation slices (64 query blocks, 36 tiles,
# 2 per slice, 18 slices); the query kernel's grid-stride loop (more than
# 2 x 16384 pairs)
_VECTOR = [(8, 60, 4500, 4096), (4, 130, 5, 65600)]
INT_CASES = [(m,) + c for m in MODELS for c in _COMMON] + \
            [(m,) + c for m in ("transe", "hole") for c in _VECTOR]

# (model, d, scale): N = 300, M = 40, 120 queries
FLOAT_CASES = [(m, d, sc) for m, d in (("transe", 40), ("hole", 33), ("rescal", 37))
               for sc in (1.0, 8.0)]

# seeds: eval_ref.case_seed of the case, with a salt where the plain seed's
# case misses tests/test_relation_ref.py's non-vacuity conditions
_SALT = {}


def int_case(model, d, N, M, nq):
    return make_int_case(model, d, N, M, nq,
                         X.case_seed("rel", model, d, N, M, nq, _SALT.get((model, d, N, M, nq), 0)))


def float_case(model, d, scale):
    return make_float_case(model, d, scale,
                           X.case_seed("rel", model, d, scale, _SALT.get((model, d, scale), 0)))
