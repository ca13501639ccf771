"""References for filtered ranking (csrc/skge_eval.hip, skge_amd/eval.py).

numpy only: no torch, no GPU.  Two references:

exact_ranks     integer-valued tables scored in int64.  With entries in
                [-3, 3] every partial sum of every model's score is an integer
                below 2^24 up to d = 788 (|q_k| <= 9 d, |score| <= 27 d^2; 8 d^2
                with entries in [-2, 2], d = 1024), so fp32, fp64 and int64
                agree bit for bit and a device rank must EQUAL the reference,
                exact ties included.
rank_envelope   float tables (fp32 values widened to fp64) scored in fp64 with
                a derived bound on any sequential fp32 evaluation's error: the
                interval [lo, hi] of ranks a correct fp32 kernel may return.

The rule is the project's (csrc/skge_eval.hip header): a position is 1 + the
number of entities scoring strictly higher than the true one; the filtered
count skips every known triple other than the query itself.

make_int_case / make_float_case build the seeded tables, test triples and
known triples that tests/test_eval_ref.py (CPU) and
tests/test_gpu_eval_exact.py (GPU) share.
"""
import numpy as np

from oracle import skge_oracle as O

U32 = 2.0 ** -24          # fp32 unit roundoff
_CHUNK_ELEMS = 1 << 23    # int64 elements of the largest temporary


# ----------------------------------------------------------------------------
# integer scores
# ----------------------------------------------------------------------------

def _int_tables(E, R):
    Ei, Ri = np.asarray(E), np.asarray(R)
    if not (np.all(Ei == np.rint(Ei)) and np.all(Ri == np.rint(Ri))):
        raise ValueError("int_scores needs integer-valued tables")
    return Ei.astype(np.int64), Ri.astype(np.int64)


def _int_query_vectors(model, E, R, S, Oo, P, direction):
    """[n, d] int64 query vectors: every model's score of entity j is a distance
    to, or a dot product with, one vector (direct sums, no FFT)."""
    d = E.shape[1]
    a = E[S] if direction == "tail" else E[Oo]
    if model == "transe":
        return a + R[P] if direction == "tail" else a - R[P]
    if model == "hole":
        k, j = np.arange(d)[:, None], np.arange(d)[None, :]
        # tail: cconv(R_p, E_s)_k = sum_j R_j E_s[(k - j) mod d]
        # head: ccorr(R_p, E_o)_k = sum_j R_j E_o[(j + k) mod d]
        idx = (k - j) % d if direction == "tail" else (j + k) % d
        return np.einsum("nj,nkj->nk", R[P], a[:, idx])
    if model == "rescal":
        # tail: E_s W_p; head: W_p E_o
        return np.einsum("nj,njk->nk", a, R[P]) if direction == "tail" else \
            np.einsum("nkj,nj->nk", R[P], a)
    if model in ("distmult", "complex"):
        # tail: E_s * R_p; head: conj(R_p) * E_o (diag_ref.q_tail / q_head)
        return int_diag_mul(model, a, R[P], False) if direction == "tail" else \
            int_diag_mul(model, R[P], a, True)
    raise ValueError("unknown model %r" % (model,))


def int_diag_mul(model, x, y, conj):
    """int64 x * y (conj: conj(x) * y) over the last axis: elementwise for
    DistMult, the complex product on interleaved (re, im) for ComplEx -- the
    query vectors of tests/diag_ref.py (tail s * r, head conj(r) * o, relation
    conj(s) * o); the score of a candidate row is its plain dot product with
    one of them.

    With entries in [-3, 3] an element of the product is at most 9 + 9 = 18
    in magnitude and a score at most 3 * 18 d = 54 d, 55,296 at d = 1024: every
    fp32 product, fma and partial sum of any evaluation order is an integer far
    below 2^24, so a device result must EQUAL the int64 one."""
    d = x.shape[-1]
    lim = int(max(np.abs(x).max(initial=0), np.abs(y).max(initial=0)))
    assert lim <= 3 and 2 * lim ** 3 * d < 2 ** 24
    if model == "distmult":
        return x * y
    if d % 2:
        raise ValueError("ComplEx needs an even width, not %d" % d)
    a, b = x[..., 0::2], x[..., 1::2]
    f, g = y[..., 0::2], y[..., 1::2]
    out = np.empty(np.broadcast(x, y).shape, dtype=np.int64)
    if conj:
        out[..., 0::2] = a * f + b * g
        out[..., 1::2] = a * g - b * f
    else:
        out[..., 0::2] = a * f - b * g
        out[..., 1::2] = a * g + b * f
    return out


def _int_scores_batch(model, E, R, S, Oo, P, direction):
    """[n, N] int64 scores of every entity for n queries."""
    q = _int_query_vectors(model, E, R, S, Oo, P, direction)
    if model == "transe":
        return -np.abs(q[:, None, :] - E[None, :, :]).sum(axis=2)
    return q @ E.T


def int_scores(model, E, R, s, o, p, direction):
    """int64 scores of every entity as the tail of (s, p, ?) (direction
    'tail') or the head of (?, p, o) ('head') on integer-valued tables:
    TransE -sum|E_s + R_p - E_j| / -sum|E_j + R_p - E_o|; HolE circular
    correlation / convolution as direct sums; RESCAL E_s W_p E^T / E W_p E_o."""
    Ei, Ri = _int_tables(E, R)
    one = lambda v: np.asarray([v], dtype=np.int64)
    return _int_scores_batch(model, Ei, Ri, one(s), one(o), one(p), direction)[0]


# ----------------------------------------------------------------------------
# the filter
# ----------------------------------------------------------------------------

def _filter_masks(a, P, ka, kb, kP, N, M):
    """[n, N] bool: mask[i, j] = the triple with fixed side a[i], relation P[i]
    and varying side j is known.  (ka, kb, kP) are the known triples' fixed
    side, varying side and relation."""
    keys = a.astype(np.int64) * M + P
    ukeys, grp = np.unique(keys, return_inverse=True)
    kkeys = ka.astype(np.int64) * M + kP
    pos = np.searchsorted(ukeys, kkeys)
    pos[pos == len(ukeys)] = 0
    hit = ukeys[pos] == kkeys if len(ukeys) else np.zeros(len(kkeys), dtype=bool)
    gmask = np.zeros((len(ukeys), N), dtype=bool)
    gmask[pos[hit], kb[hit]] = True
    return gmask, grp.reshape(-1)


def exact_ranks(model, E, R, queries, known):
    """[nq, 4] int64 (tail raw, tail filtered, head raw, head filtered) for
    queries (s, o, p) on integer-valued tables, from int_scores' arithmetic."""
    Ei, Ri = _int_tables(E, R)
    N, d = Ei.shape
    M = Ri.shape[0]
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    kn = np.asarray(known, dtype=np.int64).reshape(-1, 3)
    S, Oo, P = q[:, 0], q[:, 1], q[:, 2]
    out = np.zeros((len(q), 4), dtype=np.int64)
    per = N * d if model == "transe" else max(N, d * d)
    step = max(1, _CHUNK_ELEMS // per)
    for col, direction, fixed, true, kfix, kvar in (
            (0, "tail", S, Oo, kn[:, 0], kn[:, 1]), (2, "head", Oo, S, kn[:, 1], kn[:, 0])):
        gmask, grp = _filter_masks(fixed, P, kfix, kvar, kn[:, 2], N, M)
        for i0 in range(0, len(q), step):
            sl = slice(i0, i0 + step)
            sc = _int_scores_batch(model, Ei, Ri, S[sl], Oo[sl], P[sl], direction)
            rows = np.arange(sc.shape[0])
            higher = sc > sc[rows, true[sl]][:, None]
            mask = gmask[grp[sl]]
            mask[rows, true[sl]] = False          # the query itself is never filtered
            out[sl, col] = 1 + higher.sum(axis=1)
            out[sl, col + 1] = 1 + (higher & ~mask).sum(axis=1)
    return out


# ----------------------------------------------------------------------------
# the fp32 envelope
# ----------------------------------------------------------------------------

def _abs_scores(model, E, R, s, o, p, direction):
    """A_j: the scoring formula on absolute values (the sum of the absolute
    values of the terms of entity j's score)."""
    aE, aR = np.abs(E), np.abs(R)
    if model == "transe":
        fixed = aE[s] if direction == "tail" else aE[o]
        return np.sum(fixed + aR[p] + aE, axis=1)
    return O.entity_scores(model, aE, aR, s, o, p, direction)


def rank_envelope(model, E, R, queries, known):
    """(lo, hi), each [nq, 4] int64: the ranks any correct fp32 evaluation
    that sums its d terms sequentially may return, for float tables holding
    fp32 values (widened to fp64).

    Every entity's score sc_j is computed in fp64 (oracle.entity_scores).  Its
    fp32 counterpart differs from it by at most

        tau_j = 2 (d + 2) u A_j,      u = 2^-24,

    A_j the same formula on absolute values: a d-term sequential fp32 sum
    carries at most d u sum|t_k| to first order; the query vector the terms
    are built from is itself such a sum (HolE, RESCAL: another d u A_j) or one
    rounded add (TransE: u A_j, and one more for the rounded difference), and
    the remaining 4 u A_j covers the second-order terms (d^2 u^2 A_j, below
    4 u A_j for every d the kernels take).  The constant is derived, not
    tuned: a device rank outside [lo, hi] is a finding about the kernel.  So
    entity j certainly outscores the true entity t when sc_j - sc_t > tau_j +
    tau_t and certainly does not when sc_j - sc_t < -(tau_j + tau_t):

        lo = 1 + #{j : sc_j - sc_t > tau_j + tau_t}
        hi = 1 + #{j != t : sc_j - sc_t >= -(tau_j + tau_t)}

    and the filtered bounds are the same counts over the entities that are
    not filtered out."""
    E = np.asarray(E, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    N, d = E.shape
    kset = set(map(tuple, np.asarray(known).reshape(-1, 3).tolist()))
    q = np.asarray(queries).reshape(-1, 3).tolist()
    lo = np.zeros((len(q), 4), dtype=np.int64)
    hi = np.zeros((len(q), 4), dtype=np.int64)
    ent = np.arange(N)
    for i, (s, o, p) in enumerate(q):
        for col, direction, t in ((0, "tail", o), (2, "head", s)):
            sc = O.entity_scores(model, E, R, s, o, p, direction)
            tau = 2.0 * (d + 2) * U32 * _abs_scores(model, E, R, s, o, p, direction)
            diff = sc - sc[t]
            slack = tau + tau[t]
            above = diff > slack
            maybe = (diff >= -slack) & (ent != t)
            if direction == "tail":
                filt = np.array([(s, j, p) in kset and j != o for j in range(N)])
            else:
                filt = np.array([(j, o, p) in kset and j != s for j in range(N)])
            lo[i, col] = 1 + above.sum()
            hi[i, col] = 1 + maybe.sum()
            lo[i, col + 1] = 1 + (above & ~filt).sum()
            hi[i, col + 1] = 1 + (maybe & ~filt).sum()
    return lo, hi


# ----------------------------------------------------------------------------
# seeded cases
# ----------------------------------------------------------------------------

def eval_order(test):
    """The evaluator's query order: by relation in order of first appearance,
    then insertion order (FilteredRankingEval.idx)."""
    test = np.asarray(test).reshape(-1, 3)
    first = {}
    for i, p in enumerate(test[:, 2].tolist()):
        first.setdefault(p, i)
    key = np.array([first[p] for p in test[:, 2].tolist()], dtype=np.int64)
    return test[np.argsort(key, kind="stable")]


def random_triples(rs, N, M, nq):
    """nq test triples and a known set holding them plus, for randomly picked
    test triples, other tails (s, o', p) and heads (s', o, p): dense enough
    that filtering moves ranks."""
    test = np.stack([rs.randint(N, size=nq), rs.randint(N, size=nq), rs.randint(M, size=nq)],
                    axis=1).astype(np.int32)
    nk = int(np.clip(8 * nq, 64, 20000))
    pick = test[rs.randint(nq, size=nk)]
    tails = np.stack([pick[:, 0], rs.randint(N, size=nk), pick[:, 2]], axis=1)
    pick = test[rs.randint(nq, size=nk)]
    heads = np.stack([rs.randint(N, size=nk), pick[:, 1], pick[:, 2]], axis=1)
    known = np.unique(np.concatenate([test, tails, heads]), axis=0).astype(np.int32)
    return test, known


def rel_shape(model, M, d):
    return (M, d, d) if model == "rescal" else (M, d)


def make_int_case(model, d, N, nq, seed, M=3):
    """Integer tables with entries in [-3, 3] ([-2, 2] from d = 789 up, where
    27 d^2 would pass 2^24), as float64 arrays; test and known triples."""
    rs = np.random.RandomState(seed)
    lim = 3 if 27 * d * d < 2 ** 24 else 2
    assert (lim * lim * lim) * d * d < 2 ** 24
    E = rs.randint(-lim, lim + 1, size=(N, d)).astype(np.float64)
    R = rs.randint(-lim, lim + 1, size=rel_shape(model, M, d)).astype(np.float64)
    test, known = random_triples(rs, N, M, nq)
    return E, R, test, known


def make_float_case(model, d, scale, seed, N=300, M=5, nq=120):
    """fp32 tables, uniform at init scale (+-sqrt(6 / (rows + cols)), the
    models' init_nunif) times `scale`, widened to float64."""
    rs = np.random.RandomState(seed)

    def unif(shape):
        bnd = scale * np.sqrt(6.0) / np.sqrt(shape[0] + shape[1])
        return rs.uniform(-bnd, bnd, size=shape).astype(np.float32).astype(np.float64)
    E = unif((N, d))
    R = unif(rel_shape(model, M, d))
    test, known = random_triples(rs, N, M, nq)
    return E, R, test, known


# (model, d, N, nq): every edge of the kernels at least once per model --
# d < 4, the scalar tail (d & 3), the 32-dim chunk boundary (31 / 32 / 33,
# 64 / 65), d = 1024 (the entry points' bound, 40 KB of LDS in k_rank_query);
# N = 1, 2, below / at / above the 64- and 128-entity tiles; nq at the 64-vector
# query block (2 nq = 62, 64, 66); ragged multi-tile entity slices (nq = 2048,
# N = 4500: 64 query blocks, 36 tiles, 2 per slice, 18 slices); one slice with
# the query kernel's grid-stride loop (nq = 65600: 2050 query blocks, more
# than 2 x 16384 x 2 queries)
_COMMON = [(1, 300, 97), (3, 129, 33), (31, 63, 31), (32, 64, 32), (33, 65, 33), (64, 127, 1),
           (65, 128, 97), (33, 1, 31), (3, 2, 33), (65, 300, 32), (1024, 130, 33),
           (8, 4500, 2048), (4, 130, 65600)]
INT_CASES = [(m,) + c for m in ("transe", "hole", "rescal") for c in _COMMON]

# (model, d, scale): section (c)'s float cases, N = 300, M = 5, 120 queries
FLOAT_CASES = [(m, d, sc) for m, d in (("transe", 40), ("hole", 33), ("rescal", 37))
               for sc in (1.0, 8.0)]


def case_seed(*key):
    """A stable seed per case (Python's hash() of a str is salted per run)."""
    h = 2166136261
    for ch in repr(key).encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h
