"""References for ranking and top-k over candidate pools
(csrc/skge_pools.hip, FilteredRankingEval.candidate_ranks / typed_ranks,
LinkPredictor(..., candidates=...)).  numpy only: no torch, no GPU.  Builds on
eval_ref and topk_ref.

The contract (include/skge_hip.h, skge_rank_pools): every query vector --
vector 2i the tail query of test triple i, 2i + 1 its head query -- names a
pool of candidate entities, or -1 for all of them.  Its raw rank is 1 + the
number of POOL MEMBERS scoring strictly above the true entity (the true
entity itself adds nothing, in the pool or not; an empty pool gives 1), and
the filtered rank subtracts the known answers of the query that are pool
members and score strictly above it.

exact_pool_ranks    integer-valued tables scored in int64 (eval_ref's
                    argument): a device rank must EQUAL it.
pool_rank_envelope  float tables: eval_ref.rank_envelope's derivation with the
                    counts taken over pool members only.
exact_pool_topk     topk_ref's contract among the members of each query's pool.
"""
import numpy as np

import eval_ref as X
import topk_ref as T
from oracle import skge_oracle as O


def member_mask(pools, pool_id, N):
    """[N] bool: the candidates of pool `pool_id` (-1: every entity)."""
    m = np.ones(N, dtype=bool)
    if pool_id >= 0:
        m[:] = False
        m[np.asarray(pools[pool_id], dtype=np.int64)] = True
    return m


def type_pools_of(known, M):
    """DeviceKG.pools' lists: pool 2p = the sorted subjects of relation p in
    `known`, pool 2p + 1 its sorted objects."""
    kn = np.asarray(known, dtype=np.int64).reshape(-1, 3)
    pools = []
    for p in range(M):
        sel = kn[kn[:, 2] == p]
        pools += [np.unique(sel[:, 0]), np.unique(sel[:, 1])]
    return pools


def typed_vec_pool(queries):
    """The type-constrained assignment: the tail query of (s, o, p) ranks over
    the range of p (pool 2p + 1), the head query over its domain (pool 2p)."""
    p = np.asarray(queries, dtype=np.int64).reshape(-1, 3)[:, 2]
    return np.stack([2 * p + 1, 2 * p], axis=1).reshape(-1)


# ----------------------------------------------------------------------------
# integer tables: the exact ranks
# ----------------------------------------------------------------------------

def exact_pool_ranks(model, E, R, queries, known, pools, vec_pool):
    """[nq, 4] int64 (tail raw, tail filtered, head raw, head filtered) on
    integer-valued tables; vec_pool [2 nq]."""
    Ei, Ri = X._int_tables(E, R)
    N, d = Ei.shape
    M = Ri.shape[0]
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    kn = np.asarray(known, dtype=np.int64).reshape(-1, 3)
    vp = np.asarray(vec_pool, dtype=np.int64).reshape(-1, 2)
    S, Oo, P = q[:, 0], q[:, 1], q[:, 2]
    out = np.zeros((len(q), 4), dtype=np.int64)
    if not len(q):
        return out
    masks = {g: member_mask(pools, g, N) for g in set(vp.reshape(-1).tolist())}
    per = N * d if model == "transe" else max(N, d * d)
    step = max(1, X._CHUNK_ELEMS // per)
    for col, direction, fixed, true, kfix, kvar in (
            (0, "tail", S, Oo, kn[:, 0], kn[:, 1]), (2, "head", Oo, S, kn[:, 1], kn[:, 0])):
        gmask, grp = X._filter_masks(fixed, P, kfix, kvar, kn[:, 2], N, M)
        for i0 in range(0, len(q), step):
            sl = slice(i0, i0 + step)
            sc = X._int_scores_batch(model, Ei, Ri, S[sl], Oo[sl], P[sl], direction)
            rows = np.arange(sc.shape[0])
            member = np.stack([masks[g] for g in vp[sl, col // 2].tolist()])
            higher = (sc > sc[rows, true[sl]][:, None]) & member
            mask = gmask[grp[sl]]
            mask[rows, true[sl]] = False          # the query itself is never filtered
            out[sl, col] = 1 + higher.sum(axis=1)
            out[sl, col + 1] = 1 + (higher & ~mask).sum(axis=1)
    return out


def known_above_outside(model, E, R, queries, known, pools, vec_pool):
    """The number of (query vector, known answer) pairs where the answer is
    NOT in the vector's pool and scores strictly above the true entity: what
    a filter without the membership test would wrongly subtract."""
    everything = [-1] * (2 * len(queries))
    with_pool = exact_pool_ranks(model, E, R, queries, known, pools, vec_pool)
    without = exact_pool_ranks(model, E, R, queries, known, pools, everything)
    # known answers above the true entity: all of them, and those in the pool
    dec_all = (without[:, 0::2] - without[:, 1::2])
    dec_in = (with_pool[:, 0::2] - with_pool[:, 1::2])
    return int((dec_all - dec_in).sum())


# ----------------------------------------------------------------------------
# float tables: the fp32 envelope over pool members
# ----------------------------------------------------------------------------

def pool_rank_envelope(model, E, R, queries, known, pools, vec_pool):
    """(lo, hi), each [nq, 4] int64: eval_ref.rank_envelope (its tau_j =
    2 (d + 2) u A_j and its certainly-above / possibly-above counts) with the
    counts taken over the members of each vector's pool."""
    E = np.asarray(E, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    N, d = E.shape
    kset = set(map(tuple, np.asarray(known).reshape(-1, 3).tolist()))
    q = np.asarray(queries).reshape(-1, 3).tolist()
    vp = np.asarray(vec_pool, dtype=np.int64).reshape(-1, 2)
    lo = np.zeros((len(q), 4), dtype=np.int64)
    hi = np.zeros((len(q), 4), dtype=np.int64)
    ent = np.arange(N)
    for i, (s, o, p) in enumerate(q):
        for col, direction, t in ((0, "tail", o), (2, "head", s)):
            member = member_mask(pools, int(vp[i, col // 2]), N)
            sc = O.entity_scores(model, E, R, s, o, p, direction)
            tau = 2.0 * (d + 2) * X.U32 * X._abs_scores(model, E, R, s, o, p, direction)
            diff = sc - sc[t]
            slack = tau + tau[t]
            above = (diff > slack) & member
            maybe = (diff >= -slack) & (ent != t) & member
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
# top-k among pool members
# ----------------------------------------------------------------------------

def pool_exclusions(N, pools, query_pool, excl=None):
    """Per query the sorted ids that may not be returned: everything outside
    its pool, and its exclusion list."""
    out = []
    for g, ex in zip(np.asarray(query_pool).tolist(), T._excl_lists(excl, len(query_pool))):
        outside = np.flatnonzero(~member_mask(pools, g, N))
        out.append(np.union1d(outside, ex))
    return out


def exact_pool_topk(model, E, R, queries, direction, k, excl, pools, query_pool, l2=False):
    """topk_ref.exact_topk among the members of pool query_pool[i] that are
    not on query i's exclusion list: (ids [nq, k] int64, scores [nq, k])."""
    N = np.asarray(E).shape[0]
    return T.exact_topk(model, E, R, queries, direction, k,
                        pool_exclusions(N, pools, query_pool, excl), l2)


# ----------------------------------------------------------------------------
# seeded cases
# ----------------------------------------------------------------------------

POOL_SIZES = (0, 1, 63, 64, 65, 127, 128, 129)


def _subset(rs, N, size):
    return np.sort(rs.choice(N, size=min(size, N), replace=False)).astype(np.int64)


def make_pools(kind, rs, N, M, test, known):
    """(pools, vec_pool [2 nq]) for the seeded test and known triples.
      typed   the type index of `known` (2 M pools), tail -> 2p + 1, head -> 2p
      sizes   hand-made overlapping random pools of POOL_SIZES entries (empty,
              one, both sides of half a 128-candidate tile and of a whole
              one), vectors dealt over them in a shuffled round: the true
              entities are mostly outside their pools
      mixed   the type index plus hand-made pools; a vector takes -1, its typed
              pool or a hand-made one
      groups  groups of 1, 63, 64 and 65 vectors on one pool each (the
              64-vector block boundary) and the rest on -1, shuffled
      big     one pool of 0.9 N entries for every vector: several slices of
              several tiles, the last one ragged
      many    200 pools, far more than vectors: most stay unused
      all     no pools; every vector -1
      full    one explicit pool 0 .. N - 1 for every vector"""
    nv = 2 * len(test)
    if kind == "typed":
        return type_pools_of(known, M), typed_vec_pool(test)
    if kind == "sizes":
        pools = [_subset(rs, N, n) for n in POOL_SIZES]
        vp = np.resize(np.arange(len(pools)), nv)
        return pools, rs.permutation(vp)
    if kind == "mixed":
        pools = type_pools_of(known, M) + [_subset(rs, N, n) for n in (N // 2, N // 3, 65, 10)]
        typed = typed_vec_pool(test)
        hand = 2 * M + rs.randint(4, size=nv)
        pick = rs.randint(5, size=nv)        # 1 in 5: -1; 2 in 5: typed; 2 in 5: hand-made
        return pools, np.where(pick == 0, -1, np.where(pick <= 2, typed, hand))
    if kind == "groups":
        pools = [_subset(rs, N, n) for n in (90, 129, 40, 200)]
        vp = np.concatenate([np.full(n, g) for g, n in enumerate((1, 63, 64, 65))])
        assert nv >= len(vp)
        vp = np.concatenate([vp, np.full(nv - len(vp), -1)])
        return pools, rs.permutation(vp)
    if kind == "big":
        return [_subset(rs, N, (9 * N) // 10)], np.zeros(nv, dtype=np.int64)
    if kind == "many":
        pools = [_subset(rs, N, rs.randint(0, 40)) for _ in range(200)]
        return pools, rs.randint(200, size=nv)
    if kind == "all":
        return [], np.full(nv, -1)
    if kind == "full":
        return [np.arange(N)], np.zeros(nv, dtype=np.int64)
    raise ValueError(kind)


# (kind, d, N, nq): every d edge of the kernels (d < 4, the scalar tail, the
# 32-dim chunk boundary, d = 1024), every pool size around the 128-candidate
# tile, the 64-vector block boundary, slices (big: 4096 vectors -> 66 items at
# most, 20 slices of 2 tiles for N = 5000; the pool's 36 tiles fill 18, the
# last tile 20 rows), unused pools, -1 alone and mixed, nq = 1
_COMMON = [("typed", 1, 300, 97), ("sizes", 3, 300, 64), ("typed", 31, 63, 31),
           ("sizes", 32, 300, 40), ("mixed", 33, 130, 33), ("groups", 65, 300, 97),
           ("sizes", 1024, 130, 16), ("big", 8, 5000, 2048), ("many", 4, 130, 5),
           ("all", 33, 129, 33), ("full", 3, 129, 33), ("typed", 5, 300, 1), ("mixed", 5, 300, 1)]
INT_CASES = [(m,) + c for m in ("transe", "hole", "rescal") for c in _COMMON]
# kinds whose pools hold fewer than all entities / are hand-made (a known
# answer can lie outside them; the type index of `known` holds every answer)
RESTRICTING = ("typed", "sizes", "mixed", "groups", "big", "many")
HAND_MADE = ("sizes", "mixed", "groups")

# float cases: eval_ref's shapes (N = 300, M = 5, 120 queries, scales 1 and 8)
FLOAT_CASES = X.FLOAT_CASES
M_INT = 3


def int_case(model, kind, d, N, nq):
    """(E, R, test, known, pools, vec_pool), seeded by the case; the test
    triples come in the evaluator's order."""
    seed = X.case_seed("pools", model, kind, d, N, nq)
    E, R, test, known = X.make_int_case(model, d, N, nq, seed, M=M_INT)
    test = X.eval_order(test)
    pools, vp = make_pools(kind, np.random.RandomState(seed ^ 0x5bd1e995), N, M_INT, test, known)
    return E, R, test, known, pools, np.asarray(vp, dtype=np.int64)


def float_case(model, d, scale):
    """eval_ref's float case with `mixed` pools."""
    seed = X.case_seed("pools", model, d, scale)
    E, R, test, known = X.make_float_case(model, d, scale, seed)
    test = X.eval_order(test)
    pools, vp = make_pools("mixed", np.random.RandomState(seed ^ 0x5bd1e995), 300, 5, test, known)
    return E, R, test, known, pools, np.asarray(vp, dtype=np.int64)


def topk_query_pool(kind, vec_pool, direction):
    """The pool of each of the nq top-k queries of one direction: the ranking
    vectors' (2i: tail, 2i + 1: head); for `groups`, groups of 1, 31, 32 and
    33 queries (the 32-query block boundary of k > 32) and the rest on -1."""
    vp = np.asarray(vec_pool).reshape(-1, 2)
    if kind != "groups":
        return vp[:, 0 if direction == "tail" else 1].copy()
    qp = np.concatenate([np.full(n, g) for g, n in enumerate((1, 31, 32, 33))])
    qp = np.concatenate([qp, np.full(len(vp) - len(qp), -1)])
    return np.random.RandomState(len(vp) + (direction == "head")).permutation(qp)
