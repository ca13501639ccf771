"""Device top-k link prediction (skge_topk through skge_amd.LinkPredictor)
against the references of tests/topk_ref.py:

(a) integer tables, where fp32, fp64 and int64 scores agree bit for bit, so
    ids and scores must EQUAL exact_topk -- at the edges of the kernels (d < 4,
    the scalar tail, the 32-dim chunk boundary, d = 1024, N around the
    128-entity tile, N = 1, ragged query blocks, multi-tile entity slices), for
    k on both sides of the 32 / 64 / 128 list layouts and above N, with and
    without exclusion lists, and for TransE's squared-L2 code;
(b) ties and the bookkeeping of exclusions and padding, by construction;
(c) agreement with FilteredRankingEval's filtered ranks;
(d) float tables, inside topk_envelope's derived fp32 bounds;
(e) the facade.
"""
import functools

import numpy as np
import pytest
import torch

import eval_ref as X
import topk_ref as T

pytestmark = pytest.mark.gpu

MODELS = ["transe", "hole", "rescal"]
# (d, N, nq)
CASES_A = [(1, 300, 97), (3, 129, 33), (31, 63, 31), (32, 64, 32), (33, 65, 33), (65, 128, 97),
           (33, 1, 31), (3, 2, 33), (1024, 130, 33), (8, 4500, 2048)]
KS = (1, 2, 10, 64, 128)


def _model(name, E, R, **kw):
    """The model with the given tables (as test_gpu_eval_exact._model)."""
    import skge_amd as S
    n_ent, d = E.shape
    m = {"transe": S.TransE, "hole": S.HolE, "rescal": S.RESCAL}[name](
        (n_ent, n_ent, R.shape[0]), d, init="device_nunif", **kw)
    rid = "W" if name == "rescal" else "R"
    assert m.params["E"].shape == E.shape and m.params[rid].shape == R.shape
    m.params["E"].data.copy_(torch.tensor(E, dtype=torch.float32))
    m.params[rid].data.copy_(torch.tensor(R, dtype=torch.float32))
    return m


def _predictor(name, E, R, known=None, l2=False):
    import skge_amd as S
    kw = {"l1": False} if l2 else {}
    return S.LinkPredictor(_model(name, E, R, **kw), known,
                           scoring="model" if l2 else "eval")


def _ask(lp, direction, q, **kw):
    fn = lp.tails if direction == "tail" else lp.heads
    ents, scores = fn(q[:, 0], q[:, 1], **kw)
    assert ents.dtype == np.int64 and scores.dtype == np.float32
    assert ents.shape == scores.shape == (len(q), kw["k"])
    return ents, scores


def _queries(test, direction):
    test = np.asarray(test)
    return test[:, [0, 2]] if direction == "tail" else test[:, [1, 2]]


def _assert_equal(got, want, msg):
    np.testing.assert_array_equal(got[0], want[0], err_msg="ids, " + msg)
    np.testing.assert_array_equal(got[1].astype(np.float64), want[1], err_msg="scores, " + msg)


# ---------------------------------------------------------------------------
# (a) exact equality on integer tables
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _int_ref(model, l2, d, N, nq):
    """The case and, per (direction, with exclusions), the reference's full
    order up to the largest k asked: computed once; every smaller k's result
    is its first k columns (a prefix of a sorted list), padding included."""
    E, R, test, known = X.make_int_case(model, d, N, nq, X.case_seed(model, d, N, nq))
    kmax = max(_ks(N))
    ref = {}
    for direction in T.DIRECTIONS:
        q = _queries(test, direction)
        sc = T.int_query_scores(model, E, R, q, direction, l2=l2)
        excl = T.known_answers(q, known, direction)
        for flt in (False, True):
            ids, val = T.topk_of_scores(sc, kmax, excl if flt else None)
            ids.setflags(write=False)
            val.setflags(write=False)
            ref[direction, flt] = (ids, val)
    for a in (E, R, test, known):
        a.setflags(write=False)
    return E, R, test, known, ref


def _ks(N):
    return KS + ((N + 1,) if N + 1 <= 128 else ())


@pytest.mark.parametrize("d,N,nq", CASES_A)
@pytest.mark.parametrize("model,l2", [(m, False) for m in MODELS] + [("transe", True)])
def test_int_tables_exact(model, l2, d, N, nq):
    E, R, test, known, ref = _int_ref(model, l2, d, N, nq)
    lp = _predictor(model, E, R, known, l2=l2)
    excluded = 0
    for direction in T.DIRECTIONS:
        q = _queries(test, direction)
        for flt in (False, True):
            ids, val = ref[direction, flt]
            for k in _ks(N):
                got = _ask(lp, direction, q, k=k, filtered=flt)
                _assert_equal(got, (ids[:, :k], val[:, :k]),
                              "%s k=%d filtered=%s" % (direction, k, flt))
            excluded += (ref[direction, False][0] != ids).any()
    if N >= 63:
        assert excluded     # the exclusion lists changed results
    if N + 1 <= 128:
        assert (ref["tail", False][0][:, N] == -1).all()    # k = N + 1 pads


def test_squared_l2_is_not_l1():
    """TransE(l1=False) under scoring='model' gets the squared-L2 order and
    under scoring='eval' the evaluator's L1 order; the two differ on this
    case, so neither can pass by computing the other."""
    E, R, test, known, ref2 = _int_ref("transe", True, 33, 65, 33)
    ref1 = _int_ref("transe", False, 33, 65, 33)[4]
    import skge_amd as S
    m = _model("transe", E, R, l1=False)
    for direction in T.DIRECTIONS:
        q = _queries(test, direction)
        got2 = _ask(S.LinkPredictor(m, scoring="model"), direction, q, k=10, filtered=False)
        got1 = _ask(S.LinkPredictor(m, scoring="eval"), direction, q, k=10, filtered=False)
        _assert_equal(got2, tuple(a[:, :10] for a in ref2[direction, False]), "L2 " + direction)
        _assert_equal(got1, tuple(a[:, :10] for a in ref1[direction, False]), "L1 " + direction)
        assert (got1[0] != got2[0]).any(axis=1).any()


# ---------------------------------------------------------------------------
# (b) ties, exclusions and padding by construction: d = 5 integer tables
# ---------------------------------------------------------------------------
N_B, D_B, M_B = 70, 5, 3


def _tables_b(model, seed, N=N_B):
    rs = np.random.RandomState(seed)
    E = rs.randint(-3, 4, size=(N, D_B)).astype(np.float64)
    R = rs.randint(-3, 4, size=X.rel_shape(model, M_B, D_B)).astype(np.float64)
    return rs, E, R


@pytest.mark.parametrize("direction", T.DIRECTIONS)
@pytest.mark.parametrize("model", MODELS)
def test_identical_rows_give_the_lowest_ids(model, direction):
    rs, E, R = _tables_b(model, 21)
    E[:] = E[0]
    test, known = X.random_triples(rs, N_B, M_B, 40)
    q = _queries(test, direction)
    excl = T.known_answers(q, known, direction)
    lp = _predictor(model, E, R, known)
    for k in (1, 10, 64):
        ents, scores = _ask(lp, direction, q, k=k, filtered=True)
        for i in range(len(q)):
            want = np.setdiff1d(np.arange(N_B), excl[i])[:k]
            np.testing.assert_array_equal(ents[i, :len(want)], want)
            assert (ents[i, len(want):] == -1).all()      # k = 64 can exceed the eligible
            assert (scores[i, :len(want)] == scores[i, 0]).all()
        _assert_equal((ents, scores), T.exact_topk(model, E, R, q, direction, k, excl), "k=%d" % k)


@pytest.mark.parametrize("nq", [5, 66000])
@pytest.mark.parametrize("direction", T.DIRECTIONS)
@pytest.mark.parametrize("model", MODELS)
def test_copies_across_tiles_and_slices_come_in_id_order(model, direction, nq):
    """N = 300 is three 128-entity tiles.  Five queries: three slices of one
    tile each; 66000 queries: two slices, the first of two tiles (k = 16, 1032
    blocks of 64 queries) or one slice of three tiles (k = 64, 2063 blocks of
    32).  Copies of the best entity's row sit in every tile, so equal scores
    meet inside a tile, across the tiles of a slice and across slices, and
    must come back in ascending id.  The 66000 queries repeat the five, and
    so must their rows."""
    rs, E, R = _tables_b(model, 22, N=300)
    copies = [3, 120, 127, 128, 200, 255, 256, 299]
    base = np.stack([np.array([10, 50, 150, 210, 280]), rs.randint(M_B, size=5)], axis=1)  # no copies
    first = T.exact_topk(model, E, R, base[:1], direction, 1, None)[0][0, 0]
    E[copies] = E[first]
    members = sorted(set(copies) | {int(first)})
    q = np.tile(base, (nq // 5, 1))
    lp = _predictor(model, E, R)
    for k in (16, 64):
        want = T.exact_topk(model, E, R, base, direction, k, None)
        got = _ask(lp, direction, q, k=k, filtered=False)
        _assert_equal((got[0][:5], got[1][:5]), want, "k=%d" % k)
        assert (got[0] == np.tile(want[0], (nq // 5, 1))).all()
        assert (got[1] == np.tile(got[1][:5], (nq // 5, 1))).all()
        row = got[0][0].tolist()
        at = [row.index(j) for j in members]     # all returned, adjacent, ascending
        assert at == list(range(at[0], at[0] + len(members)))
        assert len(set(got[1][0, at].tolist())) == 1


@pytest.mark.parametrize("direction", T.DIRECTIONS)
@pytest.mark.parametrize("model", MODELS)
def test_exclusions_that_leave_too_few(model, direction):
    rs, E, R = _tables_b(model, 23)
    q = np.stack([rs.randint(N_B, size=6), rs.randint(M_B, size=6)], axis=1)
    lp = _predictor(model, E, R)
    everything = [list(range(N_B))] * len(q)
    ents, scores = _ask(lp, direction, q, k=10, filtered=False, exclude=everything)
    assert (ents == -1).all() and np.isneginf(scores).all()
    for k in (2, 10, 65):
        keep = [rs.choice(N_B, size=k - 1, replace=False) for _ in q]      # k - 1 stay eligible
        excl = [np.setdiff1d(np.arange(N_B), kp) for kp in keep]
        ents, scores = _ask(lp, direction, q, k=k, filtered=False, exclude=excl)
        _assert_equal((ents, scores), T.exact_topk(model, E, R, q, direction, k, excl), "k=%d" % k)
        assert (ents[:, -1] == -1).all() and np.isneginf(scores[:, -1]).all()
        assert (ents[:, :-1] >= 0).all()
        for i, kp in enumerate(keep):
            assert sorted(ents[i, :-1].tolist()) == sorted(kp.tolist())


@pytest.mark.parametrize("direction", T.DIRECTIONS)
@pytest.mark.parametrize("model", MODELS)
def test_one_query_and_duplicate_queries(model, direction):
    rs, E, R = _tables_b(model, 24)
    test, known = X.random_triples(rs, N_B, M_B, 12)
    lp = _predictor(model, E, R, known)
    q1 = _queries(test, direction)[:1]
    excl = T.known_answers(q1, known, direction)
    _assert_equal(_ask(lp, direction, q1, k=10, filtered=True),
                  T.exact_topk(model, E, R, q1, direction, 10, excl), "nq = 1")
    q = _queries(test, direction)[[0, 3, 0, 5, 3, 0]]
    ents, scores = _ask(lp, direction, q, k=10, filtered=True)
    for i, j in ((0, 2), (0, 5), (1, 4)):
        assert (ents[i] == ents[j]).all() and (scores[i] == scores[j]).all()
    _assert_equal((ents, scores), T.exact_topk(model, E, R, q, direction, 10,
                                               T.known_answers(q, known, direction)), "duplicates")


# ---------------------------------------------------------------------------
# (c) agreement with the evaluator's filtered ranks
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d,N,nq", [(3, 129, 33), (33, 65, 33), (65, 128, 97)])
@pytest.mark.parametrize("model", MODELS)
def test_agrees_with_filtered_ranking_eval(model, d, N, nq):
    """For a test triple (s, o, p) with the other known tails excluded, a
    filtered tail rank r <= k puts o at 1-based position r + #{eligible j < o
    tying o's score} of lp.tails (the rank counts strictly higher scores; the
    list breaks ties by id); the same for heads."""
    import skge_amd as S
    E, R, test, known = _int_ref(model, False, d, N, nq)[:4]
    m = _model(model, E, R)
    triples = X.eval_order(test)
    ranks = S.FilteredRankingEval(np.array(test, dtype=np.int32),
                                  np.array(known, dtype=np.int32)).ranks(m)
    lp = S.LinkPredictor(m)
    k, found = 10, 0
    for direction, col, true in (("tail", 1, triples[:, 1]), ("head", 3, triples[:, 0])):
        q = _queries(triples, direction)
        excl = [a[a != t] for a, t in zip(T.known_answers(q, known, direction), true.tolist())]
        ents, _ = _ask(lp, direction, q, k=k, filtered=False, exclude=excl)
        sc = T.int_query_scores(model, E, R, q, direction)
        for i, t in enumerate(true.tolist()):
            r = int(ranks[i, col])
            if r > k:
                continue
            ok = np.ones(N, dtype=bool)
            ok[excl[i]] = False
            pos = r + int((ok[:t] & (sc[i, :t] == sc[i, t])).sum())
            if pos <= k:
                assert ents[i, pos - 1] == t, (direction, i, r, pos, ents[i].tolist())
                found += 1
            else:
                assert t not in ents[i].tolist()
    assert found      # such triples exist in the case


# ---------------------------------------------------------------------------
# (d) float tables inside the derived fp32 envelope
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _float_ref(model, d, scale, k):
    E, R, test, known = X.make_float_case(model, d, scale, X.case_seed(model, d, scale))
    env = {}
    for direction in T.DIRECTIONS:
        q = _queries(test, direction)
        excl = T.known_answers(q, known, direction)
        env[direction] = (q, excl) + T.topk_envelope(model, E, R, q, direction, k, excl)
    return E, R, known, env


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("model,d,scale", X.FLOAT_CASES)
def test_float_tables_inside_envelope(model, d, scale, k):
    """Every forced entity is returned, every returned entity is allowed,
    every returned score is within tau of the fp64 score, and the rows follow
    the contract's order on the returned scores.  The forced entities are
    nearly all of the result (measured on the CPU with the reference alone:
    at least 99.5% of the fp64 top-k slots in each of the 18 cases, worst
    rescal d=37 scale 1 k=1 at 0.9958), so the test is not vacuous."""
    E, R, known, env = _float_ref(model, d, scale, k)
    lp = _predictor(model, E, R, known)
    forced_n = slots = 0
    for direction in T.DIRECTIONS:
        q, excl, sc, tau, forced, allowed = env[direction]
        ents, scores = _ask(lp, direction, q, k=k, filtered=True)
        assert (ents >= 0).all()      # 300 entities, short exclusion lists: no padding
        rows = np.arange(len(q))[:, None]
        got = np.zeros_like(forced)
        got[rows, ents] = True
        assert (got.sum(axis=1) == k).all()      # distinct ids
        err = np.abs(scores.astype(np.float64) - sc[rows, ents])
        print("%s d=%d scale=%g k=%d %s: forced %d of %d, max err / tau %.3f"
              % (model, d, scale, k, direction, forced.sum(), got.sum(),
                 (err / tau[rows, ents]).max()))
        assert not (forced & ~got).any(), np.argwhere(forced & ~got)[:5].tolist()
        assert not (got & ~allowed).any(), np.argwhere(got & ~allowed)[:5].tolist()
        assert (err <= tau[rows, ents]).all()
        s0, s1, e0, e1 = scores[:, :-1], scores[:, 1:], ents[:, :-1], ents[:, 1:]
        assert ((s0 > s1) | ((s0 == s1) & (e0 < e1))).all()
        forced_n += forced.sum()
        slots += got.sum()
    assert forced_n / slots >= 0.99


# ---------------------------------------------------------------------------
# (e) the facade
# ---------------------------------------------------------------------------

def test_facade_scalars_arrays_filter_and_exclude():
    import skge_amd as S
    rs, E, R = _tables_b("hole", 25)
    test, known = X.random_triples(rs, N_B, M_B, 20)
    m = _model("hole", E, R)
    lp = S.LinkPredictor(m, known)
    s, o, p = (int(x) for x in test[0])
    # a scalar query is one row, and equals the same query in an array
    ents, scores = lp.tails(s, p, k=5)
    assert ents.shape == scores.shape == (1, 5)
    arr = lp.tails(test[:4, 0], test[:4, 2], k=5)
    assert (arr[0][0] == ents[0]).all() and (arr[1][0] == scores[0]).all()
    # filtered: no known answer is returned, the test triple's own object included
    tails = T.known_answers([(s, p)], known, "tail")[0]
    assert o in tails and not set(ents[0].tolist()) & set(tails.tolist())
    _assert_equal((ents, scores), T.exact_topk("hole", E, R, [(s, p)], "tail", 5, [tails]), "filtered")
    # unfiltered: the plain top-k; default k = 10
    raw = lp.tails(s, p, filtered=False)
    _assert_equal(raw, T.exact_topk("hole", E, R, [(s, p)], "tail", 10, None), "raw")
    # exclude is merged with the filter (unsorted, repeated, overlapping ids)
    extra = [int(ents[0, 0]), int(ents[0, 2]), int(tails[0]), int(ents[0, 0])]
    both = lp.tails(s, p, k=5, exclude=extra)
    merged = np.union1d(tails, extra)
    _assert_equal(both, T.exact_topk("hole", E, R, [(s, p)], "tail", 5, [merged]), "merged")
    assert not set(both[0][0].tolist()) & set(merged.tolist())
    heads = lp.heads([o, o], [p, p], k=3, exclude=[None, [int(x) for x in range(0, N_B, 2)]])
    hk = T.known_answers([(o, p)], known, "head")[0]
    _assert_equal(heads, T.exact_topk("hole", E, R, [(o, p), (o, p)], "head", 3,
                                      [hk, np.union1d(hk, np.arange(0, N_B, 2))]), "heads")
    # refusals come before any launch
    with pytest.raises(ValueError, match="known_triples"):
        S.LinkPredictor(m).tails(s, p)
    with pytest.raises(ValueError, match="subject %d" % N_B):
        lp.tails(N_B, p)
    with pytest.raises(ValueError, match="relation"):
        lp.heads(o, M_B)
    with pytest.raises(ValueError, match="exclude"):
        lp.tails(s, p, exclude=[N_B])
    for k in (0, 129):
        with pytest.raises(ValueError, match="k must be"):
            lp.tails(s, p, k=k)
