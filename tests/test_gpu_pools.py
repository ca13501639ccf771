"""Device ranking and top-k over candidate pools (skge_rank_pools /
skge_topk_pools through FilteredRankingEval.candidate_ranks, typed_ranks and
LinkPredictor(..., candidates=...)) against the references of
tests/pool_ref.py:

(a) integer tables, where fp32, fp64 and int64 scores agree bit for bit: ranks
    must EQUAL exact_pool_ranks and top-k ids and scores exact_pool_topk, at
    every edge the case table lists (pool_ref.INT_CASES);
(b) float tables inside the derived fp32 envelopes;
(c) pool -1 and the explicit full pool equal skge_rank_known / skge_topk;
(d) the facade end to end on a 300-entity KG, and two runs agreeing.
"""
import functools

import numpy as np
import pytest
import torch

import eval_ref as X
import pool_ref as PR
import topk_ref as T

pytestmark = pytest.mark.gpu

MODELS = ["transe", "hole", "rescal"]
KS = (1, 10, 33, 128)      # 64- and 32-query blocks, every list layout


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


def _evaluator(test, known):
    import skge_amd as S
    return S.FilteredRankingEval(np.array(test, dtype=np.int32), np.array(known, dtype=np.int32))


def _queries(test, direction):
    test = np.asarray(test)
    return test[:, [0, 2]] if direction == "tail" else test[:, [1, 2]]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


# ---------------------------------------------------------------------------
# (a) integer tables: equality
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _int_ref(model, kind, d, N, nq):
    E, R, test, known, pools, vp = PR.int_case(model, kind, d, N, nq)
    exact = PR.exact_pool_ranks(model, E, R, test, known, pools, vp)
    _frozen(E, R, test, known, vp, exact)
    return E, R, test, known, pools, vp, exact


@pytest.mark.parametrize("model,kind,d,N,nq", PR.INT_CASES)
def test_int_tables_ranks_equal_reference(model, kind, d, N, nq):
    E, R, test, known, pools, vp, exact = _int_ref(model, kind, d, N, nq)
    ev = _evaluator(test, known)
    m = _model(model, E, R)
    got = ev.candidate_ranks(m, pools, vp[0::2], vp[1::2])
    assert got.dtype == np.int64 and got.shape == (nq, 4)
    np.testing.assert_array_equal(got, exact)
    # the CSR form, and a second run: the same integers
    import skge_amd as S
    again = ev.candidate_ranks(m, S.pool_csr(pools, N), vp[0::2], vp[1::2])
    np.testing.assert_array_equal(again, got)


@functools.lru_cache(maxsize=None)
def _int_topk_ref(model, kind, d, N, nq):
    """Per (direction, filtered) the reference's full order up to the largest
    k: every smaller k's result is its first k columns."""
    E, R, test, known, pools, vp = _int_ref(model, kind, d, N, nq)[:6]
    ref = {}
    for direction in T.DIRECTIONS:
        q = _queries(test, direction)
        qp = PR.topk_query_pool(kind, vp, direction)
        sc = T.int_query_scores(model, E, R, q, direction)
        known_excl = T.known_answers(q, known, direction)
        for flt in (False, True):
            excl = PR.pool_exclusions(N, pools, qp, known_excl if flt else None)
            ids, val = T.topk_of_scores(sc, max(KS), excl)
            _frozen(ids, val)
            ref[direction, flt] = (qp, ids, val)
    return ref


@pytest.mark.parametrize("model,kind,d,N,nq", PR.INT_CASES)
def test_int_tables_topk_equal_reference(model, kind, d, N, nq):
    import skge_amd as S
    E, R, test, known, pools, vp = _int_ref(model, kind, d, N, nq)[:6]
    ref = _int_topk_ref(model, kind, d, N, nq)
    lp = S.LinkPredictor(_model(model, E, R), known)
    csr = S.pool_csr(pools, N)
    padded = 0
    for direction in T.DIRECTIONS:
        q = _queries(test, direction)
        fn = lp.tails if direction == "tail" else lp.heads
        for flt in (False, True):
            qp, ids, val = ref[direction, flt]
            for k in KS:
                ents, scores = fn(q[:, 0], q[:, 1], k=k, filtered=flt, candidates=(csr, qp))
                assert ents.dtype == np.int64 and scores.dtype == np.float32
                msg = "%s k=%d filtered=%s" % (direction, k, flt)
                np.testing.assert_array_equal(ents, ids[:, :k], err_msg="ids, " + msg)
                np.testing.assert_array_equal(scores.astype(np.float64), val[:, :k],
                                              err_msg="scores, " + msg)
            padded += (ids == -1).any()
    if kind in ("sizes", "many", "groups"):
        assert padded       # k = 128 passes some pool's size: padding was compared


def test_l2_scoring_over_pools():
    """TransE(l1=False) under scoring='model' selects by the squared L2
    distance among pool members (skge_topk's second score form)."""
    import skge_amd as S
    E, R, test, known, pools, vp = _int_ref("transe", "sizes", 3, 300, 64)[:6]
    lp = S.LinkPredictor(_model("transe", E, R, l1=False), known, scoring="model")
    for direction in T.DIRECTIONS:
        q = _queries(test, direction)
        qp = PR.topk_query_pool("sizes", vp, direction)
        want = PR.exact_pool_topk("transe", E, R, q, direction, 10, None, pools, qp, l2=True)
        fn = lp.tails if direction == "tail" else lp.heads
        got = fn(q[:, 0], q[:, 1], k=10, filtered=False, candidates=(pools, qp))
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1].astype(np.float64), want[1])


# ---------------------------------------------------------------------------
# (b) float tables inside the envelopes
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _float_ref(model, d, scale):
    E, R, test, known, pools, vp = PR.float_case(model, d, scale)
    lo, hi = PR.pool_rank_envelope(model, E, R, test, known, pools, vp)
    _frozen(E, R, test, known, vp, lo, hi)
    return E, R, test, known, pools, vp, lo, hi


@pytest.mark.parametrize("model,d,scale", PR.FLOAT_CASES)
def test_float_tables_ranks_inside_envelope(model, d, scale):
    E, R, test, known, pools, vp, lo, hi = _float_ref(model, d, scale)
    got = _evaluator(test, known).candidate_ranks(_model(model, E, R), pools, vp[0::2], vp[1::2])
    print("%s d=%d scale=%g: %d of %d entries pinned, max width %d"
          % (model, d, scale, (lo == hi).sum(), lo.size, (hi - lo).max()))
    assert (lo <= got).all() and (got <= hi).all(), np.argwhere((got < lo) | (got > hi))[:5]


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("model,d,scale", PR.FLOAT_CASES)
def test_float_tables_topk_inside_envelope(model, d, scale, k):
    """test_gpu_topk's rule for skge_topk, with everything outside a query's
    pool excluded: every forced entity is returned, every returned entity is
    allowed and a pool member, every returned score is within tau of the fp64
    score, the rows follow the contract's order, and a row holds min(k,
    eligible) entities."""
    import skge_amd as S
    E, R, test, known, pools, vp = _float_ref(model, d, scale)[:6]
    lp = S.LinkPredictor(_model(model, E, R), known)
    N = E.shape[0]
    forced_n = slots = 0
    for direction in T.DIRECTIONS:
        q = _queries(test, direction)
        qp = PR.topk_query_pool("mixed", vp, direction)
        excl = PR.pool_exclusions(N, pools, qp, T.known_answers(q, known, direction))
        sc, tau, forced, allowed = T.topk_envelope(model, E, R, q, direction, k, excl)
        fn = lp.tails if direction == "tail" else lp.heads
        ents, scores = fn(q[:, 0], q[:, 1], k=k, filtered=True, candidates=(pools, qp))
        got = np.zeros_like(forced)
        for i in range(len(q)):
            n_ok = min(k, N - len(excl[i]))
            assert (ents[i, :n_ok] >= 0).all() and (ents[i, n_ok:] == -1).all()
            assert np.isneginf(scores[i, n_ok:]).all()
            got[i, ents[i, :n_ok]] = True
            assert got[i].sum() == n_ok          # distinct ids
            e, s = ents[i, :n_ok], scores[i, :n_ok]
            assert (np.abs(s.astype(np.float64) - sc[i, e]) <= tau[i, e]).all()
            assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (e[:-1] < e[1:]))).all()
        assert not (forced & ~got).any(), np.argwhere(forced & ~got)[:5].tolist()
        assert not (got & ~allowed).any(), np.argwhere(got & ~allowed)[:5].tolist()
        forced_n += forced.sum()
        slots += got.sum()
    print("%s d=%d scale=%g k=%d: forced %d of %d" % (model, d, scale, k, forced_n, slots))
    assert forced_n / slots >= 0.99


# ---------------------------------------------------------------------------
# (c) pool -1 and the explicit full pool are the all-entity entry points
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d,N,nq", [(33, 129, 33), (8, 4500, 2048), (65, 300, 1)])
@pytest.mark.parametrize("model", MODELS)
def test_minus_one_and_full_pool_equal_rank_known(model, d, N, nq):
    E, R, test, known = X.make_int_case(model, d, N, nq, X.case_seed("pools-c", model, d, N, nq))
    ev = _evaluator(test, known)
    m = _model(model, E, R)
    want = ev.ranks(m)
    minus = np.full(nq, -1)
    np.testing.assert_array_equal(ev.candidate_ranks(m, [], minus, minus), want)
    full = [np.arange(5), np.arange(N)]
    one = np.ones(nq, dtype=np.int64)
    np.testing.assert_array_equal(ev.candidate_ranks(m, full, one, one), want)
    np.testing.assert_array_equal(ev.candidate_ranks(m, full, minus, one), want)


@pytest.mark.parametrize("model", MODELS)
def test_minus_one_and_full_pool_equal_topk_on_float_tables(model):
    """Bit-equal scores: the gathered selection runs skge_topk's arithmetic."""
    import skge_amd as S
    E, R, test, known = X.make_float_case(model, 33, 1.0, X.case_seed("pools-c", model))
    lp = S.LinkPredictor(_model(model, E, R), known)
    for k in (10, 64):
        want = lp.tails(test[:, 0], test[:, 2], k=k)
        minus = np.full(len(test), -1)
        for cand in (([], minus), np.arange(300), ([np.arange(300)], minus + 1)):
            got = lp.tails(test[:, 0], test[:, 2], k=k, candidates=cand)
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])


# ---------------------------------------------------------------------------
# (d) the facade, end to end on a 300-entity KG
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("model", MODELS)
def test_typed_positions_candidate_ranks_and_predictor_end_to_end(model):
    import skge_amd as S
    E, R, test, known = X.make_int_case(model, 16, 300, 60, X.case_seed("pools-d", model), M=4)
    m = _model(model, E, R)
    ev = _evaluator(test, known)
    order = X.eval_order(test)
    pools = PR.type_pools_of(known, 4)
    want = PR.exact_pool_ranks(model, E, R, order, known, pools, PR.typed_vec_pool(order))
    # typed_ranks / typed_positions: the type index of true_triples
    got = ev.typed_ranks(m)
    np.testing.assert_array_equal(got, want)
    untyped = ev.ranks(m)
    assert (got <= untyped).all() and (got < untyped).any()
    cand = ev.last_typed_candidates
    assert cand.shape == (60, 2)
    for i, (s, o, p) in enumerate(order.tolist()):
        assert cand[i, 0] == len(set(pools[2 * p + 1].tolist()) | {o})
        assert cand[i, 1] == len(set(pools[2 * p].tolist()) | {s})
    assert (got[:, 0] <= cand[:, 0]).all() and (got[:, 2] <= cand[:, 1]).all()
    pos, fpos = ev.typed_positions(m)
    k = 0
    for p, sos in ev.idx.items():
        n = len(sos)
        assert pos[p] == {"tail": want[k:k + n, 0].tolist(), "head": want[k:k + n, 2].tolist()}
        assert fpos[p] == {"tail": want[k:k + n, 1].tolist(), "head": want[k:k + n, 3].tolist()}
        k += n
    raw, filt = S.ranking_scores(pos, fpos)
    uraw, ufilt = S.ranking_scores(*ev.positions(m))
    assert filt[0] >= raw[0] > uraw[0] and filt[0] > ufilt[0]        # MRR
    # another type index: the training triples, as a dict and as an array; a
    # true entity can now lie outside its pool
    train = known[::3]
    tpools = PR.type_pools_of(train, 4)
    twant = PR.exact_pool_ranks(model, E, R, order, known, tpools, PR.typed_vec_pool(order))
    np.testing.assert_array_equal(ev.typed_ranks(m, S.type_index(train.tolist())), twant)
    np.testing.assert_array_equal(ev.typed_ranks(m, train), twant)
    assert (ev.last_typed_candidates[:, 0] >=
            np.array([len(tpools[2 * p + 1]) for p in order[:, 2].tolist()])).all()
    # candidate_ranks: Python lists are sorted and de-duplicated
    lists = [list(reversed(p.tolist())) + p.tolist()[:2] for p in pools]
    vp = PR.typed_vec_pool(order)
    np.testing.assert_array_equal(ev.candidate_ranks(m, lists, vp[0::2], vp[1::2]), want)
    with pytest.raises(ValueError, match="pool 1 holds id 300"):
        ev.candidate_ranks(m, [[0], [300]], vp[0::2], vp[1::2])
    with pytest.raises(ValueError, match="tail_pool: entry 0 names pool"):
        ev.candidate_ranks(m, pools[:2], vp[0::2] + 8, vp[1::2])
    with pytest.raises(ValueError, match="pool ids for 60 test triples"):
        ev.candidate_ranks(m, pools, vp[0:10], vp[1::2])
    none = S.FilteredRankingEval(np.zeros((0, 3), dtype=np.int32), known)
    assert none.candidate_ranks(m, pools, [], []).shape == (0, 4)
    # the predictor
    lp = S.LinkPredictor(m, known)
    s, o, p = order[:, 0], order[:, 1], order[:, 2]
    for direction, anchor, fn in (("tail", s, lp.tails), ("head", o, lp.heads)):
        q = np.stack([anchor, p], axis=1)
        qp = 2 * p + (1 if direction == "tail" else 0)
        excl = T.known_answers(q, known, direction)
        got = fn(anchor, p, k=10, candidates="typed")
        ref = PR.exact_pool_topk(model, E, R, q, direction, 10, excl, pools, qp)
        np.testing.assert_array_equal(got[0], ref[0])
        np.testing.assert_array_equal(got[1].astype(np.float64), ref[1])
        # one explicit pool per query (a Python list: sorted here), and one for all
        mine = [np.arange(i % 7, 300, 7) for i in range(60)]
        got = fn(anchor, p, k=10, filtered=False, candidates=[list(x[::-1]) for x in mine])
        ref = PR.exact_pool_topk(model, E, R, q, direction, 10, None, mine, np.arange(60))
        np.testing.assert_array_equal(got[0], ref[0])
        shared = [3, 250, 17, 17, 99, 4]
        got = fn(anchor, p, k=10, filtered=False, candidates=shared)
        ref = PR.exact_pool_topk(model, E, R, q, direction, 10, None, [np.unique(shared)],
                                 np.zeros(60, dtype=np.int64))
        np.testing.assert_array_equal(got[0], ref[0])
        assert (got[0][:, 5:] == -1).all() and np.isneginf(got[1][:, 5:]).all()
        again = fn(anchor, p, k=10, filtered=False, candidates=shared)
        assert (again[0] == got[0]).all() and (again[1] == got[1]).all()
    with pytest.raises(ValueError, match="known_triples"):
        S.LinkPredictor(m).tails(s, p, filtered=False, candidates="typed")
    with pytest.raises(ValueError, match="candidates"):
        lp.tails(s, p, candidates="range")
    with pytest.raises(ValueError, match="holds id 300"):
        lp.tails(s, p, candidates=[1, 300])
    with pytest.raises(ValueError, match="2 pools for 60 queries"):
        lp.tails(s, p, candidates=[[1], [2]])
