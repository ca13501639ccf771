"""Relation prediction on the device (skge_relrank / skge_reltopk,
FilteredRankingEval.relation_ranks, LinkPredictor.relations) against the
references of tests/relation_ref.py:

(a) integer tables, where fp32, fp64 and int64 scores agree bit for bit: ranks
    and top-k lists must EQUAL the reference at every edge of the kernels;
(b) top-k bookkeeping: k on both sides of the list layouts and above M,
    exclusion lists, a query with everything excluded, the squared-L2 code,
    and agreement with the raw ranks;
(c) float tables inside relation_rank_envelope's derived fp32 bounds;
(d) the same bytes on two calls, and RESCAL's score matrix filled in passes;
(e) the Python layer.
"""
import functools

import numpy as np
import pytest
import torch

import eval_ref as X
import relation_ref as RR

pytestmark = pytest.mark.gpu

KS = (1, 10, 64, 65, 128)
# top-k: the cases whose reference sort stays quick, and M = 4500 at two k
TOPK_CASES = [c for c in RR.INT_CASES if c[3] * c[4] <= 300000]
BIG_TOPK = [c for c in RR.INT_CASES if c[3] == 4500]


def _code(model):
    from skge_amd import _lib as L
    return {"transe": L.SKGE_TRANSE_L1, "hole": L.SKGE_HOLE, "rescal": L.SKGE_RESCAL}[model]


def _dev(a, dtype):
    return torch.as_tensor(np.array(a, dtype=dtype), device="cuda:0")     # a writable copy


def _csr(mask):
    """(offsets [n + 1], ids) int32 on the device from a [n, M] bool mask."""
    off = np.concatenate([[0], np.cumsum(mask.sum(axis=1))])
    ids = np.nonzero(mask)[1]
    return _dev(off, np.int32), _dev(ids if len(ids) else [0], np.int32)


class Tables(object):
    def __init__(self, E, R):
        self.N, self.d = E.shape
        self.M = R.shape[0]
        self.E, self.R = _dev(E, np.float32), _dev(R, np.float32)

    def ranks(self, code, test, csr=None):
        from skge_amd import _lib as L
        lib = L.lib()
        q = _dev(test, np.int32)
        nq = len(test)
        out = torch.full((nq, 2), -7, dtype=torch.int32, device="cuda:0")
        nbytes = lib.skge_relrank_workspace_bytes(nq, self.d, self.M, code)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        L.check(lib.skge_relrank(L.stream_ptr(), code, L.ptr(self.E), L.ptr(self.R), self.N,
                                 self.M, self.d, L.ptr(q), nq,
                                 L.ptr(csr[0]) if csr else None, L.ptr(csr[1]) if csr else None,
                                 L.ptr(ws), nbytes, L.ptr(out)), "relrank")
        return out.cpu().numpy().astype(np.int64)

    def topk(self, code, pairs, k, csr=None):
        from skge_amd import _lib as L
        lib = L.lib()
        q = _dev(pairs, np.int32)
        nq = len(pairs)
        ids = torch.full((nq, k), -7, dtype=torch.int32, device="cuda:0")
        val = torch.full((nq, k), np.nan, dtype=torch.float32, device="cuda:0")
        nbytes = lib.skge_reltopk_workspace_bytes(nq, self.d, k, self.M, code)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        L.check(lib.skge_reltopk(L.stream_ptr(), code, L.ptr(self.E), L.ptr(self.R), self.N,
                                 self.M, self.d, L.ptr(q), nq, k,
                                 L.ptr(csr[0]) if csr else None, L.ptr(csr[1]) if csr else None,
                                 L.ptr(ws), nbytes, L.ptr(ids), L.ptr(val)), "reltopk")
        return ids.cpu().numpy().astype(np.int64), val.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _int_ref(model, d, N, M, nq):
    """The case, its score matrix, its exact ranks and its filter mask, once."""
    E, R, test, known = RR.int_case(model, d, N, M, nq)
    sc = RR.int_relation_scores(model, E, R, test[:, :2])
    exact = RR.ranks_of_scores(sc, test, known)
    mask = RR.known_mask(test, known, M)
    for a in (E, R, test, known, sc, exact, mask):
        a.setflags(write=False)
    return E, R, test, known, sc, exact, mask


def _assert_topk(got, want, msg):
    np.testing.assert_array_equal(got[0], want[0], err_msg="ids, " + msg)
    np.testing.assert_array_equal(got[1].astype(np.float64), want[1], err_msg="scores, " + msg)


# ---------------------------------------------------------------------------
# (a) exact equality on integer tables
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("model,d,N,M,nq", RR.INT_CASES)
def test_int_ranks_exact(model, d, N, M, nq):
    E, R, test, known, sc, exact, mask = _int_ref(model, d, N, M, nq)
    t = Tables(E, R)
    got = t.ranks(_code(model), test, _csr(mask))
    np.testing.assert_array_equal(got, exact)
    raw = t.ranks(_code(model), test)
    np.testing.assert_array_equal(raw, np.stack([exact[:, 0], exact[:, 0]], axis=1))


def _topk_check(model, case, ks):
    E, R, test, known, sc, exact, mask = _int_ref(model, *case)
    M = case[2]
    t = Tables(E, R)
    pairs = test[:, :2]
    full = mask.copy()
    full[np.arange(len(test)), test[:, 2]] = True      # every known relation of the pair
    excl = [np.flatnonzero(r) for r in full]
    kmax = max(ks)
    for csr, ex, tag in ((None, None, "raw"), (_csr(full), excl, "excluded")):
        ids, val = RR.T.topk_of_scores(sc, kmax, ex)
        for k in ks:
            got = t.topk(_code(model), pairs, k, csr)
            _assert_topk(got, (ids[:, :k], val[:, :k]), "%s k=%d" % (tag, k))
        if ex is None and kmax > M:
            assert (ids[:, M:] == -1).all() and np.isneginf(val[:, M:]).all()    # k > M pads
            # the entries strictly above the true relation's score: rank_raw - 1
            true = sc[np.arange(len(test)), test[:, 2]].astype(np.float64)
            np.testing.assert_array_equal((got[1] > true[:, None]).sum(axis=1), exact[:, 0] - 1)
        if ex is not None and M >= 8:
            assert (ids != RR.T.topk_of_scores(sc, kmax, None)[0]).any()   # the lists mattered


@pytest.mark.parametrize("model,d,N,M,nq", TOPK_CASES)
def test_int_topk_exact(model, d, N, M, nq):
    _topk_check(model, (d, N, M, nq), KS)


@pytest.mark.parametrize("model,d,N,M,nq", BIG_TOPK)
def test_int_topk_exact_multi_tile_slices(model, d, N, M, nq):
    _topk_check(model, (d, N, M, nq), (10, 128))


# ---------------------------------------------------------------------------
# (b) exclusions that leave nothing; the squared-L2 code
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("model", RR.MODELS)
def test_everything_excluded_gives_padding(model):
    E, R, test, known, sc, exact, mask = _int_ref(model, 33, 50, 65, 64)
    t = Tables(E, R)
    full = np.zeros_like(mask)
    full[::3] = True                     # every third query: all 65 relations excluded
    full[1::3, ::2] = True
    excl = [np.flatnonzero(r) for r in full]
    for k in (10, 65, 128):
        ids, val = t.topk(_code(model), test[:, :2], k, _csr(full))
        assert (ids[::3] == -1).all() and np.isneginf(val[::3]).all()
        _assert_topk((ids, val), RR.T.topk_of_scores(sc, k, excl), "k=%d" % k)
        assert (ids[2::3, :min(k, 65)] >= 0).all()


def test_squared_l2_orders_topk_but_ranks_stay_l1():
    from skge_amd import _lib as L
    E, R, test, known, sc, exact, mask = _int_ref("transe", 33, 50, 65, 64)
    t = Tables(E, R)
    pairs = test[:, :2]
    want2 = RR.exact_relation_topk("transe", E, R, pairs, 10, l2=True)
    want1 = RR.exact_relation_topk("transe", E, R, pairs, 10)
    got2 = t.topk(L.SKGE_TRANSE_L2, pairs, 10)
    got1 = t.topk(L.SKGE_TRANSE_L1, pairs, 10)
    _assert_topk(got2, want2, "L2")
    _assert_topk(got1, want1, "L1")
    assert (got1[0] != got2[0]).any(axis=1).any()
    np.testing.assert_array_equal(t.ranks(L.SKGE_TRANSE_L2, test, _csr(mask)), exact)


# ---------------------------------------------------------------------------
# (c) float tables inside the derived fp32 envelope
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _float_ref(model, d, scale):
    E, R, test, known = RR.float_case(model, d, scale)
    lo, hi = RR.relation_rank_envelope(model, E, R, test, known)
    return E, R, test, known, lo, hi


@pytest.mark.parametrize("model,d,scale", RR.FLOAT_CASES)
def test_float_tables_inside_envelope(model, d, scale):
    E, R, test, known, lo, hi = _float_ref(model, d, scale)
    got = Tables(E, R).ranks(_code(model), test, _csr(RR.known_mask(test, known, R.shape[0])))
    print("%s d=%d scale=%g: pinned %.3f, at lo %.3f" % (model, d, scale, (lo == hi).mean(),
                                                         (got == lo).mean()))
    assert (lo <= got).all() and (got <= hi).all(), np.argwhere((got < lo) | (got > hi))[:5]


# ---------------------------------------------------------------------------
# (d) determinism; RESCAL's matrix in passes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("model", RR.MODELS)
def test_two_calls_return_the_same_bytes(model):
    E, R, test, known, lo, hi = _float_ref(model, {"transe": 40, "hole": 33, "rescal": 37}[model],
                                           8.0)
    t = Tables(E, R)
    csr = _csr(RR.known_mask(test, known, R.shape[0]))
    r1, r2 = t.ranks(_code(model), test, csr), t.ranks(_code(model), test, csr)
    assert r1.tobytes() == r2.tobytes()
    a, b = t.topk(_code(model), test[:, :2], 40), t.topk(_code(model), test[:, :2], 40)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert np.isfinite(a[1]).all()


def test_rescal_score_matrix_in_passes(monkeypatch):
    """SKGE_REL_SCORE_BYTES caps the score matrix at 256 rows of M = 129: the
    2048 queries take eight passes and give the one-pass result."""
    from skge_amd import _lib as L
    E, R, test, known, sc, exact, mask = _int_ref("rescal", 5, 50, 129, 2048)
    t = Tables(E, R)
    lib = L.lib()
    one = lib.skge_relrank_workspace_bytes(2048, 5, 129, L.SKGE_RESCAL)
    monkeypatch.setenv("SKGE_REL_SCORE_BYTES", str(256 * 129 * 4))
    assert lib.skge_relrank_workspace_bytes(2048, 5, 129, L.SKGE_RESCAL) < one // 4
    np.testing.assert_array_equal(t.ranks(L.SKGE_RESCAL, test, _csr(mask)), exact)
    full = mask.copy()
    full[np.arange(len(test)), test[:, 2]] = True
    _assert_topk(t.topk(L.SKGE_RESCAL, test[:, :2], 10, _csr(full)),
                 RR.T.topk_of_scores(sc, 10, [np.flatnonzero(r) for r in full]), "passes")


# ---------------------------------------------------------------------------
# (e) the Python layer
# ---------------------------------------------------------------------------

def _model(name, E, R, **kw):
    import skge_amd as S
    n_ent, d = E.shape
    m = {"transe": S.TransE, "hole": S.HolE, "rescal": S.RESCAL}[name](
        (n_ent, n_ent, R.shape[0]), d, init="device_nunif", **kw)
    rid = "W" if name == "rescal" else "R"
    m.params["E"].data.copy_(torch.tensor(E, dtype=torch.float32))
    m.params[rid].data.copy_(torch.tensor(R, dtype=torch.float32))
    return m


@pytest.mark.parametrize("model", RR.MODELS)
def test_evaluator_relation_ranks_positions_and_scores(model):
    import skge_amd as S
    E, R, test, known, sc, exact, mask = _int_ref(model, 33, 50, 65, 64)
    m = _model(model, E, R)
    ev = S.FilteredRankingEval(np.array(test), np.array(known))
    order = X.eval_order(test)
    want = RR.exact_relation_ranks(model, E, R, order, known)
    assert (order != test).any()                   # the evaluator's order is not the input's
    got = ev.relation_ranks(m)
    assert got.dtype == np.int64 and got.shape == (len(test), 2)
    np.testing.assert_array_equal(got, want)
    assert ev.last_relation_ranks is got
    pos, fpos = ev.relation_positions(m)
    assert list(pos) == list(ev.idx) == list(fpos)
    k = 0
    for p in pos:
        n = len(ev.idx[p])
        assert set(pos[p]) == set(fpos[p]) == {"rel"}
        assert pos[p]["rel"] == want[k:k + n, 0].tolist()
        assert fpos[p]["rel"] == want[k:k + n, 1].tolist()
        k += n
    assert k == len(test)
    for hits in (1, 3):
        raw, filt = S.relation_ranking_scores(pos, fpos, hits=hits)
        assert raw == S.compute_scores(want[:, 0], hits)
        assert filt == S.compute_scores(want[:, 1], hits)
    assert S.relation_ranking_scores(pos, fpos) == S.relation_ranking_scores(pos, fpos, hits=1)
    assert ev.ranks(m).shape == (len(test), 4)     # the entity ranks are still there


def test_link_predictor_relations():
    import skge_amd as S
    E, R, test, known, sc, exact, mask = _int_ref("hole", 33, 50, 65, 64)
    M = 65
    m = _model("hole", E, R)
    lp = S.LinkPredictor(m, known)
    pairs = test[:, :2]
    every = RR.pair_relations(pairs, known)
    rels, scores = lp.relations(pairs[:, 0], pairs[:, 1], k=10)
    assert rels.dtype == np.int64 and scores.dtype == np.float32
    assert rels.shape == scores.shape == (len(test), 10)
    _assert_topk((rels, scores), RR.exact_relation_topk("hole", E, R, pairs, 10, every), "filtered")
    raw = lp.relations(pairs[:, 0], pairs[:, 1], filtered=False)           # default k = 10
    _assert_topk(raw, RR.exact_relation_topk("hole", E, R, pairs, 10), "raw")
    assert (raw[0] != rels).any()
    # a scalar pair is one row; exclude merges with the filter
    s, o = int(pairs[0, 0]), int(pairs[0, 1])
    one = lp.relations(s, o, k=5)
    assert one[0].shape == (1, 5) and (one[0][0] == rels[0, :5]).all()
    extra = [int(one[0][0, 0]), int(one[0][0, 2]), int(one[0][0, 0])]
    both = lp.relations(s, o, k=5, exclude=extra)
    _assert_topk(both, RR.exact_relation_topk("hole", E, R, pairs[:1], 5,
                                              [np.union1d(every[0], extra)]), "merged")
    two = lp.relations([s, s], [o, o], k=70, filtered=False, exclude=[None, range(0, M, 2)])
    _assert_topk(two, RR.exact_relation_topk("hole", E, R, [(s, o), (s, o)], 70,
                                             [[], np.arange(0, M, 2)]), "per-query exclude")
    assert (two[0][0, M:] == -1).all() and np.isneginf(two[1][0, M:]).all()
    # refusals come before any launch
    with pytest.raises(ValueError, match="known_triples"):
        S.LinkPredictor(m).relations(s, o)
    with pytest.raises(ValueError, match="subject 50"):
        lp.relations(50, o)
    with pytest.raises(ValueError, match="object -1"):
        lp.relations(s, -1)
    with pytest.raises(ValueError, match="relation 65"):
        lp.relations(s, o, exclude=[M])
    for k in (0, 129, True):
        with pytest.raises(ValueError, match="k must be"):
            lp.relations(s, o, k=k)
    bad = np.array(test)
    bad[3, 2] = M
    with pytest.raises(ValueError, match="p=65.* out of range"):
        S.FilteredRankingEval(bad, known).relation_ranks(m)


def test_link_predictor_relations_scoring_modes():
    """TransE(l1=False): scoring='model' orders by the squared distance,
    scoring='eval' by the evaluator's L1."""
    import skge_amd as S
    E, R, test, known, sc, exact, mask = _int_ref("transe", 33, 50, 65, 64)
    m = _model("transe", E, R, l1=False)
    pairs = test[:, :2]
    got2 = S.LinkPredictor(m, scoring="model").relations(pairs[:, 0], pairs[:, 1], k=10,
                                                         filtered=False)
    got1 = S.LinkPredictor(m, scoring="eval").relations(pairs[:, 0], pairs[:, 1], k=10,
                                                        filtered=False)
    _assert_topk(got2, RR.exact_relation_topk("transe", E, R, pairs, 10, l2=True), "model")
    _assert_topk(got1, RR.exact_relation_topk("transe", E, R, pairs, 10), "eval")
    assert (got1[0] != got2[0]).any()
