"""DistMult and ComplEx evaluation on the device against the integer-exact
references (eval_ref, relation_ref, topk_ref, pool_ref with their "distmult" /
"complex" branches).  On integer tables with entries in [-3, 3] every fp32
product, fma and partial sum is an exact integer (eval_ref.int_diag_mul), so
nothing here is a tolerance: ranks, ids and scores must EQUAL the int64 ones,
exact ties and their id order included.  A float envelope passes a conjugate
on the wrong operand inside a near-tie; equality does not.

(a) filtered ranks in both forms, relation ranks, top-k tails / heads /
    relations, pool ranks and raw scores at every d edge of query_elem and
    k_score_diag (tests/test_diag_int_ref.py holds the case lists and judges
    them on the CPU);
(b) test_gpu_eval_exact's tie and filter constructions at width 6;
(c) device against device at d = 66 and 130: ComplEx with zero imaginary parts
    is DistMult on the real halves, and swapping s and o under the conjugate
    relation swaps the tail and head columns.
"""
import numpy as np
import pytest
import torch

import eval_ref as X
import pool_ref as PR
import relation_ref as RR
import test_diag_int_ref as TI
import test_gpu_eval_exact as TE
import topk_ref as T

pytestmark = pytest.mark.gpu

FORMS = TE.FORMS
MODELS = ["distmult", "complex"]
K = 5


def _model(name, E, R):
    import skge_amd as S
    n_ent, d = E.shape
    m = {"distmult": S.DistMult, "complex": S.ComplEx}[name](
        (n_ent, n_ent, R.shape[0]), d, init="device_nunif")
    assert m.params["E"].shape == E.shape and m.params["R"].shape == R.shape
    m.params["E"].data.copy_(torch.tensor(E, dtype=torch.float32))
    m.params["R"].data.copy_(torch.tensor(R, dtype=torch.float32))
    return m


def _ranks(name, E, R, test, known, form, monkeypatch):
    return TE._evaluator(test, known, form, monkeypatch).ranks(_model(name, E, R))


def _assert_topk(got, want, what):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32
    np.testing.assert_array_equal(got[0], want[0], err_msg="ids, " + what)
    np.testing.assert_array_equal(got[1].astype(np.float64), want[1], err_msg="scores, " + what)


# ---------------------------------------------------------------------------
# (a) equality at every edge
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("model,d,N,nq", TI.INT_CASES)
def test_ranks_equal_reference(model, d, N, nq, form, monkeypatch):
    E, R, test, known = TI.entity_case(model, d, N, nq)
    want = X.exact_ranks(model, E, R, X.eval_order(test), known)
    got = _ranks(model, E, R, test, known, form, monkeypatch)
    assert got.shape == (nq, 4)
    for col in range(4):
        np.testing.assert_array_equal(got[:, col], want[:, col], err_msg="column %d" % col)


@pytest.mark.parametrize("model,d,N,nq", TI.INT_CASES)
def test_relation_ranks_and_topk_equal_reference(model, d, N, nq):
    """the relation query reuses query_elem's head form with swapped arguments"""
    import skge_amd as S
    E, R, test, known = TI.relation_case(model, d, N, nq)
    m = _model(model, E, R)
    got = S.FilteredRankingEval(np.array(test), np.array(known)).relation_ranks(m)
    np.testing.assert_array_equal(got, RR.exact_relation_ranks(model, E, R, X.eval_order(test),
                                                               known))
    lp = S.LinkPredictor(m, known)
    pairs = test[:, :2]
    for flt in (False, True):
        excl = RR.pair_relations(pairs, known) if flt else None
        _assert_topk(lp.relations(pairs[:, 0], pairs[:, 1], k=K, filtered=flt),
                     RR.exact_relation_topk(model, E, R, pairs, K, excl), "filtered=%s" % flt)


@pytest.mark.parametrize("model,d,N,nq", TI.INT_CASES)
def test_topk_and_scores_equal_reference(model, d, N, nq):
    import skge_amd as S
    E, R, test, known = TI.entity_case(model, d, N, nq)
    m = _model(model, E, R)
    lp = S.LinkPredictor(m, known)
    for direction, fn, q in (("tail", lp.tails, test[:, [0, 2]]), ("head", lp.heads, test[:, [1, 2]])):
        for flt in (False, True):
            excl = T.known_answers(q, known, direction) if flt else None
            _assert_topk(fn(q[:, 0], q[:, 1], k=K, filtered=flt),
                         T.exact_topk(model, E, R, q, direction, K, excl),
                         "%s filtered=%s" % (direction, flt))
    # k_score_diag on 300 triples: the int64 score
    rs = np.random.RandomState(d + N)
    trip = np.stack([rs.randint(N, size=300), rs.randint(N, size=300),
                     rs.randint(TI.M_ENT, size=300)], axis=1).astype(np.int32)
    Ei, Ri = X._int_tables(E, R)
    want = (X.int_diag_mul(model, Ei[trip[:, 0]], Ri[trip[:, 2]], False) * Ei[trip[:, 1]]).sum(1)
    got = m.score(trip).cpu().numpy()
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("model,d,N,nq", TI.POOL_CASES)
def test_pool_ranks_equal_reference(model, d, N, nq, monkeypatch):
    """candidate_ranks over `mixed` pools (pool -1, the typed pools, hand-made
    ones) and typed_ranks over the type index of the known triples"""
    E, R, test, known = TI.entity_case(model, d, N, nq)
    order = X.eval_order(test)
    seed = X.case_seed("diag-pools", model, d, N, nq)
    pools, vp = PR.make_pools("mixed", np.random.RandomState(seed), N, TI.M_ENT, order, known)
    vp = np.asarray(vp, dtype=np.int64)
    ev = TE._evaluator(test, known, "known", monkeypatch)
    m = _model(model, E, R)
    got = ev.candidate_ranks(m, pools, vp[0::2], vp[1::2])
    np.testing.assert_array_equal(got, PR.exact_pool_ranks(model, E, R, order, known, pools, vp))
    tp = PR.type_pools_of(known, TI.M_ENT)
    np.testing.assert_array_equal(
        ev.typed_ranks(m), PR.exact_pool_ranks(model, E, R, order, known, tp,
                                               PR.typed_vec_pool(order)))


# ---------------------------------------------------------------------------
# (b) ties and filter bookkeeping: test_gpu_eval_exact's constructions, N = 70,
#     integer tables of width 6 (even, so that ComplEx runs)
# ---------------------------------------------------------------------------

@pytest.fixture
def width6(monkeypatch):
    monkeypatch.setattr(TE, "D_B", 6)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("model", MODELS)
def test_identical_entity_rows_all_rank_one(model, form, monkeypatch, width6):
    rs, E, R = TE._tables_b(model, 11)
    assert E.shape == (TE.N_B, 6)
    E[:] = E[0]
    test, known = X.random_triples(rs, TE.N_B, TE.M_B, 40)
    got = _ranks(model, E, R, test, known, form, monkeypatch)
    np.testing.assert_array_equal(got, np.ones((40, 4), dtype=np.int64))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("model", MODELS)
def test_copies_of_the_true_row_do_not_count(model, form, monkeypatch, width6):
    rs, E, R = TE._tables_b(model, 12)
    s, o = 3, 8
    tcopies, hcopies = [10, 20, 30, 40, 69], [11, 21, 31, 41, 0]
    E[tcopies] = E[o]
    E[hcopies] = E[s]
    test = np.array([(s, o, p) for p in range(TE.M_B)])
    known = np.concatenate([test, [(s, j, p) for p in range(TE.M_B) for j in (10, 15, 50)],
                            [(j, o, p) for p in range(TE.M_B) for j in (11, 16, 51)]])
    got = _ranks(model, E, R, test, known, form, monkeypatch)
    np.testing.assert_array_equal(got, X.exact_ranks(model, E, R, test, known))
    for i, p in enumerate(range(TE.M_B)):
        st = X.int_scores(model, E, R, s, o, p, "tail")
        sh = X.int_scores(model, E, R, s, o, p, "head")
        assert (st[tcopies] == st[o]).all() and (sh[hcopies] == sh[s]).all()
        rest_t = np.setdiff1d(np.arange(TE.N_B), tcopies)
        rest_h = np.setdiff1d(np.arange(TE.N_B), hcopies)
        assert got[i, 0] == 1 + (st[rest_t] > st[o]).sum()
        assert got[i, 2] == 1 + (sh[rest_h] > sh[s]).sum()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("variant", ["with_query", "without_query", "duplicates", "empty"])
@pytest.mark.parametrize("model", MODELS)
def test_hand_placed_known_answers(model, variant, form, monkeypatch, width6):
    E, R, query, answers, others, (raw_t, raw_h) = TE._hand_placed(model)
    assert E.shape[1] == 6
    known = {"with_query": [query] + answers + others,
             "without_query": answers + others,
             "duplicates": [query] + answers + others + answers[::2] + [query] + answers,
             "empty": []}[variant]
    known = np.asarray(known, dtype=np.int64).reshape(-1, 3)
    got = _ranks(model, E, R, [query], known, form, monkeypatch)
    dt, dh = (0, 0) if variant == "empty" else (3, 2)
    np.testing.assert_array_equal(got, [[raw_t, raw_t - dt, raw_h, raw_h - dh]])
    np.testing.assert_array_equal(got, X.exact_ranks(model, E, R, [query], known))


# ---------------------------------------------------------------------------
# (c) the models' identities, device against device, bit for bit
# ---------------------------------------------------------------------------

def _everything(name, E, R, test, known):
    """ranks, raw scores of the test triples and the top-k lists of one model"""
    import skge_amd as S
    m = _model(name, E, R)
    test = np.asarray(test, dtype=np.int32)
    ev = S.FilteredRankingEval(test, np.asarray(known, dtype=np.int32))
    lp = S.LinkPredictor(m, known)
    return {"ranks": ev.ranks(m), "rel": ev.relation_ranks(m),
            "score": m.score(test).cpu().numpy(),
            "tails": lp.tails(test[:, 0], test[:, 2], k=K, filtered=False),
            "heads": lp.heads(test[:, 1], test[:, 2], k=K, filtered=False)}


@pytest.mark.parametrize("d", [66, 130])
def test_complex_with_zero_imaginary_parts_is_distmult_on_the_device(d):
    E, R, test, known = X.make_int_case("complex", d, 70, 40, X.case_seed("diag-zero", d))
    cx = _everything("complex", *TI.zero_imag(E, R), test, known)
    dm = _everything("distmult", *TI.real_halves(E, R), test, known)
    assert len(np.unique(dm["ranks"][:, 0])) > 3
    for key in ("ranks", "rel", "score"):
        np.testing.assert_array_equal(cx[key], dm[key], err_msg=key)
    for key in ("tails", "heads"):
        np.testing.assert_array_equal(cx[key][0], dm[key][0], err_msg=key)
        np.testing.assert_array_equal(cx[key][1], dm[key][1], err_msg=key)


@pytest.mark.parametrize("d", [66, 130])
@pytest.mark.parametrize("model", MODELS)
def test_swapping_s_and_o_under_the_conjugate_swaps_the_columns(model, d):
    E, R, test, known = X.make_int_case(model, d, 70, 40, X.case_seed("diag-swap", model, d))
    Rc = TI.conj_rows(R) if model == "complex" else R
    a = _everything(model, E, R, test, known)
    b = _everything(model, E, Rc, test[:, [1, 0, 2]], known[:, [1, 0, 2]])
    np.testing.assert_array_equal(b["ranks"][:, [2, 3, 0, 1]], a["ranks"])
    np.testing.assert_array_equal(b["score"], a["score"])
    np.testing.assert_array_equal(b["rel"], a["rel"])
    for x, y in (("tails", "heads"), ("heads", "tails")):
        np.testing.assert_array_equal(b[x][0], a[y][0])
        np.testing.assert_array_equal(b[x][1], a[y][1])
    if model == "complex":     # the conjugate matters: without it the columns differ
        c = _everything(model, E, R, test[:, [1, 0, 2]], known[:, [1, 0, 2]])
        assert (c["ranks"][:, [2, 3, 0, 1]] != a["ranks"]).any()
