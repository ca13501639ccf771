"""Device filtered ranking (skge_rank_known, and skge_rank under
SKGE_RANK_SET=1) against the references of tests/eval_ref.py:

(a) integer tables, where fp32, fp64 and int64 scores agree bit for bit, so
    all four rank columns must EQUAL exact_ranks -- at every edge of the
    kernels (d < 4, the scalar tail, the 32-dim chunk boundary, d = 1024, N
    around the 64- / 128-entity tiles, N = 1, full and one-over query blocks,
    ragged multi-tile entity slices, the single slice with the query kernel's
    grid-stride loop);
(b) ties and the filter's bookkeeping, by construction;
(c) float tables, where the ranks must lie inside rank_envelope's derived
    fp32 interval (the bounded counterpart of test_gpu_eval's 99% / +-2).
"""
import functools

import numpy as np
import pytest
import torch

import eval_ref as X
from oracle import skge_oracle as O

pytestmark = pytest.mark.gpu

FORMS = ["known", "set"]   # skge_rank_known (the default), skge_rank (SKGE_RANK_SET=1)
MODELS = ["transe", "hole", "rescal"]


def _model(name, E, R, **kw):
    """The model with the given tables (as test_gpu_eval._model copies them).
    The device initialiser keeps a length-1 axis (N = 1, d = 1), which the
    host one squeezes away as the reference's does."""
    import skge_amd as S
    n_ent, d = E.shape
    m = {"transe": S.TransE, "hole": S.HolE, "rescal": S.RESCAL}[name](
        (n_ent, n_ent, R.shape[0]), d, init="device_nunif", **kw)
    rid = "W" if name == "rescal" else "R"
    assert m.params["E"].shape == E.shape and m.params[rid].shape == R.shape
    m.params["E"].data.copy_(torch.tensor(E, dtype=torch.float32))
    m.params[rid].data.copy_(torch.tensor(R, dtype=torch.float32))
    return m


def _evaluator(test, known, form, monkeypatch):
    import skge_amd as S
    monkeypatch.setenv("SKGE_RANK_SET", "1" if form == "set" else "0")
    return S.FilteredRankingEval(np.asarray(test, dtype=np.int32).reshape(-1, 3),
                                 np.asarray(known, dtype=np.int32).reshape(-1, 3))


def _ranks(name, E, R, test, known, form, monkeypatch, **kw):
    return _evaluator(test, known, form, monkeypatch).ranks(_model(name, E, R, **kw))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------
# (a) exact equality on integer tables
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _int_ref(model, d, N, nq):
    """The case and its reference ranks (in the evaluator's order), computed
    once and shared by both forms."""
    E, R, test, known = X.make_int_case(model, d, N, nq, X.case_seed(model, d, N, nq))
    want = X.exact_ranks(model, E, R, X.eval_order(test), known)
    return _frozen(E, R, test, known, want)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("model,d,N,nq", X.INT_CASES)
def test_int_tables_exact(model, d, N, nq, form, monkeypatch):
    E, R, test, known, want = _int_ref(model, d, N, nq)
    got = _ranks(model, E, R, test, known, form, monkeypatch)
    assert got.shape == (nq, 4)
    for col in range(4):
        np.testing.assert_array_equal(got[:, col], want[:, col], err_msg="column %d" % col)
    if N >= 63:   # the filter removed known answers (with fewer entities none may outscore)
        assert (got[:, 1] < got[:, 0]).any() or (got[:, 3] < got[:, 2]).any()
    if N == 1:
        assert (got == 1).all()


@pytest.mark.parametrize("form", FORMS)
def test_l2_trained_transe_is_ranked_with_l1(form, monkeypatch):
    """A TransE(l1=False) model gets the L1 positions: the reference's
    evaluator scores -sum|E[s] + R[p] - E| and -sum|E + R[p] - E[o]|
    (skge/run_transe.py:24 and :29, TransEEval.scores_o / scores_s) whatever
    norm the model was trained with (run_transe.py:40-41 passes l1 to the
    model only)."""
    E, R, test, known, want = _int_ref("transe", 33, 65, 33)
    got = _ranks("transe", E, R, test, known, form, monkeypatch, l1=False)
    np.testing.assert_array_equal(got, want)
    # ... and they are not the squared-L2 positions
    q = X.eval_order(test)
    l2 = np.array([1 + np.sum(-((E[s] + R[p] - E) ** 2).sum(1) > -((E[s] + R[p] - E[o]) ** 2).sum())
                   for s, o, p in q.tolist()])
    assert (l2 != want[:, 0]).any()


# ---------------------------------------------------------------------------
# (b) ties and filter bookkeeping: N = 70, d = 5, integer tables
# ---------------------------------------------------------------------------
N_B, D_B, M_B = 70, 5, 3


def _tables_b(model, seed):
    rs = np.random.RandomState(seed)
    E = rs.randint(-3, 4, size=(N_B, D_B)).astype(np.float64)
    R = rs.randint(-3, 4, size=X.rel_shape(model, M_B, D_B)).astype(np.float64)
    return rs, E, R


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("model", MODELS)
def test_identical_entity_rows_all_rank_one(model, form, monkeypatch):
    rs, E, R = _tables_b(model, 11)
    E[:] = E[0]
    test, known = X.random_triples(rs, N_B, M_B, 40)
    got = _ranks(model, E, R, test, known, form, monkeypatch)
    np.testing.assert_array_equal(got, np.ones((40, 4), dtype=np.int64))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("model", MODELS)
def test_copies_of_the_true_row_do_not_count(model, form, monkeypatch):
    """Five entities hold a copy of the true tail's row and five a copy of the
    true head's: they tie the true score exactly and leave every position
    where it is without them."""
    rs, E, R = _tables_b(model, 12)
    s, o = 3, 8
    tcopies, hcopies = [10, 20, 30, 40, 69], [11, 21, 31, 41, 0]
    E[tcopies] = E[o]
    E[hcopies] = E[s]
    test = np.array([(s, o, p) for p in range(M_B)])
    known = np.concatenate([test, [(s, j, p) for p in range(M_B) for j in (10, 15, 50)],
                            [(j, o, p) for p in range(M_B) for j in (11, 16, 51)]])
    got = _ranks(model, E, R, test, known, form, monkeypatch)
    np.testing.assert_array_equal(got, X.exact_ranks(model, E, R, test, known))
    for i, p in enumerate(range(M_B)):
        st = X.int_scores(model, E, R, s, o, p, "tail")
        sh = X.int_scores(model, E, R, s, o, p, "head")
        assert (st[tcopies] == st[o]).all() and (sh[hcopies] == sh[s]).all()
        rest_t = np.setdiff1d(np.arange(N_B), tcopies)
        rest_h = np.setdiff1d(np.arange(N_B), hcopies)
        assert got[i, 0] == 1 + (st[rest_t] > st[o]).sum()
        assert got[i, 2] == 1 + (sh[rest_h] > sh[s]).sum()


def _hand_placed(model):
    """One query whose true tail and head score in the middle, with a copy of
    each true row elsewhere, and entities picked by score: strictly better,
    the exact copy, worse."""
    rs, E, R = _tables_b(model, 13)
    s, p = 5, 1
    st = X.int_scores(model, E, R, s, 0, p, "tail")
    o = int([j for j in np.argsort(st, kind="stable") if j != s][N_B // 2])
    tcopy, hcopy = [j for j in range(N_B) if j not in (s, o)][:2]
    E[tcopy] = E[o]
    E[hcopy] = E[s]
    st = X.int_scores(model, E, R, s, o, p, "tail")
    sh = X.int_scores(model, E, R, s, o, p, "head")
    pick = lambda sc, t, better: [int(j) for j in range(N_B) if j not in (s, o, tcopy, hcopy)
                                  and (sc[j] > sc[t] if better else sc[j] < sc[t])][:3]
    sets = dict(bt=pick(st, o, True), wt=pick(st, o, False), bh=pick(sh, s, True)[:2],
                wh=pick(sh, s, False))
    assert len(sets["bt"]) == 3 and len(sets["bh"]) == 2 and sets["wt"] and sets["wh"]
    assert st[tcopy] == st[o] and sh[hcopy] == sh[s]
    raw_t, raw_h = 1 + int((st > st[o]).sum()), 1 + int((sh > sh[s]).sum())
    answers = [(s, j, p) for j in sets["bt"] + [tcopy] + sets["wt"]] + \
              [(j, o, p) for j in sets["bh"] + [hcopy] + sets["wh"]]
    # answers of other queries, which must not count: another relation, another subject
    others = [(s, sets["bt"][0], (p + 1) % M_B), (s + 1, sets["bt"][1], p),
              (sets["bh"][0], o, (p + 1) % M_B), (sets["bh"][1], o + 1, p)]
    return E, R, (s, o, p), answers, others, (raw_t, raw_h)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("variant", ["with_query", "without_query", "duplicates", "empty"])
@pytest.mark.parametrize("model", MODELS)
def test_hand_placed_known_answers(model, variant, form, monkeypatch):
    """Each strictly better known answer takes one off the raw position (3
    tails, 2 heads); the exact copy of the true row, the worse answers and
    other queries' answers change nothing -- whether or not the known list
    holds the test triple itself, with duplicate rows, and with no known
    triples at all."""
    E, R, query, answers, others, (raw_t, raw_h) = _hand_placed(model)
    known = {"with_query": [query] + answers + others,
             "without_query": answers + others,
             "duplicates": [query] + answers + others + answers[::2] + [query] + answers,
             "empty": []}[variant]
    known = np.asarray(known, dtype=np.int64).reshape(-1, 3)
    got = _ranks(model, E, R, [query], known, form, monkeypatch)
    dt, dh = (0, 0) if variant == "empty" else (3, 2)
    np.testing.assert_array_equal(got, [[raw_t, raw_t - dt, raw_h, raw_h - dh]])
    np.testing.assert_array_equal(got, X.exact_ranks(model, E, R, [query], known))


def _shared_queries(model):
    """Test triples with duplicates, groups sharing (s, p) and (o, p), and
    self-loops, over all relations out of order."""
    rs, E, R = _tables_b(model, 14)
    test = [(4, 9, 2), (4, 17, 2), (4, 33, 2), (4, 9, 2),       # share (s, p); one duplicate
            (12, 6, 0), (25, 6, 0), (41, 6, 0),                # share (o, p)
            (7, 7, 1), (30, 30, 2), (7, 7, 1),                 # self-loops, one duplicate
            (4, 6, 0), (12, 6, 0), (69, 0, 1), (0, 69, 2)]
    test = np.asarray(test, dtype=np.int64)
    extra = np.stack([rs.randint(N_B, size=400), rs.randint(N_B, size=400),
                      rs.randint(M_B, size=400)], axis=1)
    extra[:150, 0], extra[:150, 2] = 4, 2      # many tails of (4, ?, 2) ...
    extra[150:300, 1], extra[150:300, 2] = 6, 0    # ... and heads of (?, 6, 0)
    known = np.concatenate([test, extra, [(7, j, 1) for j in range(0, N_B, 3)],
                            [(j, 7, 1) for j in range(1, N_B, 3)]])
    return E, R, test, known


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("model", MODELS)
def test_duplicate_shared_and_self_loop_queries(model, form, monkeypatch):
    E, R, test, known = _shared_queries(model)
    q = X.eval_order(test)
    want = X.exact_ranks(model, E, R, q, known)
    assert (want[:, 1] < want[:, 0]).any() and (want[:, 3] < want[:, 2]).any()
    got = _ranks(model, E, R, test, known, form, monkeypatch)
    np.testing.assert_array_equal(got, want)
    rows = {}
    for triple, r in zip(map(tuple, q.tolist()), got.tolist()):
        assert rows.setdefault(triple, r) == r     # duplicates get the same positions


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("model", MODELS)
def test_positions_structure_and_ranking_scores(model, form, monkeypatch):
    """positions() is ({p: {'head': [...], 'tail': [...]}}, the same filtered)
    with the relations in the evaluator's order, and ranking_scores of it is
    oracle.compute_scores of the reference's columns, concatenated per
    relation as head then tail -- exactly."""
    import skge_amd as S
    E, R, test, known = _shared_queries(model)
    q = X.eval_order(test)
    want = X.exact_ranks(model, E, R, q, known)
    ev = _evaluator(test, known, form, monkeypatch)
    pos, fpos = ev.positions(_model(model, E, R))
    assert list(pos) == list(fpos) == [2, 0, 1] == list(ev.idx)
    raw, filt = [], []
    for p in pos:
        assert set(pos[p]) == set(fpos[p]) == {"head", "tail"}
        rows = want[q[:, 2] == p]
        assert pos[p]["tail"] == rows[:, 0].tolist() and fpos[p]["tail"] == rows[:, 1].tolist()
        assert pos[p]["head"] == rows[:, 2].tolist() and fpos[p]["head"] == rows[:, 3].tolist()
        raw += rows[:, 2].tolist() + rows[:, 0].tolist()
        filt += rows[:, 3].tolist() + rows[:, 1].tolist()
    assert S.ranking_scores(pos, fpos) == (O.compute_scores(raw), O.compute_scores(filt))


# ---------------------------------------------------------------------------
# (c) float tables inside the derived fp32 envelope
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _float_ref(model, d, scale):
    E, R, test, known = X.make_float_case(model, d, scale, X.case_seed(model, d, scale))
    lo, hi = X.rank_envelope(model, E, R, X.eval_order(test), known)
    return _frozen(E, R, test, known, lo, hi)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("model,d,scale", X.FLOAT_CASES)
def test_float_tables_inside_envelope(model, d, scale, form, monkeypatch):
    E, R, test, known, lo, hi = _float_ref(model, d, scale)
    got = _ranks(model, E, R, test, known, form, monkeypatch)
    out = (got < lo) | (got > hi)
    print("%s d=%d scale=%g %s: %d of %d outside; %d entries with hi == lo"
          % (model, d, scale, form, out.sum(), out.size, (hi == lo).sum()))
    assert not out.any(), (np.argwhere(out)[:5].tolist(), got[out][:5], lo[out][:5], hi[out][:5])
