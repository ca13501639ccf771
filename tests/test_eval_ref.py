"""The ranking references of tests/eval_ref.py against the oracle and the
reference's golden positions, the envelope's tightness on the float cases of
tests/test_gpu_eval_exact.py, and the evaluator's host-side id check.  No GPU."""
import os

import numpy as np
import pytest

import eval_ref as X
from oracle import skge_oracle as O

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("model", ["transe", "hole"])
def test_envelope_holds_the_reference_positions(model):
    """The golden tables are floats (fp32 values), so the exact form does not
    apply; the envelope must contain the reference's own positions and be a
    single rank almost everywhere."""
    z = np.load(os.path.join(GOLD, "eval_%s.npz" % model))
    E, R = z["E"], z["R"]
    assert (E.astype(np.float32) == E).all() and (R.astype(np.float32) == R).all()
    lo, hi = X.rank_envelope(model, E, R, z["queries"], z["known"])
    gold = np.stack([z["tail_raw"], z["tail_filt"], z["head_raw"], z["head_filt"]], axis=1)
    assert (lo <= gold).all() and (gold <= hi).all()
    assert (lo == hi).mean() >= 0.9


def _int_case(model):
    return X.make_int_case(model, 33, 200, 60, X.case_seed("cpu", model))


@pytest.mark.parametrize("model", ["transe", "hole", "rescal"])
def test_int_scores_equal_rounded_oracle_scores(model):
    E, R, test, _ = _int_case(model)
    for s, o, p in test[:12].tolist():
        for direction in ("tail", "head"):
            got = X.int_scores(model, E, R, s, o, p, direction)
            assert got.dtype == np.int64 and got.shape == (200,)
            want = np.rint(O.entity_scores(model, E, R, s, o, p, direction)).astype(np.int64)
            np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("model", ["transe", "hole", "rescal"])
def test_exact_ranks_equal_oracle_ranks_on_rounded_scores(model, monkeypatch):
    """oracle.filtered_ranks with its scores rounded to the integers they are
    (the FFT leaves +-2e-13 on HolE's, which breaks exact ties at random)."""
    E, R, test, known = _int_case(model)
    plain = O.entity_scores
    monkeypatch.setattr(O, "entity_scores", lambda *a: np.rint(plain(*a)))
    want = O.filtered_ranks(model, E, R, test, known)
    got = X.exact_ranks(model, E, R, test, known)
    np.testing.assert_array_equal(got, want)
    assert (got[:, 1] < got[:, 0]).any() and (got[:, 3] < got[:, 2]).any()


def test_int_scores_refuse_float_tables():
    E, R, test, known = X.make_float_case("transe", 8, 1.0, 3, N=20, M=2, nq=4)
    with pytest.raises(ValueError):
        X.exact_ranks("transe", E, R, test, known)


def test_exact_ranks_tie_rule_and_filter():
    """Hand-checked: ties go the true entity's way, a known answer is skipped
    only when it is not the query itself, raw counts ignore the filter."""
    # TransE, d = 1, R = 0: score of j for (s, ?, p) is -|E_s - E_j|
    E = np.array([[0.0], [0.0], [1.0], [2.0], [0.0]])
    R = np.zeros((1, 1))
    test = [(0, 3, 0)]
    # tail: true o = 3 (score -2); entities 0, 1, 4 (0), 2 (-1) score higher
    # head: true s = 0 (score -2); entities 1, 4 tie, 2 (-1) and 3 (0) score higher
    known = [(0, 3, 0), (0, 2, 0), (0, 1, 0), (3, 3, 0), (1, 3, 0), (0, 2, 0)]
    np.testing.assert_array_equal(X.exact_ranks("transe", E, R, test, known), [[5, 3, 3, 2]])
    np.testing.assert_array_equal(X.exact_ranks("transe", E, R, test, np.zeros((0, 3), int)),
                                  [[5, 5, 3, 3]])
    same = np.ones((6, 3))
    q = [(0, 1, 0), (2, 2, 1), (5, 0, 1)]
    for model, Rr in (("transe", np.ones((2, 3))), ("hole", np.ones((2, 3))),
                      ("rescal", np.ones((2, 3, 3)))):
        np.testing.assert_array_equal(X.exact_ranks(model, same, Rr, q, q), np.ones((3, 4)))


def test_eval_order_groups_by_relation_in_first_appearance_order():
    test = np.array([(0, 1, 2), (3, 4, 0), (5, 6, 2), (7, 8, 1), (9, 9, 0)])
    np.testing.assert_array_equal(X.eval_order(test),
                                  [(0, 1, 2), (5, 6, 2), (3, 4, 0), (9, 9, 0), (7, 8, 1)])


@pytest.mark.parametrize("model,d,scale", X.FLOAT_CASES)
def test_envelope_is_informative_on_the_float_cases(model, d, scale):
    """The GPU test asserts lo <= ranks <= hi on these cases; that only has
    teeth while the interval is a single rank almost everywhere."""
    E, R, test, known = X.make_float_case(model, d, scale, X.case_seed(model, d, scale))
    lo, hi = X.rank_envelope(model, E, R, test, known)
    width = hi - lo
    assert lo.shape == (120, 4) and (width >= 0).all() and (lo >= 1).all()
    print("%s d=%d scale=%g: %d of %d entries with hi == lo, max width %d"
          % (model, d, scale, (width == 0).sum(), width.size, width.max()))
    assert (width == 0).mean() >= 0.9
    assert width.max() <= 2
    assert (lo[:, 1] < lo[:, 0]).any() and (lo[:, 3] < lo[:, 2]).any()   # the filter bites


@pytest.mark.parametrize("model,d,N,nq", X.INT_CASES)
def test_int_cases_filter_moves_ranks(model, d, N, nq):
    """Every integer case of the GPU test has a known set dense enough that
    filtering changes a rank, unless it has too few entities for any rank to
    move (and the two large cases take a second or so on one core)."""
    E, R, test, known = X.make_int_case(model, d, N, nq, X.case_seed(model, d, N, nq))
    r = X.exact_ranks(model, E, R, test, known)
    assert (r >= 1).all() and (r <= N).all()
    assert (r[:, 1] <= r[:, 0]).all() and (r[:, 3] <= r[:, 2]).all()
    if N >= 63:
        assert (r[:, 1] < r[:, 0]).any() or (r[:, 3] < r[:, 2]).any()
    if N == 1:
        assert (r == 1).all()


# ---- the evaluator's id check (skge_amd/eval.py check_triple_ids) ----

def test_check_triple_ids_accepts_valid_and_empty():
    from skge_amd.eval import check_triple_ids
    check_triple_ids(np.array([(0, 4, 0), (4, 0, 2)], dtype=np.int32), 5, 3, "test triples")
    check_triple_ids(np.zeros((0, 3), dtype=np.int32), 5, 3, "test triples")
    check_triple_ids([], 5, 3, "known triples")


@pytest.mark.parametrize("bad,row", [((-1, 0, 0), 1), ((0, -1, 0), 1), ((0, 0, -1), 1),
                                     ((5, 0, 0), 1), ((0, 5, 0), 1), ((0, 0, 3), 1),
                                     ((7, 9, 4), 0)])
def test_check_triple_ids_names_the_first_offender(bad, row):
    from skge_amd.eval import check_triple_ids
    trip = [(1, 2, 0), (3, 4, 2), (5, 5, 5)]
    trip.insert(row, bad)
    with pytest.raises(ValueError) as e:
        check_triple_ids(np.array(trip, dtype=np.int32), 5, 3, "known triples")
    msg = str(e.value)
    assert "known triples" in msg and "triple %d " % row in msg
    assert "s=%d, o=%d, p=%d" % bad in msg


def test_ranks_checks_ids_before_touching_the_device(monkeypatch):
    """ranks() raises on an out-of-range test or known triple before it loads
    the library, allocates or launches: here no library call can succeed."""
    import skge_amd.eval as EV

    class Table(object):
        def __init__(self, rows):
            self.rows = rows

    class Model(object):
        device, d = "cpu", 4
        params = {"E": Table(5), "R": Table(3)}

    def refuse(*a, **k):
        raise AssertionError("the device path was reached")
    monkeypatch.setattr(EV, "_model_code", lambda m: (0, m.params["R"]))
    monkeypatch.setattr(EV.L, "lib", refuse)
    monkeypatch.setattr(EV.torch, "as_tensor", refuse)
    monkeypatch.setattr(EV.torch, "empty", refuse)
    ok = [(0, 1, 0), (4, 4, 2)]
    with pytest.raises(ValueError, match="test triples"):
        EV.FilteredRankingEval(ok + [(0, 5, 0)], ok).ranks(Model())
    with pytest.raises(ValueError, match="known triples"):
        EV.FilteredRankingEval(ok, ok + [(0, 0, 3)]).ranks(Model())
    with pytest.raises(ValueError, match="known triples"):
        EV.FilteredRankingEval([], [(-1, 0, 0)]).ranks(Model())
    with pytest.raises(AssertionError):   # valid ids go on to the device path
        EV.FilteredRankingEval(ok, ok).ranks(Model())
