"""CPU checks of the link-prediction references (tests/linkpred_ref.py), the
new entry points' ABI and the Python host checks (skge_amd/linkpred.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import linkpred_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["skge_score_workspace_bytes", "skge_score", "skge_curve_stats_workspace_bytes",
       "skge_curve_stats"]

# sklearn refuses +-inf scores and a single class: those cases are held to the
# Fraction reference's own definitions only
SK_CASES = [(k, n, 10 * i + j) for i, k in enumerate(("equal", "levels8", "distinct", "zeros",
                                                      "informative"))
            for j, n in enumerate((2, 255, 256, 257, 4097))]


def _two_classes(y):
    if y.sum() == 0:
        y[0] = 1
    if y.sum() == len(y):
        y[-1] = 0
    return y


@pytest.mark.parametrize("kind,n,seed", SK_CASES)
def test_reference_agrees_with_sklearn(kind, n, seed):
    from sklearn.metrics import auc, average_precision_score, precision_recall_curve, roc_auc_score
    s, y = LR.curve_case(kind, n, seed)
    y = _two_classes(y)
    r = LR.curve_ref(s, y)
    pr, rc, _ = precision_recall_curve(y, s)
    assert abs(float(r["pr_auc"]) - auc(rc, pr)) <= 1e-12
    assert abs(float(LR.roc_auc_ref(r)) - roc_auc_score(y, s)) <= 1e-12
    assert abs(float(r["average_precision"]) - average_precision_score(y, s)) <= 1e-12


def test_reference_agrees_with_the_golden_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "linkpred", "linkpred_ref.npz"))
    assert int(z["n_cases"]) >= 5
    for k in range(int(z["n_cases"])):
        r = LR.curve_ref(z["scores_%d" % k], z["ys_%d" % k])
        pr, roc = z["expect_%d" % k]
        assert abs(float(r["pr_auc"]) - pr) <= 1e-12, k
        assert abs(float(LR.roc_auc_ref(r)) - roc) <= 1e-12, k


@pytest.mark.parametrize("kind", LR.CURVE_KINDS)
@pytest.mark.parametrize("n", (0, 1, 2, 63, 257))
def test_threshold_rule_against_brute_force(kind, n):
    s, y = LR.curve_case(kind, n, 3 + n)
    r = LR.curve_ref(s, y)
    best, thr = LR.best_correct_brute(s, y)
    assert r["best_correct"] == best
    assert np.float32(r["thresh"]).tobytes() == np.float32(thr).tobytes()
    # the rule score >= thresh reaches best_correct (but +inf as "predict none"
    # cannot say so of a set that holds +inf scores)
    if n and not (np.isposinf(r["thresh"]) and np.isposinf(s).any()):
        assert int(((LR.canon(s) >= r["thresh"]) == (y > 0)).sum()) == best


def test_edge_values_of_the_reference():
    r = LR.curve_ref(np.zeros(0, np.float32), np.zeros(0, np.int8))
    assert (r["P"], r["Nneg"], r["twoU"], r["best_correct"]) == (0, 0, 0, 0)
    assert r["pr_auc"] is None and np.isposinf(r["thresh"])
    r = LR.curve_ref(np.array([0.0, -0.0], np.float32), np.array([1, 0], np.int8))
    assert r["twoU"] == 1 and LR.roc_auc_ref(r) == LR.Fraction(1, 2)   # one tie group
    segs = LR.curve_ref_segments(np.array([1, 2, 3], np.float32), np.array([1, 0, 1]),
                                 np.array([2, 0, 2]), 3)
    assert [x["P"] + x["Nneg"] for x in segs] == [1, 0, 2]
    for n in LR.CURVE_SIZES:
        for nseg in (1, 18, 1345):
            assert LR.area_rel_bound(n, nseg) < 1e-12
    assert LR.area_rel_bound(10 ** 7, 1) < 1e-12


def test_int_scores_are_exact_integers_and_fft_matches_direct():
    rs = np.random.RandomState(0)
    for model in LR.MODELS:
        for d in (1, 5, 68):
            E, R = LR.int_tables(model, d, 9, 3, 1)
            t = LR.repeated_triples(rs, 9, 3, 17)
            sc = LR.scores_f64(model, E, R, t, integer=True)
            assert (sc == np.rint(sc)).all() and np.abs(sc).max() < 2 ** 24
            if model == "hole":
                ref = [R[p] @ LR.ccorr_direct(E[s], E[o]) for s, o, p in t]
                assert (sc == np.array(ref)).all()
    E, R = LR.int_tables("hole", 1024, 4, 2, 1)
    assert np.abs(E).max() == 2


def test_segment_ids_have_the_promised_shapes():
    for nseg in (18, 1345):
        seg = LR.segment_ids(70001, nseg, 1)
        cnt = np.bincount(seg, minlength=nseg)
        assert (cnt == 0).any() and (cnt == 1).any() and cnt.max() > 2048
        assert seg.min() >= 0 and seg.max() < nseg


# ---- ABI: these fail without the feature ----
def test_new_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "skge_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(skge_[a-z0-9_]+)\s*\(", body))
    from skge_amd import _lib as L
    lib = L.load()
    for f in NEW:
        assert f in declared and f in L.SIGNATURES and hasattr(lib, f), f
    assert len(L.SIGNATURES["skge_score"][1]) == 12
    assert len(L.SIGNATURES["skge_curve_stats"][1]) == 12
    assert lib.skge_abi_version() == 2


def test_bad_arguments_are_refused_without_a_gpu():
    from skge_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 24

    def score(model=0, E=p, R=p, N=5, M=2, d=8, trip=p, n=1, ws=p, nb=big, out=p):
        return lib.skge_score(None, model, E, R, N, M, d, trip, n, ws, nb, out)
    for kw in ({"model": 4}, {"n": -1}, {"d": 0}, {"d": 1025}, {"E": None}, {"R": None},
               {"trip": None}, {"out": None}, {"ws": None}, {"nb": 8}, {"M": 0}, {"N": 0},
               {"model": 3, "nb": 300}):
        assert score(**kw) == -1, kw
        assert lib.skge_last_error()
    assert lib.skge_score_workspace_bytes(0, -1, 2, 8) == 0
    assert lib.skge_score_workspace_bytes(3, 10, 2, 1025) == 0
    assert lib.skge_score_workspace_bytes(3, 1000, 18, 200) > 1000 * 8
    assert score(n=0) == 0                      # nothing to launch

    def curve(score_=p, lab=p, seg=None, n=4, nseg=1, ws=p, nb=64, cnt=p, ar=p, th=p, st=p):
        return lib.skge_curve_stats(None, score_, lab, seg, n, nseg, ws, nb, cnt, ar, th, st)
    for kw in ({"n": -1}, {"nseg": 0}, {"score_": None}, {"lab": None}, {"ws": None},
               {"cnt": None}, {"ar": None}, {"th": None}, {"st": None}, {"nb": 64}):
        assert curve(**kw) == -1, kw
    assert lib.skge_curve_stats_workspace_bytes(-1, 1) == 0
    assert lib.skge_curve_stats_workspace_bytes(10, 0) == 0


# ---- Python host checks ----
class _P(object):
    def __init__(self, rows):
        self.rows = rows


def test_python_host_checks(monkeypatch):
    import skge_amd as S
    from skge_amd import linkpred as LP
    with pytest.raises(ValueError, match="NaN"):
        LP.check_curve_status(1)
    with pytest.raises(ValueError, match="segment"):
        LP.check_curve_status(2)
    LP.check_curve_status(0)
    with pytest.raises(ValueError, match="undefined"):
        LP.require_both_classes(5, 0, "AUC")
    with pytest.raises(ValueError, match="undefined"):
        LP.require_both_classes(0, 5, "AUC")
    with pytest.raises(ValueError, match="3 triples but 2 labels"):
        S.LinkPredictionEval([(0, 1, 0), (1, 2, 0), (2, 0, 1)], [1, -1])
    ev = S.LinkPredictionEval([((0, 1, 0), 1), ((1, 2, 0), -1)], [1, 0])
    assert ev.xs.shape == (2, 3) and ev.ys.tolist() == [1, 0]
    assert LP.labels_array([1, -1, 0, 1]).tolist() == [1, 0, 0, 1]
    # ids are range-checked before anything touches the device
    monkeypatch.setattr(LP.L, "require_gpu", lambda: None)

    class M(object):
        rel_id = "R"
        params = {"E": _P(5), "R": _P(2)}
        device = "cpu"
        d = 8

        def _kernel_model(self):
            return 0
    for bad in ([(5, 0, 0)], [(0, -1, 0)], [(0, 1, 2)]):
        with pytest.raises(ValueError, match="out of range"):
            LP.score_triples(M(), bad)
    # a tensor is checked before it is narrowed to int32: 2^32 must not wrap to 0
    import torch
    for bad in (torch.tensor([[2 ** 32, 0, 0]]), torch.tensor([[0, 1, 2 ** 32 + 1]]),
                torch.tensor([[0, 5, 0]], dtype=torch.int32)):
        with pytest.raises(ValueError, match="out of range"):
            LP.score_triples(M(), bad)
    for bad in (np.array([[2 ** 32, 0, 0]]), [(0, 2 ** 32 + 1, 0)], [((0, 1, 2 ** 32), 1)]):
        with pytest.raises(ValueError, match="out of range"):
            LP.score_triples(M(), bad)
    assert S.LinkPredictionEval(np.array([[2 ** 32, 0, 0]]), [1]).xs[0, 0] == 2 ** 32   # kept wide
    assert hasattr(S.Model, "score")
    f = S.link_prediction_callback(None, None, every=2)
    assert f.best["epoch"] is None
