"""The top-k references of tests/topk_ref.py against brute force, the
envelope's sandwich (forced <= fp64 top-k <= allowed) and its tightness on the
float cases of tests/test_gpu_topk.py, the padding rule, skge_topk's argument
refusals and LinkPredictor's host-side checks.  No GPU."""
import ctypes

import numpy as np
import pytest

import eval_ref as X
import topk_ref as T

MODELS = ["transe", "hole", "rescal"]


def _brute(scores, k, excluded):
    """The contract, literally: sort the eligible (-score, id) pairs."""
    pairs = sorted((-int(s), j) for j, s in enumerate(scores) if j not in excluded)[:k]
    ids = [j for _, j in pairs] + [-1] * (k - len(pairs))
    sc = [float(-s) for s, _ in pairs] + [-np.inf] * (k - len(pairs))
    return ids, sc


def _int_case(model):
    E, R, test, known = X.make_int_case(model, 5, 40, 30, X.case_seed("topk-cpu", model))
    return E, R, test, known


@pytest.mark.parametrize("direction", T.DIRECTIONS)
@pytest.mark.parametrize("model,l2", [(m, False) for m in MODELS] + [("transe", True)])
def test_exact_topk_equals_brute_force(model, direction, l2):
    E, R, test, known = _int_case(model)
    q = test[:, [0, 2]] if direction == "tail" else test[:, [1, 2]]
    excl = T.known_answers(q, known, direction)
    assert any(len(e) for e in excl)
    ties = 0
    for k in (1, 7, 40, 45):
        for ex in (None, excl):
            ids, sc = T.exact_topk(model, E, R, q, direction, k, ex, l2=l2)
            assert ids.shape == sc.shape == (len(q), k) and ids.dtype == np.int64
            for i, (a, p) in enumerate(q.tolist()):
                if l2:
                    qv = E[a] + R[p] if direction == "tail" else E[a] - R[p]
                    full = -((qv - E) ** 2).sum(axis=1)
                else:
                    full = X.int_scores(model, E, R, a, a, p, direction)
                want = _brute(full, k, set() if ex is None else set(ex[i].tolist()))
                assert ids[i].tolist() == want[0] and sc[i].tolist() == want[1]
                ties += len(set(want[1])) < len(want[1])
    assert ties    # equal scores occur, so the id rule is exercised


def test_padding_rule():
    """Fewer eligible entities than k: ids -1 and scores -inf fill the row."""
    E = np.array([[0.0], [2.0], [1.0], [2.0]])
    R = np.zeros((1, 1))
    # TransE, tail of (0, ?, 0): scores 0, -2, -1, -2
    ids, sc = T.exact_topk("transe", E, R, [(0, 0)], "tail", 6, None)
    assert ids.tolist() == [[0, 2, 1, 3, -1, -1]]
    assert sc.tolist() == [[0.0, -1.0, -2.0, -2.0, -np.inf, -np.inf]]
    ids, sc = T.exact_topk("transe", E, R, [(0, 0)], "tail", 3, [[0, 1, 2]])
    assert ids.tolist() == [[3, -1, -1]] and sc.tolist() == [[-2.0, -np.inf, -np.inf]]
    ids, sc = T.exact_topk("transe", E, R, [(0, 0)], "tail", 2, [[0, 1, 2, 3]])
    assert ids.tolist() == [[-1, -1]] and np.isneginf(sc).all()
    # squared L2 reorders nothing here but squares the scores
    ids, sc = T.exact_topk("transe", E, R, [(0, 0)], "tail", 4, None, l2=True)
    assert ids.tolist() == [[0, 2, 1, 3]] and sc.tolist() == [[0.0, -1.0, -4.0, -4.0]]


def _float_queries(test, direction):
    return test[:, [0, 2]] if direction == "tail" else test[:, [1, 2]]


FLOAT_K = (1, 10, 64)


def forced_share(model, d, scale, k, l2=False):
    """Over both directions of a float case, with the known answers excluded:
    checks forced <= fp64 top-k <= allowed and returns forced / top-k slots."""
    E, R, test, known = X.make_float_case(model, d, scale, X.case_seed(model, d, scale))
    forced_n = slots = 0
    for direction in T.DIRECTIONS:
        q = _float_queries(test, direction)
        excl = T.known_answers(q, known, direction)
        sc, tau, forced, allowed = T.topk_envelope(model, E, R, q, direction, k, excl, l2=l2)
        ids, _ = T.topk_of_scores(sc, k, excl)
        top = np.zeros_like(forced)
        for i, row in enumerate(ids):
            top[i, row[row >= 0]] = True
            assert not forced[i, excl[i]].any() and not allowed[i, excl[i]].any()
        assert (tau > 0).all()
        assert not (forced & ~top).any() and not (top & ~allowed).any()
        forced_n += forced.sum()
        slots += top.sum()
    return forced_n / slots


@pytest.mark.parametrize("k", FLOAT_K)
@pytest.mark.parametrize("model,d,scale", X.FLOAT_CASES)
def test_envelope_sandwich_and_tightness(model, d, scale, k):
    share = forced_share(model, d, scale, k)
    print("%s d=%d scale=%g k=%d: forced share %.4f" % (model, d, scale, k, share))
    assert share >= 0.99


@pytest.mark.parametrize("k", FLOAT_K)
def test_envelope_squared_l2(k):
    share = forced_share("transe", 40, 1.0, k, l2=True)
    print("transe L2 d=40 k=%d: forced share %.4f" % (k, share))
    assert share >= 0.99


# ---- skge_topk's refusals (no GPU: every check precedes the first launch) ----

def _call(lib, **kw):
    n, d, k, N = 4, 8, 3, 16
    host = lambda ct, m: (ct * m)()
    a = dict(stream=None, model=0, E=host(ctypes.c_float, N * d), R=host(ctypes.c_float, 2 * d),
             N=N, d=d, queries=host(ctypes.c_int, 2 * n), nq=n, direction=0, k=k, excl_off=None,
             excl_ent=None, ws=host(ctypes.c_char, 1 << 16), ws_bytes=1 << 16,
             ent=host(ctypes.c_int, n * 130), score=host(ctypes.c_float, n * 130))
    a.update(kw)
    p = lambda x: None if x is None else ctypes.cast(x, ctypes.c_void_p)
    return lib.skge_topk(a["stream"], a["model"], p(a["E"]), p(a["R"]), a["N"], a["d"],
                         p(a["queries"]), a["nq"], a["direction"], a["k"], p(a["excl_off"]),
                         p(a["excl_ent"]), p(a["ws"]), a["ws_bytes"], p(a["ent"]), p(a["score"]))


@pytest.mark.parametrize("bad,word", [
    (dict(E=None), b"NULL"), (dict(R=None), b"NULL"), (dict(queries=None), b"NULL"),
    (dict(ent=None), b"NULL"), (dict(score=None), b"NULL"),
    (dict(excl_off=(ctypes.c_int * 5)()), b"NULL"),
    (dict(model=4), b"model"), (dict(model=-1), b"model"), (dict(direction=2), b"direction"),
    (dict(k=0), b"k = 0"), (dict(k=129), b"k = 129"), (dict(d=1025), b"1024"),
    (dict(N=0), b"sizes"), (dict(ws=None), b"workspace"), (dict(ws_bytes=64), b"workspace")])
def test_topk_refuses_bad_arguments(bad, word):
    from skge_amd import _lib as L
    lib = L.load()
    assert _call(lib, **bad) == -1
    assert word in lib.skge_last_error()


def test_topk_no_queries_is_ok_and_workspace_grows():
    from skge_amd import _lib as L
    lib = L.load()
    assert _call(lib, nq=0, ws=None, ws_bytes=0) == 0
    w = lib.skge_topk_workspace_bytes
    assert w(4, 8, 3, 16) >= 4 * 8 * 4 + 4 * 3 * 8
    assert w(5000, 200, 100, 40943) > w(5000, 200, 10, 40943) > w(50, 200, 10, 40943)
    assert w(4, 8, 128, 1) > 0      # k > N is legal


# ---- LinkPredictor's host-side checks (skge_amd/predict.py) ----

class _Table(object):
    def __init__(self, rows):
        self.rows = rows


class _Model(object):
    device, d = "cpu", 4
    params = {"E": _Table(5), "R": _Table(3)}

    def _kernel_model(self):
        return 1


@pytest.fixture
def no_device(monkeypatch):
    """Any step towards the device fails the test (as
    test_ranks_checks_ids_before_touching_the_device arranges)."""
    import skge_amd.predict as P

    def refuse(*a, **k):
        raise AssertionError("the device path was reached")
    monkeypatch.setattr(P, "_model_code", lambda m: (0, m.params["R"]))
    monkeypatch.setattr(P.L, "lib", refuse)
    monkeypatch.setattr(P.torch, "as_tensor", refuse)
    monkeypatch.setattr(P.torch, "empty", refuse)
    return P


def test_predictor_checks_before_touching_the_device(no_device):
    P = no_device
    known = [(0, 1, 0), (4, 4, 2)]
    lp = P.LinkPredictor(_Model(), known)
    with pytest.raises(ValueError, match="subject 5"):
        lp.tails([0, 5], [0, 0])
    with pytest.raises(ValueError, match="query 1 has object -1"):
        lp.heads([0, -1, 9], 0)
    with pytest.raises(ValueError, match="relation 3"):
        lp.tails(0, 3)
    with pytest.raises(ValueError, match="exclude: query 1 has entity 5"):
        lp.tails([0, 1], [0, 0], exclude=[[1], [2, 5]])
    with pytest.raises(ValueError, match="exclude"):
        lp.tails([0, 1], [0, 0], exclude=[[1]])
    for k in (0, 129, -1, 2.5, None):
        with pytest.raises(ValueError, match="k must be"):
            lp.tails(0, 0, k=k)
    with pytest.raises(ValueError, match="known_triples"):
        P.LinkPredictor(_Model()).tails(0, 0)
    with pytest.raises(ValueError, match="known triples"):
        P.LinkPredictor(_Model(), [(0, 5, 0)]).tails(0, 0)
    with pytest.raises(ValueError, match="scoring"):
        P.LinkPredictor(_Model(), known, scoring="l2")
    with pytest.raises(AssertionError):     # valid queries go on to the device path
        lp.tails(0, 0)
    with pytest.raises(AssertionError):
        P.LinkPredictor(_Model()).heads([1, 2], [0, 1], filtered=False, exclude=[[0], None])
    ents, scores = lp.tails([], [], k=3)    # no queries: nothing to launch
    assert ents.shape == scores.shape == (0, 3)


def test_predictor_merges_filter_and_exclude(no_device):
    P = no_device
    known = [(0, 3, 1), (0, 1, 1), (0, 1, 1), (2, 1, 1), (0, 4, 2)]
    lp = P.LinkPredictor(_Model(), known)
    a, r = np.array([0, 2, 0]), np.array([1, 1, 0])
    off, ent = lp._exclusions(a, r, 0, True, [[4, 1, 4], None, [2]], 5)
    assert off.tolist() == [0, 3, 4, 5] and ent.tolist() == [1, 3, 4, 1, 2]
    assert off.dtype == ent.dtype == np.int32
    off, ent = lp._exclusions(np.array([1]), np.array([1]), 1, True, None, 5)   # heads of (?, 1, 1)
    assert off.tolist() == [0, 2] and ent.tolist() == [0, 2]
    assert lp._exclusions(a, r, 0, False, None, 5) is None
    off, ent = lp._exclusions(np.array([0]), np.array([1]), 0, False, [3, 0, 3], 5)  # one query, flat
    assert off.tolist() == [0, 2] and ent.tolist() == [0, 3]
