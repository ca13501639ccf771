"""GPU tests of skge_score, skge_curve_stats and the link-prediction facade
(skge_amd/linkpred.py) against tests/linkpred_ref.py.

Mutants, each run once over this file (tools/mutants_linkpred.sh builds them
with -DSKGE_MUTANT_*; all stay inside their buffers): see DESIGN.md 3.10 for
the failure counts.
"""
import numpy as np
import pytest
import torch

import linkpred_ref as LR
from width_cases import km_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the smallest d of every row-width layout (KM = 1, 2, 3, 4, 8, 16), the
# smallest multiple of 4 of each (the 16-byte-load kernels), and d = 200
_KM = (1, 2, 3, 4, 8, 16)
D_ODD = tuple(min(d for d in range(1, 1025) if km_for(d) == km) for km in _KM)
D_QUAD = tuple(min(d for d in range(4, 1025, 4) if km_for(d) == km) for km in _KM)
assert D_ODD == (1, 65, 129, 193, 257, 513) and D_QUAD == (4, 68, 132, 196, 260, 516)
DS = tuple(sorted(set(D_ODD + D_QUAD + (200,))))
NS = (1, 63, 64, 65, 1000)


def _score(model, E, R, trip):
    """skge_score through the C ABI on fp32 copies of the tables."""
    from skge_amd import _lib as L
    lib = L.load()
    Et = torch.as_tensor(E, dtype=torch.float32, device=DEV).contiguous()
    Rt = torch.as_tensor(R, dtype=torch.float32, device=DEV).contiguous()
    t = torch.as_tensor(np.ascontiguousarray(trip, dtype=np.int32), device=DEV)
    n, d = len(trip), E.shape[1]
    code = LR.MODEL_CODE[model]
    nb = int(lib.skge_score_workspace_bytes(code, n, R.shape[0], d))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    out = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    L.check(lib.skge_score(L.stream_ptr(), code, L.ptr(Et), L.ptr(Rt), E.shape[0], R.shape[0], d,
                           L.ptr(t), n, L.ptr(ws), nb, L.ptr(out)), "score")
    return out.cpu().numpy()


def _rel_counts(n, M):
    """M = 18: relation 0 without a triple, 1 with one, 2 with 33, 3 with most."""
    if M == 1:
        return [n]
    c = [0] * M
    if n >= 1:
        c[1] = 1
    if n >= 40:
        c[2] = 33
    rest = n - sum(c)
    tail = min(rest // 8, M - 4)
    for j in range(tail):
        c[4 + j] = 1
    c[3] = n - sum(c)
    return c


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("model", LR.MODELS)
def test_scores_integer_tables_bit_equal(model, d):
    rs = np.random.RandomState(d)
    for M in ((1, 18) if model == "rescal" else (5,)):
        E, R = LR.int_tables(model, d, 40, M, 7 + d)     # once per (d, M)
        for n in NS:
            # RESCAL, M = 18: relation 0 empty, 1 with one triple, 2 with 33, 3 with most
            counts = _rel_counts(n, M) if model == "rescal" and M == 18 else None
            trip = LR.repeated_triples(rs, 40, M, n, counts)
            want = LR.scores_f64(model, E, R, trip, integer=True).astype(np.float32)
            got = _score(model, E, R, trip)
            bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
            print("%s d=%d M=%d n=%d mismatches=%d" % (model, d, M, n, bad))
            assert bad == 0, (model, d, M, n, got[:4], want[:4])


def test_rel_counts_shape():
    c = _rel_counts(1000, 18)
    assert sum(c) == 1000 and c[0] == 0 and c[1] == 1 and c[2] == 33 and c[3] > 900
    assert sum(_rel_counts(1, 18)) == 1 and sum(_rel_counts(63, 18)) == 63


@pytest.mark.parametrize("model,d", [(m, d) for m in LR.MODELS for d in (65, 200)])
def test_scores_float_tables_within_oracle_bar(model, d):
    from oracle import skge_oracle as O
    rs = np.random.RandomState(11)
    M, N, n = 18, 300, 257

    def unif(shape):
        b = np.sqrt(6.0) / np.sqrt(shape[-2] + shape[-1])
        return rs.uniform(-b, b, size=shape).astype(np.float32).astype(np.float64)
    E = unif((N, d))
    R = unif((M, d, d) if model == "rescal" else (M, d))
    trip = LR.repeated_triples(rs, N, M, n)
    if model.startswith("transe"):
        want = O.transe_scores(E, R, trip, l1=model == "transe_l1")
    else:
        want = (O.hole_scores if model == "hole" else O.rescal_scores)(E, R, trip)
    got = _score(model, E, R, trip)
    err = float(np.abs(got - want).max())
    print("%s d=%d max abs err %.3g" % (model, d, err))
    assert err < 1e-5
    again = _score(model, E, R, trip)
    assert got.tobytes() == again.tobytes()          # two runs, equal bytes


def _reltopk_all(E, R, pairs):
    """skge_reltopk (RESCAL) with k = M and no exclusions: the score of every
    relation for every (s, o) pair, [nq][M] by relation id."""
    from skge_amd import _lib as L
    lib = L.load()
    Et = torch.as_tensor(E, dtype=torch.float32, device=DEV).contiguous()
    Rt = torch.as_tensor(R, dtype=torch.float32, device=DEV).contiguous()
    q = torch.as_tensor(np.ascontiguousarray(pairs, dtype=np.int32), device=DEV)
    nq, d, M = len(pairs), E.shape[1], R.shape[0]
    code = LR.MODEL_CODE["rescal"]
    nb = int(lib.skge_reltopk_workspace_bytes(nq, d, M, M, code))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    ids = torch.full((nq, M), -7, dtype=torch.int32, device=DEV)
    val = torch.full((nq, M), float("nan"), dtype=torch.float32, device=DEV)
    L.check(lib.skge_reltopk(L.stream_ptr(), code, L.ptr(Et), L.ptr(Rt), E.shape[0], M, d, L.ptr(q),
                             nq, M, None, None, L.ptr(ws), nb, L.ptr(ids), L.ptr(val)), "reltopk")
    ids, val = ids.cpu().numpy(), val.cpu().numpy()
    assert (np.sort(ids, axis=1) == np.arange(M)).all()      # every relation once
    out = np.empty((nq, M), dtype=np.float32)
    np.put_along_axis(out, ids, val, axis=1)
    return out


# (d, M, nq): scalar-tail staging, one partial column tile, a partial last row
# block / the vector path, exactly two 32-column tiles / two 128-column passes
# with a 2-column second pass, one live row
@pytest.mark.parametrize("d,M,nq", [(33, 5, 70), (64, 3, 33), (130, 4, 1)])
def test_rescal_score_and_reltopk_share_their_bits(d, M, nq):
    """k_score_rescal and k_rel_rescal run one score tile (skge_rescal_tile.h):
    the score of (s, o, p_j) is bit-equal from skge_score and from skge_reltopk,
    whatever block width, row place and relation grouping either picks."""
    rs = np.random.RandomState(1000 * d + nq)
    N = 40
    b = np.sqrt(6.0) / np.sqrt(2 * d)
    E = rs.uniform(-b, b, size=(N, d)).astype(np.float32)
    R = rs.uniform(-b, b, size=(M, d, d)).astype(np.float32)
    pairs = rs.randint(0, N, size=(nq, 2)).astype(np.int32)
    mat = _reltopk_all(E, R, pairs)
    trip = np.concatenate([np.repeat(pairs, M, axis=0),
                           np.tile(np.arange(M, dtype=np.int32), nq)[:, None]], axis=1)
    got = _score("rescal", E, R, trip).reshape(nq, M)
    assert (got != 0).all()           # the top-k key holds -0 as +0: no score is a zero
    bad = int((got.view(np.int32) != mat.view(np.int32)).sum())
    print("d=%d M=%d nq=%d mismatches=%d of %d" % (d, M, nq, bad, nq * M))
    assert bad == 0, (got[:2], mat[:2])


def _curve(scores, labels, seg, nseg):
    """skge_curve_stats through the C ABI; (status, counts, areas, thresh)."""
    from skge_amd import _lib as L
    lib = L.load()
    n = len(scores)
    s = torch.as_tensor(np.ascontiguousarray(scores, dtype=np.float32), device=DEV)
    y = torch.as_tensor(np.ascontiguousarray(labels, dtype=np.int8), device=DEV)
    g = None if seg is None else torch.as_tensor(np.ascontiguousarray(seg, dtype=np.int32),
                                                 device=DEV)
    nb = int(lib.skge_curve_stats_workspace_bytes(n, nseg))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    counts = torch.full((nseg, 4), -7, dtype=torch.int64, device=DEV)
    areas = torch.full((nseg, 2), -7.0, dtype=torch.float64, device=DEV)
    thresh = torch.full((nseg,), -7.0, dtype=torch.float32, device=DEV)
    status = torch.full((1,), 99, dtype=torch.int32, device=DEV)
    L.check(lib.skge_curve_stats(L.stream_ptr(), L.ptr(s), L.ptr(y), L.ptr(g), n, nseg, L.ptr(ws),
                                 nb, L.ptr(counts), L.ptr(areas), L.ptr(thresh), L.ptr(status)),
            "curve_stats")
    return (int(status.item()), counts.cpu().numpy(), areas.cpu().numpy(), thresh.cpu().numpy())


def _check_curve(scores, labels, seg, nseg):
    st, counts, areas, thresh = _curve(scores, labels, seg, nseg)
    assert st == 0
    refs = LR.curve_ref_segments(scores, labels, seg, nseg)
    bound = LR.area_rel_bound(len(scores), nseg)
    worst = 0.0
    for i, r in enumerate(refs):
        got = tuple(int(x) for x in counts[i])
        assert got == (r["P"], r["Nneg"], r["twoU"], r["best_correct"]), (i, got, r)
        assert thresh[i].tobytes() == np.float32(r["thresh"]).tobytes(), (i, thresh[i], r["thresh"])
        for j, key in enumerate(("pr_auc", "average_precision")):
            if r[key] is None:
                assert np.isnan(areas[i, j]), (i, key)
            else:
                rel = abs(LR.Fraction(float(areas[i, j])) - r[key]) / r[key]
                worst = max(worst, float(rel))
                assert rel <= bound, (i, key, float(rel), bound)
    st2, c2, a2, t2 = _curve(scores, labels, seg, nseg)
    assert (c2.tobytes(), a2.tobytes(), t2.tobytes()) == (counts.tobytes(), areas.tobytes(),
                                                          thresh.tobytes())
    return worst


@pytest.mark.parametrize("kind", LR.CURVE_KINDS)
def test_curve_stats_one_segment_every_size(kind):
    for n in LR.CURVE_SIZES:
        s, y = LR.curve_case(kind, n, 17 + n)
        worst = _check_curve(s, y, None, 1)
        print("%s n=%d worst relative area error %.3g (bound %.3g)"
              % (kind, n, worst, LR.area_rel_bound(n, 1)))


@pytest.mark.parametrize("nseg", (18, 1345))
@pytest.mark.parametrize("kind", ("levels8", "informative", "zeros"))
def test_curve_stats_segments(kind, nseg):
    for n in (0, 1, 257, 4097, 70001):
        s, y = LR.curve_case(kind, n, 5 + n)
        seg = LR.segment_ids(n, nseg, 3)
        worst = _check_curve(s, y, seg, nseg)
        print("%s nseg=%d n=%d worst relative area error %.3g" % (kind, nseg, n, worst))


def test_curve_stats_nan_sets_status_and_writes_nothing():
    s, y = LR.curve_case("informative", 4097, 1)
    s[3000] = np.nan
    st, counts, areas, thresh = _curve(s, y, None, 1)
    assert st & 1
    assert (counts == -7).all() and (areas == -7.0).all() and (thresh == -7.0).all()
    from skge_amd import linkpred as LP
    with pytest.raises(ValueError, match="NaN"):
        LP.curve_stats(torch.as_tensor(s, device=DEV), y)
    with pytest.raises(ValueError, match="labels"):
        LP.curve_stats(torch.zeros(4, device=DEV), np.ones(3))


# ---- facade ----
@pytest.fixture(scope="module")
def trained():
    """A small HolE model after a few logistic epochs, and labelled sets."""
    import skge_amd as S
    np.random.seed(3)
    N, M, d = 60, 6, 32
    rs = np.random.RandomState(2)
    pos = {(int(rs.randint(N)), int(rs.randint(N)), int(rs.randint(M - 1))) for _ in range(400)}
    pos = sorted(pos)
    neg = [(int(rs.randint(N)), int(rs.randint(N)), p) for _, _, p in pos]
    xs = pos + neg
    ys = [1] * len(pos) + [-1] * len(neg)
    m = S.HolE((N, N, M), d)
    tr = S.StochasticTrainer(m, nbatches=4, max_epochs=5, learning_rate=0.1)
    tr.fit(list(xs), list(ys))
    perm = rs.permutation(len(xs))
    xs, ys = np.array(xs, dtype=np.int32)[perm], np.array(ys)[perm]
    half = len(xs) // 2
    return m, (xs[:half], ys[:half]), (xs[half:], ys[half:])


def test_link_prediction_eval_equals_sklearn_on_device_scores(trained):
    from sklearn.metrics import auc, average_precision_score, precision_recall_curve, roc_auc_score
    import skge_amd as S
    m, (xs, ys), _ = trained
    sc = m.score(xs).cpu().numpy()
    assert sc.dtype == np.float32 and np.isfinite(sc).all()
    want = LR.scores_f64("hole", np.asarray(m.params["E"], dtype=np.float64),
                         np.asarray(m.params["R"], dtype=np.float64), xs)
    assert np.abs(sc - want).max() < 1e-5
    # the tensor path (host int64, device int32) and the list path give the same bytes
    for t in (torch.as_tensor(xs.astype(np.int64)), torch.as_tensor(xs, device=DEV)):
        assert m.score(t).cpu().numpy().tobytes() == sc.tobytes()
    assert m.score([tuple(int(v) for v in r) for r in xs[:7]]).cpu().numpy().tobytes() == \
        sc[:7].tobytes()
    assert m.score(torch.zeros((0, 3), dtype=torch.int64)).shape == (0,)
    with pytest.raises(ValueError, match="out of range"):
        m.score(torch.tensor([[2 ** 32, 0, 0]], device=DEV))
    ev = S.LinkPredictionEval(xs, ys)
    pr, roc = ev.scores(m)
    p, r, _ = precision_recall_curve(ys, sc)
    bound = LR.area_rel_bound(len(xs), 1)
    assert abs(pr - auc(r, p)) <= (bound + 1e-15) * pr + 1e-15
    assert abs(roc - roc_auc_score(ys, sc)) <= 1e-15 + 4 * LR.U53
    ap = ev.average_precision(m)
    assert abs(ap - average_precision_score(ys, sc)) <= (bound + 1e-15) * ap + 1e-15
    per = ev.per_relation(m)
    refs = LR.curve_ref_segments(sc, ys, xs[:, 2], 6)
    assert per["P"].tolist() == [x["P"] for x in refs]
    assert np.isnan(per["roc_auc"][5]) and np.isnan(per["pr_auc"][5])   # relation 5 is unused
    # 0/1 labels mean the same
    assert S.LinkPredictionEval(xs, (ys > 0).astype(int)).scores(m) == (pr, roc)


def test_triple_classifier_equals_reference(trained):
    import skge_amd as S
    m, (vx, vy), (tx, ty) = trained
    keep = vx[:, 2] != 4                 # relation 4 is absent from validation
    vx, vy = vx[keep], vy[keep]
    sc_v = m.score(vx).cpu().numpy()
    sc_t = m.score(tx).cpu().numpy()
    clf = S.TripleClassifier(m).fit(vx, vy)
    g = LR.curve_ref(sc_v, vy)
    refs = LR.curve_ref_segments(sc_v, vy, vx[:, 2], 6)
    want = np.array([r["thresh"] if r["P"] + r["Nneg"] else g["thresh"] for r in refs],
                    dtype=np.float32)
    assert clf.thresh.tobytes() == want.tobytes()
    assert clf.thresh[4].tobytes() == np.float32(g["thresh"]).tobytes()   # the global fall-back
    assert (tx[:, 2] == 4).any()
    pred = clf.predict(tx)
    assert pred.dtype == torch.bool
    ref_pred = sc_t >= want[tx[:, 2]]
    assert (pred.cpu().numpy() == ref_pred).all()
    acc, per = clf.accuracy(tx, ty)
    assert acc == float((ref_pred == (ty > 0)).mean())
    # on the validation set itself the per-relation fit reaches best_correct
    _, per_v = clf.accuracy(vx, vy)
    for r in range(6):
        tot = refs[r]["P"] + refs[r]["Nneg"]
        if tot:
            assert per_v[r] == refs[r]["best_correct"] / tot
    one = S.TripleClassifier(m).fit(vx, vy, per_relation=False)
    assert (one.thresh == np.float32(g["thresh"])).all()


def test_link_prediction_callback_remembers_the_best_epoch(trained):
    import skge_amd as S
    m, (vx, vy), (tx, ty) = trained
    f = S.link_prediction_callback(S.LinkPredictionEval(vx, vy), S.LinkPredictionEval(tx, ty), 2)

    class T(object):
        model = m
        epoch = 1
    assert f(T) is True and f.best["epoch"] is None
    T.epoch = 2
    assert f(T) is True and f.best["epoch"] == 2
    assert f.best["auc pr test"] == S.LinkPredictionEval(tx, ty).scores(m)[0]
    T.epoch = 4
    f(T)
    assert f.best["epoch"] == 2          # no improvement: the record stays
