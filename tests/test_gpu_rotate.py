"""RotatE on the device against tests/rotate_ref.py (fp64).

Explicit-pair step and Model.score at d in {2, 8, 50, 66, 130, 200, 258, 514}
(KM 1 to 16, rows ending one complex component into a register), N = 64,
M = 4, P = 64.  Scale, margin and seed of every width are chosen on the CPU
(rotate_ref.case, judged by tests/test_rotate_ref.py): the worst fp32 score
error bound stays under 5e-6 and no margin decision is within 1e-5, so
violation counts are compared exactly; scores and tables at the project's
1e-5 + 1e-5 |x|.

Pair-loop epochs (3 batches) run in child processes (tests/rotate_child.py),
k_rot_pos and the explicit pairs (SKGE_ROT_PAIRS=1) each in its own, and are
replayed from the device's own records."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import rotate_ref as RR

pytestmark = pytest.mark.gpu

LR = 0.1
ATOL = RTOL = 1e-5
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rotate_child.py")


def _close(got, want, what):
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
    err = np.abs(got - want)
    tol = ATOL + RTOL * np.abs(want)
    print("%s: max err %.3g, headroom %.3g" % (what, err.max(), (tol / np.maximum(err, 1e-300)).min()))
    assert np.all(err <= tol), "%s: max err %.3g" % (what, err.max())


def _model(d, E=None, R=None, margin=None, N=RR.N, M=RR.M):
    import skge_amd as S
    np.random.seed(42)
    m = S.RotatE((N, N, M), d)
    if E is not None:
        m.E.data.copy_(torch.tensor(E, dtype=torch.float32))
        m.R.data.copy_(torch.tensor(R, dtype=torch.float32))
    if margin is not None:
        m.add_hyperparam("margin", margin)
    return m


def _updaters(m, opt):
    import skge_amd as S
    U = S.AdaGrad if opt == "adagrad" else S.SGD
    return {pid: U(p, LR) for pid, p in m.params.items()}


def _check_projections(m, ids_e, ids_r):
    R = m.R.data.cpu().numpy().astype(np.float64)[ids_r]
    mod = np.sqrt(R[:, 0::2] ** 2 + R[:, 1::2] ** 2)
    assert np.abs(mod - 1.0).max() <= 4 * 2.0 ** -24
    # E: the squared norm is a fp32 sum of KM terms per lane and the wave tree's
    # 8 levels, each term one rounding more: (KM + 9) u on it, half of that on
    # its root, then the root's and the division's rounding
    E = m.E.data.cpu().numpy().astype(np.float64)[ids_e]
    bound = ((RR.km_for(E.shape[1]) + 9) / 2 + 2) * 2.0 ** -24
    assert np.abs(np.sqrt((E ** 2).sum(axis=1)) - 1.0).max() <= bound


def test_init_matches_the_restatement():
    m = _model(10)
    E, R = RR.init(RR.N, RR.M, 10, 42)
    np.testing.assert_array_equal(m.E.data.cpu().numpy(), E.astype(np.float32))
    np.testing.assert_array_equal(m.R.data.cpu().numpy(), R.astype(np.float32))
    import skge_amd as S
    with pytest.raises(ValueError):
        S.RotatE((4, 4, 2), 7)


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("d", RR.WIDTHS)
def test_explicit_pair_step_and_score(d, opt):
    E, R, pos, neg, scale, margin, seed = RR.case(d)
    m = _model(d, E, R, margin)
    what = "rotate d%d %s" % (d, opt)
    # Model.score (k_score_rot) and the pair kernel's scores
    trip = np.concatenate([pos, neg]).astype(np.int32)
    want = RR.scores(E, R, trip)
    _close(m.score(trip), want, what + " score")
    g = m._pairwise_gradients([(tuple(x), 1.0) for x in pos.tolist()],
                              [(tuple(x), -1.0) for x in neg.tolist()])
    ps, ns, nv, grads = RR.pairwise_gradients(E, R, pos, neg, margin)
    _close(m._pscore, ps, what + " pscore")
    _close(m._nscore, ns, what + " nscore")
    assert m.nviolations == nv
    for pid in ("E", "R"):
        np.testing.assert_array_equal(g[pid][1].cpu().numpy(), grads[pid][1])
        _close(g[pid][0], grads[pid][0], what + " grad " + pid)
    # the fused step from the same state
    upd = _updaters(m, opt)
    params = {"E": E.copy(), "R": R.copy()}
    state = {k: np.zeros_like(v) for k, v in params.items()}
    nviol = torch.zeros(1, dtype=torch.int32, device=m.device)
    m._pairwise_step(torch.as_tensor(pos.astype(np.int32), device=m.device),
                     torch.as_tensor(neg.astype(np.int32), device=m.device), upd, nviol)
    _, _, nv2, grads = RR.pairwise_step(params, state, pos, neg, LR, margin, opt)
    assert int(nviol.item()) == nv2 == nv
    for pid in ("E", "R"):
        _close(m.params[pid].data, params[pid], what + " step " + pid)
        if opt == "adagrad":
            _close(upd[pid].p2, state[pid], what + " p2 " + pid)
    _check_projections(m, grads["E"][1], grads["R"][1])
    for acc in m._acc.values():
        assert int(acc.cnt.abs().sum().item()) == 0


def test_zero_component_projects_to_one():
    """unitmod on the device: a zero component becomes (1, 0), the others are
    divided by their modulus (skge_update_rows with a zero gradient)."""
    from skge_amd.param import unitmod
    m = _model(130)
    X = np.random.RandomState(3).uniform(-2, 2, (RR.M, 130)).astype(np.float32)
    X[1, 64:66] = 0.0      # the component in the second register's first lanes
    X[2, 128:130] = 0.0    # the row's last component
    m.R.data.copy_(torch.tensor(X))
    unitmod(m.R, [1, 2])
    got = m.R.data.cpu().numpy()
    want = RR.unitmod_rows(X.astype(np.float64))
    np.testing.assert_array_equal(got[[0, 3]], X[[0, 3]])
    _close(got[[1, 2]], want[[1, 2]], "unitmod rows")
    assert tuple(got[1, 64:66]) == (1.0, 0.0) and tuple(got[2, 128:130]) == (1.0, 0.0)


# ---------------------------------------------------------------------------
# the device pair loop
# ---------------------------------------------------------------------------

def _pairs_of(rec, n1, start, count):
    pos, neg = [], []
    for j in range(start, start + count):
        s, o, p, a = (int(x) for x in rec[j])
        b = int(n1[j])
        if a >= 0:
            pos.append((s, o, p))
            neg.append((a, o, p))
        if b >= 0:
            pos.append((s, o, p))
            neg.append((s, b, p))
    return np.array(pos, dtype=np.int64).reshape(-1, 3), np.array(neg, dtype=np.int64).reshape(-1, 3)


def _run_children(tmp_path, d, opt, det, kg):
    out, procs = {}, {}
    for form in ("0", "1"):   # side by side: most of a child's time is its start-up
        path = str(tmp_path / ("form%s.npz" % form))
        env = dict(os.environ, SKGE_ROT_PAIRS=form)
        procs[form] = (subprocess.Popen([sys.executable, CHILD, str(d), opt, str(det), kg, path],
                                        env=env), path)
    for form, (proc, path) in procs.items():
        assert proc.wait(timeout=300) == 0, form
        out[form] = np.load(path)
    return out


def _replay(z, opt, what):
    from skge_amd.device import batch_sizes
    params = {"E": z["E0"].astype(np.float64), "R": z["R0"].astype(np.float64)}
    state = {k: np.zeros_like(v) for k, v in params.items()}
    rec, n1 = z["rec"], z["n1"]
    want_v, start = 0, 0
    for c in batch_sizes(int(z["T"]), 3):
        pos, neg = _pairs_of(rec, n1, start, c)
        start += c
        if len(pos):
            want_v += RR.pairwise_step(params, state, pos, neg, LR, 0.5, opt)[2]
    assert int(z["nviol"]) == want_v > 0, what
    assert int(z["cnt"]) == 0
    for pid in ("E", "R"):
        _close(z[pid], params[pid], "%s %s" % (what, pid))
        if opt == "adagrad":
            _close(z["p2" + pid], state[pid], "%s p2 %s" % (what, pid))
    mod = np.sqrt(z["R"].astype(np.float64)[:, 0::2] ** 2 + z["R"].astype(np.float64)[:, 1::2] ** 2)
    assert np.abs(mod - 1.0).max() <= 4 * 2.0 ** -24
    return rec, n1


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("d", [8, 130, 200])
def test_pair_loop_epoch_both_forms_vs_reference(d, opt, tmp_path):
    out = _run_children(tmp_path, d, opt, 0, "loop")
    for form, name in (("0", "k_rot_pos"), ("1", "pairs")):
        _replay(out[form], opt, "rotate d%d loop %s %s" % (d, name, opt))
    np.testing.assert_array_equal(out["0"]["rec"], out["1"]["rec"])


@pytest.mark.parametrize("d", [256, 260])
def test_deterministic_forms_leave_identical_tables(d, tmp_path):
    """Under set_deterministic(True) the sums are exact, so k_rot_pos (d = 256:
    its last width; d = 260 runs the explicit pairs either way) and
    SKGE_ROT_PAIRS=1 must leave the same bits."""
    out = _run_children(tmp_path, d, "adagrad", 1, "loop")
    assert int(out["0"]["nviol"]) == int(out["1"]["nviol"]) > 0
    for k in ("E", "R", "p2E", "p2R"):
        assert np.array_equal(out["0"][k], out["1"][k]), k
    assert not np.array_equal(out["0"]["E"], out["0"]["E0"])


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
def test_dense_kg_records_without_a_negative(opt, tmp_path):
    out = _run_children(tmp_path, 8, opt, 0, "dense")
    for form, name in (("0", "k_rot_pos"), ("1", "pairs")):
        rec, n1 = _replay(out[form], opt, "rotate dense %s %s" % (name, opt))
        assert (rec[:, 3] < 0).any() and (n1 < 0).any()
        assert (rec[:, 3] >= 0).any() or (n1 >= 0).any()


import multineg_ref as MR
import sampler_ref as SR

SAMPLERS = [("typed", SR.TYPED, 1, [0, 1]), ("lcwa", SR.LCWA, 1, [0, 1]),
            ("random_2x012", SR.RANDOM, 2, [0, 1, 2])]


@pytest.mark.parametrize("name,sampler,n,modes", SAMPLERS, ids=[x[0] for x in SAMPLERS])
def test_sampler_epochs_vs_reference(name, sampler, n, modes):
    """Typed, LCWA and RandomModeSampler(2, [0, 1, 2]) draws on the device (the
    trainer's device_negatives=True route; K > 2 runs the explicit pairs), one
    epoch of 3 batches (SGD) replayed from the device's own draws."""
    from skge_amd.device import DeviceKG, PairLoopRunner, batch_sizes, epoch_records_multi
    d = 50
    m = _model(d, margin=0.5, N=MR.N, M=MR.M)
    upd = _updaters(m, "sgd")
    kg = DeviceKG(MR.XS, m.device)
    rr = MR.REL_RANGE if sampler == SR.TYPED else None
    params = {pid: p.data.cpu().numpy().astype(np.float64) for pid, p in m.params.items()}
    state = {k: np.zeros_like(v) for k, v in params.items()}
    r = PairLoopRunner(m, upd, kg, 3, seed=MR.SEED, sampler=sampler, negatives=(n, modes, rr))
    pos, neg = epoch_records_multi(kg, MR.N, MR.M, MR.SEED, 0, n, modes, sampler=sampler,
                                   rel_range=rr)
    pos, neg = pos.cpu().numpy().astype(np.int64), neg.cpu().numpy().astype(np.int64)
    r.run(1)
    r.synchronize()
    total, start = 0, 0
    for c in batch_sizes(MR.T, 3):
        pp, nn = MR.batch_pairs(pos, neg, modes, start, c)
        total += RR.pairwise_step(params, state, np.array(pp), np.array(nn), LR, 0.5, "sgd")[2]
        start += c
    assert int(r.nviol_total.item()) == total > 0
    for pid in ("E", "R"):
        _close(m.params[pid].data, params[pid], "rotate loop %s %s" % (name, pid))


def test_evaluation_entry_points_accept_rotate():
    import skge_amd as S
    d = 50
    E, R = RR.tables(RR.N, RR.M, d, 77, 0.5)
    m = _model(d, E, R)
    xs = _kg()
    test = xs[:10]
    ev = S.FilteredRankingEval(test, xs)
    got = ev.ranks(m)
    assert got.shape == (10, 4) and (got >= 1).all() and (got[:, 1] <= got[:, 0]).all()
    none = -np.ones(10, dtype=np.int64)
    np.testing.assert_array_equal(ev.candidate_ranks(m, [[0]], none, none), got)
    typed = ev.typed_ranks(m)
    assert (typed >= 1).all() and (typed <= got).all()
    assert len(ev.positions(m)) > 0
    lp = S.LinkPredictor(m, xs)
    ids, sc = lp.tails(test[:, 0], test[:, 2], k=3, filtered=False)
    want = np.stack([RR.scores(E, R, np.stack([np.full(RR.N, s), np.arange(RR.N), np.full(RR.N, p)], 1))
                     for s, _, p in test.tolist()])
    _close(sc, -np.sort(-want, axis=1)[:, :3], "top-k tail scores")
    pool = np.arange(0, RR.N, 2)
    ct, _ = lp.heads(test[:4, 1], test[:4, 2], k=3, filtered=False, candidates=pool)
    assert set(ct.reshape(-1).tolist()) <= set(pool.tolist())
    rs = np.random.RandomState(1)
    trip = np.stack([rs.randint(RR.N, size=200), rs.randint(RR.N, size=200),
                     rs.randint(RR.M, size=200)], axis=1).astype(np.int32)
    ys = np.where(rs.rand(200) < 0.5, 1.0, -1.0)
    areas = S.LinkPredictionEval(trip, ys).scores(m)
    assert all(np.isfinite(float(a)) for a in np.ravel(np.asarray(areas, dtype=np.float64)))
    tc = S.TripleClassifier(m)
    tc.fit(trip, ys)
    assert 0.0 <= float(tc.accuracy(trip, ys)[0]) <= 1.0
    ids = S.Neighbours(m).topk(k=3, rows=np.arange(4))[0]
    assert tuple(np.asarray(ids.cpu() if torch.is_tensor(ids) else ids).shape) == (4, 3)


# ---------------------------------------------------------------------------
# trainer, refusals, checkpoints
# ---------------------------------------------------------------------------

def _kg(T=96):
    import rotate_child as RC
    return RC.loop_kg(RR.N, RR.M, T)


def _trainer(m, **kw):
    import skge_amd as S
    xs = [tuple(int(v) for v in x) for x in _kg().tolist()]
    return S.PairwiseStochasticTrainer(
        m, nbatches=3, max_epochs=2, learning_rate=LR, margin=0.5,
        samplef=S.RandomModeSampler(1, [0, 1], xs, (RR.N, RR.N, RR.M)).sample,
        file_grad=None, file_embed=None, **kw)


def _fit(tr):
    xs = [tuple(int(v) for v in x) for x in _kg().tolist()]
    tr.fit(xs, [1.0] * len(xs))


def test_trainer_auto_runs_the_pair_loop():
    from skge_amd.device import PairLoopRunner
    m = _model(50)
    before = m.R.data.clone()
    tr = _trainer(m, device_loop=True)
    _fit(tr)
    assert isinstance(tr._runner, PairLoopRunner)
    assert tr.nviolations > 0
    assert not torch.equal(before, m.R.data)
    mod = (m.R.data[:, 0::2].double() ** 2 + m.R.data[:, 1::2].double() ** 2).sqrt()
    assert float((mod - 1).abs().max()) <= 4 * 2.0 ** -24


def test_trainer_per_batch_path():
    m = _model(50)
    tr = _trainer(m)
    _fit(tr)
    assert tr.nviolations > 0


@pytest.mark.parametrize("runner", ["pipe", "epoch", "hole_pipe"])
def test_other_runners_refuse_rotate(runner):
    m = _model(8)
    tr = _trainer(m, device_loop=True, device_runner=runner)
    with pytest.raises(ValueError, match="pairs"):
        _fit(tr)


def test_logistic_trainer_and_relation_prediction_refuse_rotate():
    import skge_amd as S
    m = _model(8)
    xs = [tuple(int(v) for v in x) for x in _kg().tolist()]
    tr = S.StochasticTrainer(m, nbatches=3, max_epochs=1, learning_rate=LR,
                             samplef=S.RandomModeSampler(1, [0, 1], xs, (RR.N, RR.N, RR.M)).sample)
    with pytest.raises(ValueError, match="RotatE"):
        tr.fit(xs, [1.0] * len(xs))
    ev = S.FilteredRankingEval(np.array(xs[:5]), np.array(xs))
    with pytest.raises(ValueError, match="RotatE"):
        ev.relation_ranks(m)
    with pytest.raises(ValueError, match="RotatE"):
        S.LinkPredictor(m, np.array(xs)).relations([0], [1], k=2)
    assert ev.ranks(m).shape == (5, 4)


def test_checkpoint_round_trip(tmp_path):
    import skge_amd as S
    from skge_amd.param import normalize, unitmod
    m = _model(10)
    f = str(tmp_path / "m.pkl")
    m.save(f)
    m2 = S.Model.load(f)
    assert isinstance(m2, S.RotatE) and m2.model_code == 7
    assert m2.params["R"].post is unitmod and m2.params["E"].post is normalize
    for pid in ("E", "R"):
        assert torch.equal(m.params[pid].data, m2.params[pid].data)
    f2 = str(tmp_path / "ref.pkl")
    m.save_reference(f2)
    m3 = S.load_reference(f2)
    assert isinstance(m3, S.RotatE) and m3.params["R"].post is unitmod
    assert torch.equal(m.params["R"].data, m3.params["R"].data)
    assert pickle.loads(pickle.dumps(m)).params["R"].post is unitmod
