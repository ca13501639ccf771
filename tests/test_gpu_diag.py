"""DistMult and ComplEx on the device against tests/diag_ref.py (fp64).

Shapes: the project's golden grid, N = 512, M = 18, P <= 256, d in {8, 50,
130, 200} (KM = 1 partly filled, KM = 1 not a multiple of 4, KM = 3 with a
partly filled last register, KM = 4); ComplEx at the same four, all even.
Tolerances are parity_util's, as applied to the HolE golden cases."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import diag_ref as DR
import multineg_ref as MR
import parity_util
import sampler_ref as R
from oracle import skge_oracle as O

pytestmark = pytest.mark.gpu

N, M, P = 512, 18, 256
DS = [8, 50, 130, 200]
MARGIN = 0.2
LR = 0.1
KINDS = [("distmult", "DistMult"), ("complex", "ComplEx")]
KIND_IDS = ["distmult", "complex"]


def _model(cls, sz, d, E=None, Rt=None, **kw):
    import skge_amd as S
    np.random.seed(42)
    m = getattr(S, cls)(sz, d, **kw)
    if E is not None:
        m.E.data.copy_(torch.tensor(E, dtype=torch.float32))
        m.R.data.copy_(torch.tensor(Rt, dtype=torch.float32))
    m.add_hyperparam("margin", MARGIN)
    return m


def _updaters(m, opt):
    import skge_amd as S
    U = S.AdaGrad if opt == "adagrad" else S.SGD
    return {pid: U(p, LR) for pid, p in m.params.items()}


def _snapshot(m, upd):
    params = {pid: p.data.detach().cpu().numpy().astype(np.float64) for pid, p in m.params.items()}
    state = {pid: (upd[pid].p2.detach().cpu().numpy().astype(np.float64)
                   if getattr(upd[pid], "p2", None) is not None else np.zeros_like(params[pid]))
             for pid in m.params}
    return params, state


def _check_grads(g, want, what):
    for pid in ("E", "R"):
        gv, gi = g[pid]
        np.testing.assert_array_equal(gi.cpu().numpy(), want[pid][1], err_msg=what + pid)
        parity_util.check(gv, want[pid][0], "%s grad %s" % (what, pid))


def _check_params(m, upd, params, state, before, grads, opt, what):
    for pid in m.params:
        parity_util.check_step(m.params[pid].data, params[pid], before[pid],
                               grads[pid] if grads else None, state[pid], LR,
                               "%s %s" % (what, pid), post=parity_util.POSTS["hole"].get(pid),
                               opt=opt)
        if opt == "adagrad":
            parity_util.check(upd[pid].p2, state[pid], "%s p2 %s" % (what, pid))


# ---------------------------------------------------------------------------
# 1. the per-batch step kernels
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("rparam", [0.0, 0.01])
@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("kind,cls", KINDS, ids=KIND_IDS)
def test_pairwise_gradients_and_step(kind, cls, d, opt, rparam):
    E, Rt = DR.tables(kind, N, M, d, 7 + d, scale=0.5)
    pos, neg = DR.forced_pairs(N, M, P, 3 + d)
    m = _model(cls, (N, N, M), d, E, Rt, rparam=rparam)
    upd = _updaters(m, opt)
    what = "%s d%d %s rparam %g pairwise" % (kind, d, opt, rparam)
    g = m._pairwise_gradients([(tuple(x), 1.0) for x in pos.tolist()],
                              [(tuple(x), -1.0) for x in neg.tolist()])
    ps, ns, nv, want = DR.pairwise_gradients(kind, E, Rt, pos, neg, MARGIN, rparam=rparam)
    parity_util.check(m._pscore, ps, what + " pscore")
    parity_util.check(m._nscore, ns, what + " nscore")
    assert m.nviolations == nv > 0
    _check_grads(g, want, what)
    # the fused step from the same state
    params, state = _snapshot(m, upd)
    before = {k: v.copy() for k, v in params.items()}
    nviol = torch.zeros(1, dtype=torch.int32, device=m.device)
    m._pairwise_step(torch.as_tensor(pos.astype(np.int32), device=m.device),
                     torch.as_tensor(neg.astype(np.int32), device=m.device), upd, nviol)
    _, _, nv2, grads = DR.pairwise_step(kind, params, state, pos, neg, LR, MARGIN, opt,
                                        rparam=rparam)
    assert int(nviol.item()) == nv2
    _check_params(m, upd, params, state, before, grads, opt, what + " step")
    for acc in m._acc.values():
        assert int(acc.cnt.abs().sum().item()) == 0


def _labelled(pos, neg):
    trip = np.concatenate([pos, neg])
    ys = np.concatenate([np.ones(len(pos)), -np.ones(len(neg))])
    return trip, ys


@pytest.mark.parametrize("rparam", [0.0, 0.01])
@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("kind,cls", KINDS, ids=KIND_IDS)
def test_logistic_gradients_and_step(kind, cls, d, opt, rparam):
    E, Rt = DR.tables(kind, N, M, d, 9 + d, scale=0.5)
    pos, neg = DR.forced_pairs(N, M, P // 2, 5 + d)
    trip, ys = _labelled(pos, neg)
    m = _model(cls, (N, N, M), d, E, Rt, rparam=rparam)
    upd = _updaters(m, opt)
    what = "%s d%d %s rparam %g logistic" % (kind, d, opt, rparam)
    g = m._gradients([(tuple(t), float(y)) for t, y in zip(trip.tolist(), ys.tolist())])
    sc, loss, want = DR.gradients(kind, E, Rt, trip, ys, rparam=rparam)
    parity_util.check(m._score, sc, what + " score")
    np.testing.assert_allclose(m.loss, loss, rtol=1e-5)
    _check_grads(g, want, what)
    params, state = _snapshot(m, upd)
    before = {k: v.copy() for k, v in params.items()}
    dl = torch.zeros(1, dtype=torch.float32, device=m.device)
    m._logistic_step(torch.as_tensor(trip.astype(np.int32), device=m.device),
                     torch.as_tensor(ys.astype(np.float32), device=m.device), upd, dl)
    _, loss2, grads = DR.logistic_step(kind, params, state, trip, ys, LR, opt, rparam=rparam)
    np.testing.assert_allclose(float(dl.item()), loss2, rtol=1e-5)
    _check_params(m, upd, params, state, before, grads, opt, what + " step")


@pytest.mark.parametrize("d", [50, 200])
@pytest.mark.parametrize("kind,cls", KINDS, ids=KIND_IDS)
def test_four_batch_trajectory_through_batch_step(kind, cls, d):
    """_pairwise_gradients -> updater(g, idx), four batches; the last batch has
    one relation on every pair.  Each batch is replayed from the device state
    before it (as test_gpu_runner_oracle does for AdaGrad)."""
    import skge_amd as S
    E, Rt = DR.tables(kind, N, M, d, 21 + d, scale=0.5)
    m = _model(cls, (N, N, M), d, E, Rt, rparam=0.01)
    upd = _updaters(m, "adagrad")
    tr = S.PairwiseStochasticTrainer(m, nbatches=1, max_epochs=1, learning_rate=LR,
                                     margin=MARGIN, fused=False, file_grad=None, file_embed=None)
    tr._updaters = upd
    for b in range(4):
        pos, neg = DR.forced_pairs(N, M, P, 100 + b)
        if b == 3:
            pos[:, 2] = neg[:, 2] = 2
        params, state = _snapshot(m, upd)
        before = {k: v.copy() for k, v in params.items()}
        g = m._pairwise_gradients([(tuple(x), 1.0) for x in pos.tolist()],
                                  [(tuple(x), -1.0) for x in neg.tolist()])
        _, _, nv, grads = DR.pairwise_step(kind, params, state, pos, neg, LR, MARGIN, "adagrad",
                                           rparam=0.01)
        assert m.nviolations == nv > 0
        tr._batch_step(g)
        _check_params(m, upd, params, state, before, grads, "adagrad",
                      "%s d%d trajectory b%d" % (kind, d, b))


# ---------------------------------------------------------------------------
# 2. the device epochs
# ---------------------------------------------------------------------------

def loop_kg(T=3 * 96):
    """T distinct triples over the grid with forced duplicates: a hub subject,
    some s == o, one relation on a third of them."""
    rs = np.random.RandomState(17)
    seen, out = set(), []
    while len(out) < T:
        s, o, p = int(rs.randint(N)), int(rs.randint(N)), int(rs.randint(M))
        k = len(out)
        if k % 7 == 0:
            s = 3
        elif k % 11 == 0:   # (never both: s, o and p all forced would repeat a triple)
            o = s
        if k % 3 == 0:
            p = 1
        if (s, o, p) not in seen:
            seen.add((s, o, p))
            out.append((s, o, p))
    return np.array(out, dtype=np.int32)


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
    return np.array(pos, dtype=np.int64), np.array(neg, dtype=np.int64)


# The epochs are replayed the way test_gpu_runner_oracle.py replays them:
#   "sgd"      one epoch of 3 batches chained through the reference, SGD, at the
#              plain bar 1e-5 + 1e-5 |x|: the chain stays linear in the
#              gradient's rounding;
#   "adagrad"  one batch from the device state before it, at check_step's
#              step-aware bar.  AdaGrad divides by max(sqrt(p2), 1e-7): where
#              the first gradient of an element is ~0, an fp32 rounding e of it
#              becomes up to 1e6 lr e of parameter, which a chain of batches
#              would then carry through p2 -- a property of the updater, not
#              of the kernels (parity_util.check_step, test_gpu_runner_oracle).
LOOP_OPTS = [("sgd", 3), ("adagrad", 1)]


def _check_epoch(m, upd, params, state, before, grads, opt, nb, what):
    if nb == 1:
        _check_params(m, upd, params, state, before, grads, opt, what)
    else:
        assert opt == "sgd"
        for pid in m.params:
            parity_util.check(m.params[pid].data, params[pid], "%s %s" % (what, pid))
    for acc in m._acc.values():
        assert int(acc.cnt.abs().sum().item()) == 0


@pytest.mark.parametrize("opt,nb", LOOP_OPTS)
@pytest.mark.parametrize("form", ["pos", "pairs"])
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("kind,cls", KINDS, ids=KIND_IDS)
def test_pair_loop_epoch_vs_reference(kind, cls, d, form, opt, nb, monkeypatch):
    """One epoch (3 batches, or one: LOOP_OPTS), replayed by diag_ref from the
    device's own draws; both forms of the batch (k_diag_pos, the explicit
    pairs)."""
    from skge_amd.device import DeviceKG, PairLoopRunner, batch_sizes, epoch_records
    monkeypatch.setenv("SKGE_DIAG_PAIRS", "1" if form == "pairs" else "0")
    m = _model(cls, (N, N, M), d, rparam=0.01)
    upd = _updaters(m, opt)
    kg = DeviceKG(loop_kg(96 * nb), m.device)
    params, state = _snapshot(m, upd)
    r = PairLoopRunner(m, upd, kg, nb, seed=5)
    rec, n1 = epoch_records(kg, N, 5, 0)
    rec, n1 = rec.cpu().numpy(), n1.cpu().numpy()
    with torch.cuda.stream(r.stream):
        r.run(1)
    r.synchronize()
    want_v, start = 0, 0
    for c in batch_sizes(kg.T, nb):
        pos, neg = _pairs_of(rec, n1, start, c)
        start += c
        before = {k: v.copy() for k, v in params.items()}
        _, _, nv, grads = DR.pairwise_step(kind, params, state, pos, neg, LR, MARGIN, opt,
                                           rparam=0.01)
        want_v += nv
    assert int(r.nviol_total.item()) == want_v > 0
    _check_epoch(m, upd, params, state, before, grads, opt, nb,
                 "%s d%d pair loop (%s, %s)" % (kind, d, form, opt))


@pytest.mark.parametrize("opt,nb", LOOP_OPTS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("kind,cls", KINDS, ids=KIND_IDS)
def test_logistic_loop_epoch_vs_reference(kind, cls, d, opt, nb):
    from skge_amd.device import DeviceKG, LogisticLoopRunner, batch_sizes, epoch_records
    m = _model(cls, (N, N, M), d, rparam=0.01)
    upd = _updaters(m, opt)
    kg = DeviceKG(loop_kg(96 * nb), m.device)
    params, state = _snapshot(m, upd)
    r = LogisticLoopRunner(m, upd, kg, nb, seed=6)
    rec, n1 = epoch_records(kg, N, 6, 0)
    rec, n1 = rec.cpu().numpy(), n1.cpu().numpy()
    r.run(1)
    r.synchronize()
    want, start = 0.0, 0
    for c in batch_sizes(kg.T, nb):
        # xys += samplef(xys): the positives, then each positive's kept negatives
        trip = [tuple(int(v) for v in rec[j][:3]) for j in range(start, start + c)]
        ys = [1.0] * c
        for j in range(start, start + c):
            s, o, p, a = (int(x) for x in rec[j])
            if a >= 0:
                trip.append((a, o, p))
                ys.append(-1.0)
            if int(n1[j]) >= 0:
                trip.append((s, int(n1[j]), p))
                ys.append(-1.0)
        start += c
        before = {k: v.copy() for k, v in params.items()}
        _, li, grads = DR.logistic_step(kind, params, state, np.array(trip), np.array(ys), LR,
                                        opt, rparam=0.01)
        want += float(li)
    np.testing.assert_allclose(float(r.loss_total.item()), want, rtol=1e-5)
    _check_epoch(m, upd, params, state, before, grads, opt, nb,
                 "%s d%d logistic loop (%s)" % (kind, d, opt))


@pytest.mark.parametrize("d", [8, 132, 200])
@pytest.mark.parametrize("cls", ["DistMult", "ComplEx"])
def test_deterministic_forms_leave_identical_tables(cls, d, tmp_path):
    """Under set_deterministic(True) the sums are exact, so k_diag_pos and the
    explicit pairs (SKGE_DIAG_PAIRS=1) must leave the same bits.  The switch is
    read at create: one fresh child process per form.  The fixed-point
    accumulator takes widths that are multiples of 4 only (check_table), so the
    grid's 50 and 130 are replaced by 132 here: KM = 1, KM = 3 with a partly
    filled last register, KM = 4."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "diag_child.py")
    out, procs = {}, {}
    for form in ("0", "1"):   # side by side: most of a child's time is its start-up
        path = str(tmp_path / ("form%s.npz" % form))
        env = dict(os.environ, SKGE_DIAG_PAIRS=form)
        procs[form] = (subprocess.Popen([sys.executable, child, cls, str(d), path], env=env), path)
    for form, (proc, path) in procs.items():
        assert proc.wait(timeout=300) == 0, form
        out[form] = np.load(path)
    assert int(out["0"]["nviol"]) == int(out["1"]["nviol"]) > 0
    for pid in ("E", "R"):
        assert np.array_equal(out["0"][pid], out["1"][pid]), pid


SAMPLERS = [("typed", R.TYPED, 1, [0, 1]), ("lcwa", R.LCWA, 1, [0, 1]),
            ("random_2x012", R.RANDOM, 2, [0, 1, 2])]


@pytest.mark.parametrize("name,sampler,n,modes", SAMPLERS, ids=[s[0] for s in SAMPLERS])
@pytest.mark.parametrize("loop", ["pair", "logistic"])
@pytest.mark.parametrize("kind,cls", KINDS, ids=KIND_IDS)
def test_sampler_epochs_vs_reference(kind, cls, loop, name, sampler, n, modes):
    """Typed, LCWA and RandomModeSampler(2, [0, 1, 2]) draws on the device (the
    trainers' device_negatives=True route), one epoch of 3 batches (SGD, see
    LOOP_OPTS) on the samplers' shared KG, replayed from the device's own
    draws."""
    from skge_amd.device import (DeviceKG, LogisticLoopRunner, PairLoopRunner, batch_sizes,
                                 epoch_records_multi)
    d, sz = 50, (MR.N, MR.N, MR.M)
    m = _model(cls, sz, d, rparam=0.01)
    upd = _updaters(m, "sgd")
    kg = DeviceKG(MR.XS, m.device)
    rr = MR.REL_RANGE if sampler == R.TYPED else None
    params, state = _snapshot(m, upd)
    Runner = PairLoopRunner if loop == "pair" else LogisticLoopRunner
    r = Runner(m, upd, kg, 3, seed=MR.SEED, sampler=sampler, negatives=(n, modes, rr))
    pos, neg = epoch_records_multi(kg, MR.N, MR.M, MR.SEED, 0, n, modes, sampler=sampler,
                                   rel_range=rr)
    pos, neg = pos.cpu().numpy().astype(np.int64), neg.cpu().numpy().astype(np.int64)
    r.run(1)
    r.synchronize()
    total, start = 0.0, 0
    for c in batch_sizes(MR.T, 3):
        if loop == "pair":
            pp, nn = MR.batch_pairs(pos, neg, modes, start, c)
            _, _, nv, _ = DR.pairwise_step(kind, params, state, np.array(pp), np.array(nn), LR,
                                           MARGIN, "sgd", rparam=0.01)
            total += nv
        else:
            trip, ys = MR.batch_triples(pos, neg, modes, start, c)
            _, li, _ = DR.logistic_step(kind, params, state, np.array(trip), np.array(ys), LR,
                                        "sgd", rparam=0.01)
            total += float(li)
        start += c
    if loop == "pair":
        assert int(r.nviol_total.item()) == total > 0
    else:
        np.testing.assert_allclose(float(r.loss_total.item()), total, rtol=1e-5)
    _check_epoch(m, upd, params, state, None, None, "sgd", 3,
                 "%s %s loop %s" % (kind, loop, name))


def test_trainer_runs_on_the_pair_loop_and_refuses_pipe():
    import skge_amd as S
    xs = [tuple(int(v) for v in t) for t in loop_kg().tolist()]
    for runner in ("auto", "pipe"):
        m = _model("ComplEx", (N, N, M), 50)
        tr = S.PairwiseStochasticTrainer(m, nbatches=3, max_epochs=1, learning_rate=LR,
                                         margin=MARGIN, samplef=S.RandomModeSampler(1, [0, 1], xs, (N, N, M)).sample,
                                         device_loop=True, device_runner=runner, file_grad=None,
                                         file_embed=None)
        if runner == "pipe":
            with pytest.raises(ValueError, match="'pairs'"):
                tr.fit(xs, [1.0] * len(xs))
        else:
            tr.fit(xs, [1.0] * len(xs))
            assert type(tr._runner).__name__ == "PairLoopRunner" and tr.nviolations > 0


# ---------------------------------------------------------------------------
# 3. evaluation
# ---------------------------------------------------------------------------
import test_diag_ref as TDR   # the cases whose open share the CPU test bounds


@pytest.mark.parametrize("model,n_ent,n_rel,d", TDR.EVAL_CASES)
def test_ranks_topk_and_relation_ranks_inside_the_envelope(model, n_ent, n_rel, d):
    import skge_amd as S
    cls = dict(KINDS)[model]
    E, Rt, test, known = DR.eval_case(model, n_ent, n_rel, d, TDR.NQ, 100 + d + n_ent)
    m = _model(cls, (n_ent, n_ent, n_rel), d, E, Rt)
    ev = S.FilteredRankingEval(test, known)
    from eval_ref import eval_order
    q = eval_order(test)
    lo, hi = DR.rank_envelope(model, E, Rt, q, known)
    got = ev.ranks(m)
    assert ((lo <= got) & (got <= hi)).all(), np.argwhere((got < lo) | (got > hi))[:5]
    rlo, rhi = DR.relation_envelope(model, E, Rt, q, known)
    rgot = ev.relation_ranks(m)
    assert ((rlo <= rgot) & (rgot <= rhi)).all()
    # every vector on pool -1: rank_known's integers
    none = -np.ones(len(q), dtype=np.int64)
    np.testing.assert_array_equal(ev.candidate_ranks(m, [[0]], none, none), got)
    typed = ev.typed_ranks(m)
    assert typed.shape == got.shape and (typed >= 1).all() and (typed <= got).all()
    # top-k: every forced member is returned
    lp = S.LinkPredictor(m, known)
    k = TDR.TOPK
    s, o, p = test[:, 0], test[:, 1], test[:, 2]
    tails, _ = lp.tails(s, p, k=k, filtered=False)
    heads, _ = lp.heads(o, p, k=k, filtered=False)
    rels, _ = lp.relations(s, o, k=k, filtered=False)
    for i, (si, oi, pi) in enumerate(test.tolist()):
        for slot, ids in (("tail", tails[i]), ("head", heads[i]), ("rel", rels[i])):
            forced, places = DR.topk_forced(model, E, Rt, si, oi, pi, slot, k)
            assert set(forced) <= set(ids[:places].tolist()), (i, slot)
    pool = np.arange(0, n_ent, 2)
    ct, _ = lp.tails(s[:4], p[:4], k=3, filtered=False, candidates=pool)
    assert set(ct.reshape(-1).tolist()) <= set(pool.tolist())


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("kind,cls", KINDS, ids=KIND_IDS)
def test_score_and_link_prediction(kind, cls, d):
    import skge_amd as S
    E, Rt = DR.tables(kind, N, M, d, 31 + d, scale=0.5)
    m = _model(cls, (N, N, M), d, E, Rt)
    rs = np.random.RandomState(d)
    trip = np.stack([rs.randint(N, size=1000), rs.randint(N, size=1000),
                     rs.randint(M, size=1000)], axis=1).astype(np.int32)
    parity_util.check(m.score(trip), DR.scores(kind, E, Rt, trip), "%s d%d score" % (kind, d))
    ys = np.where(rs.rand(1000) < 0.5, 1.0, -1.0)
    areas = S.LinkPredictionEval(trip, ys).scores(m)
    assert all(np.isfinite(float(a)) for a in np.ravel(np.asarray(areas, dtype=np.float64)))
    tc = S.TripleClassifier(m)
    tc.fit(trip, ys)
    assert 0.0 <= float(tc.accuracy(trip, ys)[0]) <= 1.0
    ids = S.Neighbours(m).topk(k=3, rows=np.arange(4))[0]
    assert tuple(np.asarray(ids.cpu() if torch.is_tensor(ids) else ids).shape) == (4, 3)


@pytest.mark.parametrize("kind,cls", KINDS, ids=KIND_IDS)
def test_checkpoint_round_trip(kind, cls, tmp_path):
    import skge_amd as S
    from skge_amd.param import normless1
    E, Rt = DR.tables(kind, N, M, 50, 41, scale=0.5)
    m = _model(cls, (N, N, M), 50, E, Rt, rparam=0.01)
    trip = np.stack([np.arange(200) % N, (7 * np.arange(200)) % N, np.arange(200) % M],
                    axis=1).astype(np.int32)
    before = m.score(trip).cpu().numpy()
    f = str(tmp_path / "m.pkl")
    m.save(f)
    m2 = S.Model.load(f)
    assert type(m2) is type(m) and m2.E.post is normless1 and m2.R.post is None
    assert np.array_equal(m2.score(trip).cpu().numpy(), before)
    g = str(tmp_path / "ref.pkl")
    m.save_reference(g)
    m3 = S.load_reference(g)
    assert type(m3) is type(m) and m3.E.post is normless1
    assert np.array_equal(m3.score(trip).cpu().numpy(), before)
