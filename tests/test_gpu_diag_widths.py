"""DistMult and ComplEx on the device at every row width of
tests/diag_width_cases.py, against tests/diag_ref.py (fp64): KM = 2, 3, 4, 8
and 16, full registers and rows that end one element (DistMult) or one complex
component (ComplEx) into a register -- the layouts where a wrong zero fill, a
wrong `e < d` guard or a wrong lane partner of the ComplEx quad permutation
shows.  Bars are parity_util's, as tests/test_gpu_diag.py applies them; every
violation count must match exactly, which the CPU tests of the table make a
fair demand (tests/test_diag_width_cases.py: no decision is within rounding).

Per case: the explicit-pair step, the logistic step and the scores; at the
widths of LOOP_D the pair-loop epoch in both forms (k_diag_pos<*, 2>, and both
sides of the d <= 256 edge of k_diag_pos).  Then the records a sampler cannot
fill -- a corruption that was not drawn -- on a dense eight-entity KG.

Two things the epochs do NOT assert, on purpose:

* Bit-identical tables of the two forms at d = 257 / 258.  Past 256 both forms
  run the explicit pairs, but the rows are summed with fp32 atomics whose order
  differs from run to run, so two runs of the SAME kernels may differ in the
  last bit; the exact sums of the deterministic mode take widths that are
  multiples of 4 only.  What is exact is asserted instead: at 257 / 258 both
  settings of the switch count the violations of the one fp64 replay and stay
  within the bar of it, and in the deterministic mode the two forms leave
  identical bits at d = 256 (k_diag_pos<*, 4> against the explicit pairs) and
  at d = 260 (the first width past the edge that mode takes).
* k_diag_pos's `ms` / `mo` branches (a corruption that drew the id it
  replaces).  No public path reaches them: every sampler kind -- random, typed
  and LCWA, with negatives=None or not -- accepts a candidate c only if the
  corrupted triple is not in the KG's own triple set (sample_record,
  draw_pools, sample_slot: `!set_contains(...)`), and c equal to the replaced
  id gives back the positive, which is in that set.  The runners take their
  records from those samplers alone.  The branches mirror diag_acc_pair's
  merge of the explicit-pair kernel, which the forced pairs here do reach
  (neg == pos in one position is allowed there).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import diag_ref as DR
import diag_width_cases as W
import parity_util
import test_gpu_diag as TG
from oracle import skge_oracle as O

pytestmark = pytest.mark.gpu

LR = TG.LR
RPARAM = 0.01
SZ = (W.N, W.N, W.M)


def _model(c, E=None, Rt=None):
    m = TG._model(c.cls, SZ, c.d, E, Rt, rparam=RPARAM)
    m.add_hyperparam("margin", c.margin)
    return m


# ---------------------------------------------------------------------------
# 1. the per-batch step kernels and the score kernel, every case
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("cid", W.IDS)
def test_explicit_pair_step(cid):
    """k_pair_grad<MODEL, KM> through _pairwise_gradients and the fused
    _pairwise_step (AdaGrad, rparam 0.01)"""
    c = W.BY_ID[cid]
    E, Rt = W.tables(c)
    pos, neg = W.pairs(c)
    m = _model(c, E, Rt)
    upd = TG._updaters(m, "adagrad")
    what = "%s pairwise" % cid
    g = m._pairwise_gradients([(tuple(x), 1.0) for x in pos.tolist()],
                              [(tuple(x), -1.0) for x in neg.tolist()])
    ps, ns, nv, want = DR.pairwise_gradients(c.model, E, Rt, pos, neg, c.margin, rparam=RPARAM)
    parity_util.check(m._pscore, ps, what + " pscore")
    parity_util.check(m._nscore, ns, what + " nscore")
    assert m.nviolations == nv and 0 < nv < W.P
    TG._check_grads(g, want, what)
    params, state = TG._snapshot(m, upd)
    before = {k: v.copy() for k, v in params.items()}
    nviol = torch.zeros(1, dtype=torch.int32, device=m.device)
    m._pairwise_step(torch.as_tensor(pos.astype(np.int32), device=m.device),
                     torch.as_tensor(neg.astype(np.int32), device=m.device), upd, nviol)
    _, _, nv2, grads = DR.pairwise_step(c.model, params, state, pos, neg, LR, c.margin, "adagrad",
                                        rparam=RPARAM)
    assert int(nviol.item()) == nv2 == nv
    TG._check_params(m, upd, params, state, before, grads, "adagrad", what + " step")
    for acc in m._acc.values():
        assert int(acc.cnt.abs().sum().item()) == 0


@pytest.mark.parametrize("cid", W.IDS)
def test_logistic_step(cid):
    """k_triple_grad<MODEL, KM> through _gradients and the fused _logistic_step"""
    c = W.BY_ID[cid]
    E, Rt = W.tables(c)
    trip, ys = W.labelled(c)
    m = _model(c, E, Rt)
    upd = TG._updaters(m, "adagrad")
    what = "%s logistic" % cid
    g = m._gradients([(tuple(t), float(y)) for t, y in zip(trip.tolist(), ys.tolist())])
    sc, loss, want = DR.gradients(c.model, E, Rt, trip, ys, rparam=RPARAM)
    parity_util.check(m._score, sc, what + " score")
    np.testing.assert_allclose(m.loss, loss, rtol=1e-5)
    TG._check_grads(g, want, what)
    params, state = TG._snapshot(m, upd)
    before = {k: v.copy() for k, v in params.items()}
    dl = torch.zeros(1, dtype=torch.float32, device=m.device)
    m._logistic_step(torch.as_tensor(trip.astype(np.int32), device=m.device),
                     torch.as_tensor(ys.astype(np.float32), device=m.device), upd, dl)
    _, loss2, grads = DR.logistic_step(c.model, params, state, trip, ys, LR, "adagrad",
                                       rparam=RPARAM)
    np.testing.assert_allclose(float(dl.item()), loss2, rtol=1e-5)
    TG._check_params(m, upd, params, state, before, grads, "adagrad", what + " step")
    for acc in m._acc.values():
        assert int(acc.cnt.abs().sum().item()) == 0


@pytest.mark.parametrize("cid", W.IDS)
def test_scores(cid):
    """k_score_diag<MODEL, KM>"""
    c = W.BY_ID[cid]
    E, Rt = W.tables(c)
    trip = W.score_triples(c)
    got = _model(c, E, Rt).score(trip)
    parity_util.check(got, DR.scores(c.model, E, Rt, trip), "%s score" % cid)


# ---------------------------------------------------------------------------
# 2. the pair-loop epoch at the widths of LOOP_D
# ---------------------------------------------------------------------------
NB, BATCH = 3, 64


def _decisions_clear(model, km, params, pos, neg, margin, what):
    """No margin decision of the batch is within rounding of the fp32 path:
    per pair, |f(n) + margin - f(p)| exceeds the worst fp32 error of the two
    scores through the sigmoid (slope <= 1/4), (KM + 10) u (A_p + A_n) / 4
    (diag_width_cases.score_error_bound), plus an ulp each for the sigmoid's
    own rounding.  The pairs are the device's own draws, so this is judged
    here, before the counts are compared."""
    E, R = params["E"], params["R"]
    pf = O.Sigmoid.f(DR.scores(model, E, R, pos))
    nf = O.Sigmoid.f(DR.scores(model, E, R, neg))
    err = (km + 10) * DR.U32 * (W.abs_scores(model, E, R, pos) +
                                W.abs_scores(model, E, R, neg)) / 4 + 4 * DR.U32
    gap = np.abs(nf + margin - pf)
    assert (gap > err).all(), (what, float((gap - err).min()))


def _pair_epoch(c, form, monkeypatch, seed=5):
    """One SGD epoch of 3 batches of 64 from the case's tables; returns the
    model, the runner's violation count and the fp64 replay (params,
    violations) from the device's own records."""
    from skge_amd.device import DeviceKG, PairLoopRunner, batch_sizes, epoch_records
    monkeypatch.setenv("SKGE_DIAG_PAIRS", "1" if form == "pairs" else "0")
    E, Rt = W.tables(c)
    m = _model(c, E, Rt)
    upd = TG._updaters(m, "sgd")
    kg = DeviceKG(W.loop_kg(NB * BATCH), m.device)
    params, state = TG._snapshot(m, upd)
    r = PairLoopRunner(m, upd, kg, NB, seed=seed)
    rec, n1 = epoch_records(kg, W.N, seed, 0)
    rec, n1 = rec.cpu().numpy(), n1.cpu().numpy()
    with torch.cuda.stream(r.stream):
        r.run(1)
    r.synchronize()
    want_v, start = 0, 0
    for b, cnt in enumerate(batch_sizes(kg.T, NB)):
        assert cnt == BATCH
        pos, neg = TG._pairs_of(rec, n1, start, cnt)
        start += cnt
        _decisions_clear(c.model, c.km, params, pos, neg, c.margin, "%s batch %d" % (c.id, b))
        _, _, nv, _ = DR.pairwise_step(c.model, params, state, pos, neg, LR, c.margin, "sgd",
                                       rparam=RPARAM)
        want_v += nv
    return m, upd, int(r.nviol_total.item()), params, want_v


@pytest.mark.parametrize("form", ["pos", "pairs"])
@pytest.mark.parametrize("cid", W.LOOP_IDS)
def test_pair_loop_epoch(cid, form, monkeypatch):
    c = W.BY_ID[cid]
    m, upd, got_v, params, want_v = _pair_epoch(c, form, monkeypatch)
    assert got_v == want_v and 0 < want_v < 2 * NB * BATCH
    TG._check_epoch(m, upd, params, None, None, None, "sgd", NB,
                    "%s pair loop (%s)" % (cid, form))


@pytest.mark.parametrize("d", [256, 260])
@pytest.mark.parametrize("cls", ["DistMult", "ComplEx"])
def test_deterministic_forms_leave_identical_tables_around_the_edge(cls, d, tmp_path):
    """test_gpu_diag's deterministic comparison (diag_child.py, one child per
    form) at the edge of k_diag_pos, KM = 4 full, and at the first width past
    it that the fixed-point accumulator takes, KM = 8: identical bits."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "diag_child.py")
    out, procs = {}, {}
    for form in ("0", "1"):
        path = str(tmp_path / ("form%s.npz" % form))
        env = dict(os.environ, SKGE_DIAG_PAIRS=form)
        procs[form] = (subprocess.Popen([sys.executable, child, cls, str(d), path], env=env), path)
    for form, (proc, path) in procs.items():
        assert proc.wait(timeout=300) == 0, form
        out[form] = np.load(path)
    assert int(out["0"]["nviol"]) == int(out["1"]["nviol"]) > 0
    if d > W.DIAG_POS_MAX_D:      # the switch selects nothing here: the same graph
        assert int(out["0"]["nlaunch"]) == int(out["1"]["nlaunch"])
    for pid in ("E", "R"):
        assert np.array_equal(out["0"][pid], out["1"][pid]), pid


# ---------------------------------------------------------------------------
# 3. corruptions that were not drawn: the dense KG, N = 8, M = 2
# ---------------------------------------------------------------------------
DENSE_SZ = (W.DENSE_N, W.DENSE_N, W.DENSE_M)
NTRIES = 4
DENSE_NB = 2


def _dense(cls, d, seed):
    from skge_amd.device import DeviceKG, epoch_records
    m = TG._model(cls, DENSE_SZ, d, rparam=RPARAM)
    upd = TG._updaters(m, "sgd")
    kg = DeviceKG(W.dense_kg(), m.device)
    rec, n1 = epoch_records(kg, W.DENSE_N, seed, 0, ntries=NTRIES)
    rec, n1 = rec.cpu().numpy(), n1.cpu().numpy()
    # the records the test is about: -1 by construction, and others with a draw
    no_s, no_o = W.undrawn(rec, n1)
    assert no_s.sum() == W.DENSE_N and no_o.sum() == W.DENSE_N
    assert (rec[no_s, 3] == -1).all() and (n1[no_o] == -1).all()
    assert (rec[~no_s, 3] >= 0).any() and (n1[~no_o] >= 0).any()
    assert sorted(map(tuple, rec[:, :3].tolist())) == sorted(map(tuple, W.dense_kg().tolist()))
    return m, upd, kg, rec, n1


@pytest.mark.parametrize("form", ["pos", "pairs"])
@pytest.mark.parametrize("d", [50, 130])
@pytest.mark.parametrize("kind,cls", TG.KINDS, ids=TG.KIND_IDS)
def test_undrawn_corruptions_pair_loop(kind, cls, d, form, monkeypatch):
    """k_diag_pos's neg = -1 handling (the row substitution, slot count 0, no
    violation) and the explicit-pair builder's, against the fp64 replay in
    which _pairs_of drops the missing pair."""
    from skge_amd.device import PairLoopRunner, batch_sizes
    monkeypatch.setenv("SKGE_DIAG_PAIRS", "1" if form == "pairs" else "0")
    m, upd, kg, rec, n1 = _dense(cls, d, 5)
    params, state = TG._snapshot(m, upd)
    r = PairLoopRunner(m, upd, kg, DENSE_NB, seed=5, ntries=NTRIES)
    with torch.cuda.stream(r.stream):
        r.run(1)
    r.synchronize()
    want_v, start, npairs = 0, 0, 0
    for b, cnt in enumerate(batch_sizes(kg.T, DENSE_NB)):
        pos, neg = TG._pairs_of(rec, n1, start, cnt)
        start += cnt
        npairs += len(pos)
        _decisions_clear(kind, W.km_for(d), params, pos, neg, TG.MARGIN,
                         "%s d%d dense batch %d" % (kind, d, b))
        _, _, nv, _ = DR.pairwise_step(kind, params, state, pos, neg, LR, TG.MARGIN, "sgd",
                                       rparam=RPARAM)
        want_v += nv
    assert npairs < 2 * kg.T          # some pairs are missing
    assert int(r.nviol_total.item()) == want_v > 0
    TG._check_epoch(m, upd, params, None, None, None, "sgd", DENSE_NB,
                    "%s d%d undrawn pair loop (%s)" % (kind, d, form))


@pytest.mark.parametrize("d", [50, 130])
@pytest.mark.parametrize("kind,cls", TG.KINDS, ids=TG.KIND_IDS)
def test_undrawn_corruptions_logistic_loop(kind, cls, d):
    """the skipped triple of k_triple_grad (relation -1: slots that name no
    row, coefficient 0)"""
    from skge_amd.device import LogisticLoopRunner, batch_sizes
    m, upd, kg, rec, n1 = _dense(cls, d, 6)
    params, state = TG._snapshot(m, upd)
    r = LogisticLoopRunner(m, upd, kg, DENSE_NB, seed=6, ntries=NTRIES)
    r.run(1)
    r.synchronize()
    want, start, ntrip = 0.0, 0, 0
    for cnt in batch_sizes(kg.T, DENSE_NB):
        trip = [tuple(int(v) for v in rec[j][:3]) for j in range(start, start + cnt)]
        ys = [1.0] * cnt
        for j in range(start, start + cnt):
            s, o, p, a = (int(x) for x in rec[j])
            if a >= 0:
                trip.append((a, o, p))
                ys.append(-1.0)
            if int(n1[j]) >= 0:
                trip.append((s, int(n1[j]), p))
                ys.append(-1.0)
        start += cnt
        ntrip += len(trip)
        _, li, _ = DR.logistic_step(kind, params, state, np.array(trip), np.array(ys), LR, "sgd",
                                    rparam=RPARAM)
        want += float(li)
    assert ntrip < 3 * kg.T
    np.testing.assert_allclose(float(r.loss_total.item()), want, rtol=1e-5)
    TG._check_epoch(m, upd, params, None, None, None, "sgd", DENSE_NB,
                    "%s d%d undrawn logistic loop" % (kind, d))
