"""Device logistic loop (skge_triple_runner_*, LogisticLoopRunner, GPU) for
HolE and RESCAL against the fp64 oracle.

The runner draws the epoch's permutation and negatives on the device; the
same draws are exposed by skge_epoch_sample, so each test replays them on the
host the way StochasticTrainer._process_batch builds a batch
(skge/base.py:1293-1304, ``xys += samplef(xys)``: the batch's positives with
y = +1, then for each positive its s-corruption and its o-corruption with
y = -1, a negative missing after ntries draws simply absent,
skge/sample.py:41-46) and feeds them to oracle.logistic_step
(skge/hole.py:22-42, skge/rescal.py:37-76, skge/param.py:140-174) from the
device state snapshotted before the epoch.

Bar: the epoch's loss at rtol 1e-5 (test_gpu_models.py's logistic bar);
tables and AdaGrad state within 1e-5 + 1e-5|x| with the step-aware bound
(parity_util.check / check_step).
"""
import numpy as np
import pytest
import torch

import parity_util
from oracle import skge_oracle as O

pytestmark = pytest.mark.gpu

CLS = {"hole": "HolE", "rescal": "RESCAL"}
# (kind, SKGE_HOLE_TRIPLES): HolE's per-positive kernel, its explicit triples, RESCAL
FORMS = [("hole", None), ("hole", "1"), ("rescal", None)]


def _kg(n_ent, n_rel, T, seed=21):
    rs = np.random.RandomState(seed)
    seen, out = set(), []
    while len(out) < T:
        t = (int(rs.randint(n_ent)), int(rs.randint(n_ent)), int(rs.randint(n_rel)))
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def _form(monkeypatch, triples):
    if triples is None:
        monkeypatch.delenv("SKGE_HOLE_TRIPLES", raising=False)
    else:
        monkeypatch.setenv("SKGE_HOLE_TRIPLES", triples)
    monkeypatch.delenv("SKGE_HOLE_DIRECT", raising=False)


def _setup(kind, xs, n_ent, n_rel, d, opt, rparam=0.0, lr=0.1):
    import skge_amd as S
    from skge_amd.device import DeviceKG
    np.random.seed(42)
    m = getattr(S, CLS[kind])((n_ent, n_ent, n_rel), d, rparam=rparam)
    U = S.AdaGrad if opt == "adagrad" else S.SGD
    upd = {pid: U(p, lr) for pid, p in m.params.items()}
    return m, upd, DeviceKG(xs, m.device)


def _triples(rec, n1, start, count):
    """The batch's labelled triples in the reference's order, -1 negatives dropped."""
    trip = [tuple(int(x) for x in rec[j][:3]) for j in range(start, start + count)]
    for j in range(start, start + count):
        s, o, p, a = (int(x) for x in rec[j])
        b = int(n1[j])
        if a >= 0:
            trip.append((a, o, p))
        if b >= 0:
            trip.append((s, b, p))
    ys = np.concatenate([np.ones(count), -np.ones(len(trip) - count)])
    return np.array(trip, dtype=np.int64), ys


def _snapshot(m, upd):
    params = {pid: p.data.detach().cpu().numpy().astype(np.float64) for pid, p in m.params.items()}
    state = {pid: upd[pid].p2.detach().cpu().numpy().astype(np.float64)
             for pid in m.params if getattr(upd[pid], "p2", None) is not None}
    return params, state


def _oracle_epoch(kind, params, state, rec, n1, sizes, opt, rparam=0.0, lr=0.1):
    """Chain the epoch's batches through the oracle; returns (loss, before, grads)
    of the last batch with the epoch's loss."""
    loss, start, before, grads = 0.0, 0, None, None
    for c in sizes:
        trip, ys = _triples(rec, n1, start, c)
        start += c
        before = {k: v.copy() for k, v in params.items()}
        _, li, grads = O.logistic_step(kind, params, state, trip, ys, lr, opt, rparam=rparam)
        loss += float(li)
    return loss, before, grads


def _epoch_vs_oracle(kind, m, upd, runner, kg, n_ent, seed, epoch, nb, opt, what, ntries=100,
                     rparam=0.0):
    """Run epoch `epoch` (0-based; the runner's key is at it) on the device and
    replay its batches through the oracle from the device state before it.
    Returns the epoch's records."""
    from skge_amd.device import batch_sizes, epoch_records
    params, state = _snapshot(m, upd)
    if opt == "sgd":
        state = {k: np.zeros_like(v) for k, v in params.items()}
    rec, n1 = epoch_records(kg, n_ent, seed, epoch, ntries)
    rec, n1 = rec.cpu().numpy(), n1.cpu().numpy()
    runner.loss_total.zero_()
    runner.run(1)
    runner.synchronize()
    assert int(runner.epoch_key.item()) == epoch + 1
    got_loss = float(runner.loss_total.item())
    want_loss, before, grads = _oracle_epoch(kind, params, state, rec, n1,
                                             batch_sizes(kg.T, nb), opt, rparam)
    print("%s: loss %.9g want %.9g" % (what, got_loss, want_loss))
    np.testing.assert_allclose(got_loss, want_loss, rtol=1e-5, err_msg=what)
    for pid in m.params:
        if nb == 1:     # one step from the snapshot: the step-aware bound
            parity_util.check_step(m.params[pid].data, params[pid], before[pid], grads[pid],
                                   state[pid], 0.1, "%s %s" % (what, pid),
                                   post=parity_util.POSTS[kind].get(pid), opt=opt)
        else:
            parity_util.check(m.params[pid].data, params[pid], "%s %s" % (what, pid),
                              lr=0.1 if opt == "adagrad" else None,
                              p2=state[pid] if opt == "adagrad" else None)
        if opt == "adagrad":
            parity_util.check(upd[pid].p2, state[pid], "%s p2 %s" % (what, pid))
    for acc in m._acc.values():   # accumulators drained after every batch
        assert int(acc.cnt.abs().sum().item()) == 0
    return rec, n1


def _runner(m, upd, kg, nb, seed, ntries=100):
    from skge_amd.device import LogisticLoopRunner
    return LogisticLoopRunner(m, upd, kg, nb, seed=seed, ntries=ntries)


# ---- 1. AdaGrad, one batch per epoch, from device state ----

@pytest.mark.parametrize("kind,triples", FORMS)
@pytest.mark.parametrize("n_ent,n_rel,d,T", [(400, 18, 200, 350), (300, 7, 40, 300)])
def test_adagrad_batches_vs_oracle_from_device_state(kind, triples, n_ent, n_rel, d, T,
                                                     monkeypatch):
    """One batch of T positives (3T labelled triples) per epoch, 3 epochs, each
    replayed from the device state (parameters AND AdaGrad state) before it.
    d = 200: HolE's FFT kernels (per-positive and explicit), RESCAL's MFMA path."""
    _form(monkeypatch, triples)
    m, upd, kg = _setup(kind, _kg(n_ent, n_rel, T), n_ent, n_rel, d, "adagrad")
    r = _runner(m, upd, kg, 1, 41)
    with torch.cuda.stream(r.stream):
        for e in range(3):
            _epoch_vs_oracle(kind, m, upd, r, kg, n_ent, 41, e, 1, "adagrad",
                             "%s/%s logistic loop d%d e%d" % (kind, triples, d, e))


# ---- 2. split geometry and the chain ----

@pytest.mark.parametrize("kind,triples", FORMS)
def test_split_geometry_and_chain_sgd(kind, triples, monkeypatch):
    """T = 500 at nbatches = 3: batches of 166, 166, 166 and the remainder of 2
    (np.split, skge/base.py:1246-1268).  SGD keeps the 4-batch oracle chain
    linear; an epoch is trained first so the tables have moved."""
    from skge_amd.device import batch_sizes
    _form(monkeypatch, triples)
    n_ent, n_rel, d, T = 400, 18, 200, 500
    assert batch_sizes(T, 3) == [166, 166, 166, 2]
    m, upd, kg = _setup(kind, _kg(n_ent, n_rel, T), n_ent, n_rel, d, "sgd")
    r = _runner(m, upd, kg, 3, 42)
    with torch.cuda.stream(r.stream):
        r.run(1)
        r.synchronize()
        _epoch_vs_oracle(kind, m, upd, r, kg, n_ent, 42, 1, 3, "sgd",
                         "%s/%s logistic loop sgd 4 batches" % (kind, triples))


# ---- 3. skipped negatives ----

def _dense_kg():
    """N = 8, M = 2.  Relation 0 holds all 64 (s, o): every corruption of a
    relation-0 positive is a training triple, so both draws end at -1.
    Relation 1 holds (i, i+1) and (i, i+3) mod 8: no full row or column."""
    xs = [(s, o, 0) for s in range(8) for o in range(8)]
    xs += [(i, (i + 1) % 8, 1) for i in range(8)] + [(i, (i + 3) % 8, 1) for i in range(8)]
    return xs


@pytest.mark.parametrize("kind,triples", FORMS)
@pytest.mark.parametrize("d", [40, 200])
def test_skipped_negatives_vs_oracle(kind, triples, d, monkeypatch):
    """ntries = 4, two batches of 40, AdaGrad.  The AdaGrad state starts at 0.01
    on the device (it is part of the snapshot the oracle starts from), so
    H >= 0.1 and the two-batch chain cannot turn the fp32 rounding of a
    near-zero gradient into a visible step: from p2 = 0, an element whose two
    gradients are both ~1e-6 takes lr * rounding / H ~ 1e-4 of error (measured:
    RESCAL d = 200, 5 of W's 80000 elements, max 1.8e-4, every other element
    and the loss inside the bar), which is why the chains elsewhere use SGD."""
    _form(monkeypatch, triples)
    xs = _dense_kg()
    m, upd, kg = _setup(kind, xs, 8, 2, d, "adagrad")
    for u in upd.values():
        u.p2.fill_(0.01)
    r = _runner(m, upd, kg, 2, 43, ntries=4)
    with torch.cuda.stream(r.stream):
        rec, n1 = _epoch_vs_oracle(kind, m, upd, r, kg, 8, 43, 0, 2, "adagrad",
                                   "%s/%s logistic loop skipped d%d" % (kind, triples, d), ntries=4)
    rel0 = rec[:, 2] == 0
    assert rel0.sum() == 64
    assert (rec[rel0, 3] == -1).all() and (n1[rel0] == -1).all()
    assert (rec[~rel0, 3] >= 0).sum() + (n1[~rel0] >= 0).sum() > 0   # not vacuous


@pytest.mark.parametrize("kind,d", [("hole", 200), ("hole", 40), ("hole", 28), ("hole", 30),
                                    ("rescal", 200), ("rescal", 40)])
def test_triple_step_skips_relation_minus_one(kind, d):
    """skge_triple_step with some relations set to -1 (their s and o set to
    entities 0 and 1: read as rows, they would show in those rows' sums and
    counts) against oracle.logistic_step on the list with those rows removed.  d = 200 / 40:
    k_hole_triple_fft; 28: the register-tiled HolE kernel; 30: the generic
    one; RESCAL: the MFMA path's bucketing and k_rescal_logistic."""
    n_ent, n_rel, B = 300, 7, 120
    xs = _kg(n_ent, n_rel, 3 * B, seed=5)
    m, upd, _ = _setup(kind, xs[:4], n_ent, n_rel, d, "adagrad")
    trip = np.array(xs, dtype=np.int32)
    ys = np.concatenate([np.ones(B), -np.ones(2 * B)]).astype(np.float32)
    skip = np.zeros(3 * B, dtype=bool)
    skip[np.random.RandomState(3).choice(np.arange(B, 3 * B), B // 2, replace=False)] = True
    dev_trip = trip.copy()
    dev_trip[skip] = (0, 1, -1)
    params, state = _snapshot(m, upd)
    before = {k: v.copy() for k, v in params.items()}
    loss = torch.zeros(1, dtype=torch.float32, device=m.device)
    m._logistic_step(torch.as_tensor(dev_trip, device=m.device),
                     torch.as_tensor(ys, device=m.device), upd, loss)
    torch.cuda.synchronize()
    _, want, grads = O.logistic_step(kind, params, state, trip[~skip].astype(np.int64),
                                     ys[~skip].astype(np.float64), 0.1, "adagrad")
    np.testing.assert_allclose(float(loss.item()), want, rtol=1e-5)
    for pid in m.params:
        what = "%s d%d triple_step skip %s" % (kind, d, pid)
        parity_util.check_step(m.params[pid].data, params[pid], before[pid], grads[pid],
                               state[pid], 0.1, what, post=parity_util.POSTS[kind].get(pid))
        parity_util.check(upd[pid].p2, state[pid], what + " p2")
    for acc in m._acc.values():
        assert int(acc.cnt.abs().sum().item()) == 0


@pytest.mark.parametrize("kind,d", [("hole", 40), ("hole", 30), ("rescal", 24)])
def test_gradients_skip_relation_minus_one(kind, d):
    """The reference-protocol path (model._gradients: skge_triple_grad, and for
    RESCAL the per-triple kernel with skge_rescal_wgrad) with relations set to
    -1 against the oracle's gradients of the list without those rows."""
    n_ent, n_rel, B = 200, 5, 60
    xs = _kg(n_ent, n_rel, 3 * B, seed=6)
    m, _, _ = _setup(kind, xs[:4], n_ent, n_rel, d, "adagrad")
    ys = np.concatenate([np.ones(B), -np.ones(2 * B)])
    skip = np.zeros(3 * B, dtype=bool)
    skip[np.random.RandomState(4).choice(np.arange(B, 3 * B), B // 2, replace=False)] = True
    xys = [(((0, 1, -1) if skip[i] else xs[i]), float(ys[i]))
           for i in range(3 * B)]
    params = {pid: p.data.detach().cpu().numpy().astype(np.float64) for pid, p in m.params.items()}
    got = m._gradients(xys)
    keep = np.array(xs, dtype=np.int64)[~skip]
    fn = O.hole_gradients if kind == "hole" else O.rescal_gradients
    _, want_loss, want = fn(params["E"], params[m.rel_id], keep, ys[~skip])
    np.testing.assert_allclose(m.loss, want_loss, rtol=1e-5)
    for pid in m.params:
        g, idx = got[pid]
        wg, widx = want[pid]
        assert np.array_equal(idx.cpu().numpy(), np.asarray(widx))
        parity_util.check(g, wg, "%s d%d _gradients skip %s" % (kind, d, pid))


# ---- 4. coinciding rows ----

def test_coinciding_rows_per_positive_kernel(monkeypatch):
    """N = 3, M = 1: positives with s == o, and corruptions that land on the
    positive's other entity (s' == o, o' == s), through the per-positive HolE
    kernel: separate slots and atomic adds of one row must end with the sum
    and the count the explicit triples give."""
    _form(monkeypatch, None)
    import skge_amd as S
    from skge_amd.device import DeviceKG
    xs = [(0, 0, 0), (1, 2, 0), (2, 1, 0)]
    # (a one-relation table given as a value: the reference's squeezed init,
    # skge/param.py:23-51, would make a (1, d) shape a vector)
    np.random.seed(42)
    m = S.HolE((3, 3, 2), 40)
    m.add_param("R", None, value=m.R.data[:1].clone())
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    kg = DeviceKG(xs, m.device)
    assert m.R.shape == (1, 40)
    r = _runner(m, upd, kg, 1, 44)
    hits = 0
    with torch.cuda.stream(r.stream):
        for e in range(2):
            rec, n1 = _epoch_vs_oracle("hole", m, upd, r, kg, 3, 44, e, 1, "adagrad",
                                       "hole logistic loop coinciding rows e%d" % e)
            hits += int((rec[:, 0] == rec[:, 1]).sum() + (rec[:, 3] == rec[:, 1]).sum() +
                        (n1 == rec[:, 0]).sum())
    assert hits > 0


# ---- 5. rparam ----

@pytest.mark.parametrize("kind,triples", FORMS)
def test_rparam_vs_oracle(kind, triples, monkeypatch):
    _form(monkeypatch, triples)
    n_ent, n_rel, d, T = 300, 7, 40, 300
    m, upd, kg = _setup(kind, _kg(n_ent, n_rel, T), n_ent, n_rel, d, "adagrad", rparam=0.05)
    r = _runner(m, upd, kg, 1, 45)
    with torch.cuda.stream(r.stream):
        _epoch_vs_oracle(kind, m, upd, r, kg, n_ent, 45, 0, 1, "adagrad",
                         "%s/%s logistic loop rparam" % (kind, triples), rparam=0.05)


# ---- 6. trainer level ----

@pytest.mark.parametrize("kind", ["hole", "rescal"])
def test_trainer_device_loop_losses_vs_oracle(kind):
    import skge_amd as S
    from skge_amd.device import DeviceKG, LogisticLoopRunner, batch_sizes, epoch_records
    n_ent, n_rel, d, T = 300, 7, 40, 300
    xs = _kg(n_ent, n_rel, T)
    np.random.seed(42)
    m = getattr(S, CLS[kind])((n_ent, n_ent, n_rel), d)
    params = {pid: p.data.detach().cpu().numpy().astype(np.float64) for pid, p in m.params.items()}
    state = {k: np.zeros_like(v) for k, v in params.items()}
    seen = []
    tr = S.StochasticTrainer(m, device_loop=True, max_epochs=2, nbatches=3, seed=5,
                             samplef=S.RandomModeSampler(1, [0, 1], xs,
                                                         (n_ent, n_ent, n_rel)).sample,
                             post_epoch=[lambda t: seen.append((t.epoch, t.loss)) or True])
    tr.fit(xs, [1] * T)
    assert isinstance(tr._runner, LogisticLoopRunner)
    assert [e for e, _ in seen] == [1, 2]
    kg = DeviceKG(xs, m.device)
    for e in range(2):
        rec, n1 = epoch_records(kg, n_ent, 5, e)
        want, _, _ = _oracle_epoch(kind, params, state, rec.cpu().numpy(), n1.cpu().numpy(),
                                   batch_sizes(T, 3), "adagrad")
        print("%s trainer epoch %d: loss %.9g want %.9g" % (kind, e + 1, seen[e][1], want))
        np.testing.assert_allclose(seen[e][1], want, rtol=1e-5)


@pytest.mark.parametrize("why", ["samplef_none", "n2", "ym1"])
def test_trainer_ineligible_sampler_warns_and_trains(why):
    import skge_amd as S
    n_ent, n_rel, d, T = 40, 3, 16, 60
    xs = _kg(n_ent, n_rel, T)
    sz = (n_ent, n_ent, n_rel)
    np.random.seed(42)
    m = S.HolE(sz, d)
    E0 = m.E.data.clone()
    ys = [1] * T
    samplef = S.RandomModeSampler(1, [0, 1], xs, sz).sample
    if why == "samplef_none":
        samplef = None
    elif why == "n2":
        samplef = S.RandomModeSampler(2, [0, 1], xs, sz).sample
    else:
        ys[3] = -1
    tr = S.StochasticTrainer(m, device_loop=True, max_epochs=1, nbatches=3, samplef=samplef)
    with pytest.warns(UserWarning, match="device_loop"):
        tr.fit(xs, ys)
    assert tr._runner is None
    assert not torch.equal(E0, m.E.data)
    assert np.isfinite(m.E.data.cpu().numpy()).all()


def test_trainer_transe_raises():
    import skge_amd as S
    xs = _kg(40, 3, 60)
    np.random.seed(42)
    m = S.TransE((40, 40, 3), 16)
    tr = S.StochasticTrainer(m, device_loop=True, max_epochs=1, nbatches=3,
                             samplef=S.RandomModeSampler(1, [0, 1], xs, (40, 40, 3)).sample)
    with pytest.raises(NotImplementedError):
        tr.fit(xs, [1] * 60)


def test_pairwise_trainer_device_loop_keeps_its_runner():
    import skge_amd as S
    from skge_amd.device import PairLoopRunner
    xs = _kg(200, 5, 600)
    np.random.seed(42)
    m = S.RESCAL((200, 200, 5), 16)
    tr = S.PairwiseStochasticTrainer(m, nbatches=5, max_epochs=1, margin=0.2, device_loop=True,
                                     seed=3, ntries=50,
                                     samplef=S.RandomModeSampler(1, [0, 1], xs,
                                                                 (200, 200, 5)).sample,
                                     file_grad=None, file_embed=None)
    assert tr.device_loop is True and tr.seed == 3 and tr.ntries == 50
    tr.fit(xs, [1] * len(xs))
    assert isinstance(tr._runner, PairLoopRunner)
    assert tr.nviolations > 0


# ---- 7. deterministic mode ----

@pytest.mark.parametrize("kind", ["hole", "rescal"])
def test_logistic_loop_bitwise_reproducible(kind, monkeypatch):
    """set_deterministic(True): exact fixed-point entity / relation sums, so two
    fresh models trained one epoch by the runner hold the same bits (HolE's
    per-positive kernel adds each contribution through the same accumulator)."""
    import skge_amd as S
    _form(monkeypatch, None)
    n_ent, n_rel, d, T = 60, 3, 40, 600
    xs = _kg(n_ent, n_rel, T, seed=16)
    prev = S.deterministic()
    S.set_deterministic(True)
    try:
        outs = []
        for _ in range(2):
            m, upd, kg = _setup(kind, xs, n_ent, n_rel, d, "adagrad", rparam=0.05)
            r = _runner(m, upd, kg, 4, 17)
            with torch.cuda.stream(r.stream):
                r.run(1)
            r.synchronize()
            outs.append({pid: p.data.cpu().numpy().copy() for pid, p in m.params.items()})
    finally:
        S.set_deterministic(prev)
    for pid in outs[0]:
        assert np.array_equal(outs[0][pid], outs[1][pid]), pid
