"""Self-adversarial negative-sampling loss on the device (TransE-L1 / -L2,
RotatE): k_sadv_pos through Model._sadv_gradients / _sadv_step, the device loop
(SadvLoopRunner) and SelfAdversarialTrainer, against the fp64 restatement of
tests/sadv_ref.py at its derived rounding bounds.  The cases, their input
conditions and the bounds are chosen in sadv_ref.py on the CPU
(tests/test_sadv_ref.py judges them); every check's headroom goes to
parity_util.RECORDS."""
import numpy as np
import pytest
import torch

import sadv_ref as SR
import test_gpu_pairloop as TP

pytestmark = pytest.mark.gpu

LR = 0.1
DEV = "cuda:0"


def make_model(form, n_ent, n_rel, d, E, R, gamma, alpha):
    import skge_amd as S
    np.random.seed(1)
    sz = (n_ent, n_ent, n_rel)
    # (d = 1: the host initialiser squeezes a one-column table, the reference's quirk)
    kw = {"init": "device_nunif"} if d == 1 or n_rel == 1 else {}
    m = S.RotatE(sz, d) if form == "rot" else S.TransE(sz, d, l1=(form == "l1"), **kw)
    m.E.data.copy_(torch.from_numpy(E.astype(np.float32)))
    m.R.data.copy_(torch.from_numpy(R.astype(np.float32)))
    m.add_hyperparam("gamma", gamma)
    m.add_hyperparam("alpha", alpha)
    return m


def make_updaters(m, opt, seed=None):
    import skge_amd as S
    if opt == "sgd":
        return {pid: S.SGD(p, LR) for pid, p in m.params.items()}, None
    upd = {pid: S.AdaGrad(p, LR) for pid, p in m.params.items()}
    state = {}
    for i, pid in enumerate(("E", "R")):
        state[pid] = SR.adagrad_state(tuple(m.params[pid].data.shape), (seed or 0) + i)
        upd[pid].p2.copy_(torch.from_numpy(state[pid].astype(np.float32)))
    return upd, state


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def check_gradients(m, form, E, R, pos, negK, modes, gamma, alpha, what):
    """_sadv_gradients against the restatement: scores (bits of model.score
    too), coefficients, loss, rows and ids."""
    got = m._sadv_gradients(pos, negK, modes)
    fw, grads = SR.gradients(form, E, R, pos, negK, modes, gamma, alpha)
    SR.check_scores(_np(m._pscore), fw["pphi"], what + " pscore")
    SR.check_scores(_np(m._nscore), fw["nphi"], what + " nscore")
    SR.check_coef(_np(m._coef), fw, what + " coef")
    assert np.all(_np(m._nscore)[~fw["valid"]] == 0) and np.all(_np(m._coef)[:, 1:][~fw["valid"]] == 0)
    ltol = SR.ATOL + SR.RTOL * abs(fw["loss"]) + len(pos) * (SR.ATOL + SR.RTOL * 12.0)
    SR._record(np.array([m.loss]), np.array([fw["loss"]]), np.array([ltol]), what + " loss")
    for pid in ("E", "R"):
        g, idx = got[pid]
        SR.check_rows(_np(g), idx.cpu().numpy(), grads[pid], what + " g" + pid)
    # the scores are model.score's bits
    trips = np.concatenate([fw["pos"], fw["neg"].reshape(-1, 3)[fw["valid"].reshape(-1)]])
    sc = m.score(trips).cpu().numpy()
    mine = np.concatenate([m._pscore.cpu().numpy(),
                           m._nscore.cpu().numpy().reshape(-1)[fw["valid"].reshape(-1)]])
    assert np.array_equal(sc, mine), what + ": scores differ from model.score's bits"
    return fw


def check_step(m, upd, state, form, E, R, pos, negK, modes, gamma, alpha, opt, what, flips=0):
    """_sadv_step against one restatement step from the same tables and state."""
    params = {"E": E.copy(), "R": R.copy()}
    st = ({k: v.copy() for k, v in state.items()} if state and state["E"] is not None
          else {"E": None, "R": None})
    before_cnt = {pid: np.asarray(m.params[pid].updateCounts).copy() for pid in ("E", "R")}
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    m._sadv_step(pos, negK, modes, upd, loss)
    fw, grads, pre = SR.step(form, params, st, pos, negK, modes, gamma, alpha, LR, opt)
    ltol = SR.ATOL + SR.RTOL * abs(fw["loss"]) + len(pos) * (SR.ATOL + SR.RTOL * 12.0)
    SR._record(_np(loss), np.array([fw["loss"]]), np.array([ltol]), what + " step loss")
    before = {"E": E, "R": R}
    for pid in ("E", "R"):
        SR.check_param(_np(m.params[pid].data), params[pid], before[pid], grads[pid], pre[pid],
                       st[pid], LR, opt, SR.posts(form)[pid], what + " " + pid, flips=flips)
        if opt == "adagrad":
            SR._record(_np(upd[pid].p2), st[pid], SR.ATOL + SR.RTOL * np.abs(st[pid]) +
                       np.zeros_like(st[pid]), what + " p2 " + pid)
            cnt = np.asarray(m.params[pid].updateCounts) - before_cnt[pid]
            want = np.zeros(len(cnt), dtype=cnt.dtype)
            want[grads[pid][1]] = 1
            assert np.array_equal(cnt, want), what + " updateCounts " + pid
    for acc in m._acc.values():   # accumulators drained
        assert int(acc.cnt.abs().sum().item()) == 0
    return fw, params, st


@pytest.mark.parametrize("form,d,K,modes", SR.step_cases(),
                         ids=["%s-d%d-K%d" % c[:3] for c in SR.step_cases()])
def test_step_parity(form, d, K, modes):
    E, R, pos, negK, gamma, alpha = SR.build_case(form, d, K, modes)
    SR.check_conditions(form, E, R, pos, negK, modes)
    what = "sadv %s d%d K%d" % (form, d, K)
    m = make_model(form, SR.N, SR.M, d, E, R, gamma, alpha)
    check_gradients(m, form, E, R, pos, negK, modes, gamma, alpha, what)
    for opt in ("sgd", "adagrad"):
        m = make_model(form, SR.N, SR.M, d, E, R, gamma, alpha)
        upd, state = make_updaters(m, opt, seed=d)
        check_step(m, upd, state, form, E, R, pos, negK, modes, gamma, alpha, opt,
                   what + " " + opt)


@pytest.mark.parametrize("name", sorted(SR.edge_records()))
@pytest.mark.parametrize("d", SR.EDGE_WIDTHS)
@pytest.mark.parametrize("form", SR.FORMS)
def test_edge_cases(form, d, name):
    """Hand-built records (sadv_ref.edge_records, the relation table of one row
    among them): _sadv_gradients and _sadv_step against the restatement."""
    E, R, pos, negK, modes, n_rel = SR.edge_case(form, d, name)
    SR.check_conditions(form, E, R, pos, negK, modes)
    what = "sadv edge %s d%d %s" % (form, d, name)
    m = make_model(form, SR.N, n_rel, d, E, R, 6.0, 1.0)
    check_gradients(m, form, E, R, pos, negK, modes, 6.0, 1.0, what)
    upd, state = make_updaters(m, "adagrad", seed=d)
    check_step(m, upd, state, form, E, R, pos, negK, modes, 6.0, 1.0, "adagrad", what)


@pytest.mark.parametrize("form", SR.FORMS)
def test_stability_on_the_device(form):
    """alpha = 8 with every phi_k near -40; gamma = 60; gamma + phi near -100:
    every output finite, coefficients within the bound."""
    d, K, modes = 200, 64, (0, 1)
    pos, negK = SR.records(K, modes, 5)
    rs = np.random.RandomState(5)
    if form == "rot":
        E, R = SR.RR.tables(SR.N, SR.M, d, 5, 3.0)        # phi about -40
    else:
        E = rs.uniform(-1, 1, (SR.N, d)).astype(np.float32).astype(np.float64)
        R = rs.uniform(-1, 1, (SR.M, d)).astype(np.float32).astype(np.float64)
        sc = 40.0 / -SR.phi(form, E, R, pos).mean()
        sc = sc if form == "l1" else np.sqrt(sc)
        E = (E * sc).astype(np.float32).astype(np.float64)
        R = (R * sc).astype(np.float32).astype(np.float64)
    for gamma, alpha in ((0.0, 8.0), (60.0, 1.0), (-60.0, 1.0)):
        m = make_model(form, SR.N, SR.M, d, E, R, gamma, alpha)
        m._sadv_gradients(pos, negK, modes)
        fw = SR.forward(form, E, R, pos, negK, modes, gamma, alpha)
        for t in (m._pscore, m._nscore, m._coef):
            assert torch.isfinite(t).all().item()
        assert np.isfinite(m.loss)
        what = "sadv stability %s g%g a%g" % (form, gamma, alpha)
        SR.check_coef(_np(m._coef), fw, what)
        w = _np(m._coef)[:, 1:] / np.maximum(SR.sigmoid(gamma + fw["nphi"]), 1e-300)
        if gamma >= 0:
            assert np.allclose(w.sum(axis=1), 1.0, atol=1e-4)


@pytest.mark.parametrize("form,d", [("l2", 200), ("rot", 200), ("rot", 258), ("l2", 258)])
def test_deterministic_mode_repeats_bits(form, d):
    import skge_amd as S
    K, modes = 6, (1, 0, 0)
    E, R, pos, negK, gamma, alpha = SR.build_case(form, d, K, modes)
    outs = []
    S.set_deterministic(True)
    try:
        for _ in range(2):
            m = make_model(form, SR.N, SR.M, d, E, R, gamma, 1.0)
            upd, _ = make_updaters(m, "adagrad", seed=d)
            loss = torch.zeros(1, dtype=torch.float32, device=DEV)
            m._sadv_step(pos, negK, modes, upd, loss)
            torch.cuda.synchronize()
            outs.append([m.E.data.cpu().numpy(), m.R.data.cpu().numpy(),
                         upd["E"].p2.cpu().numpy(), upd["R"].p2.cpu().numpy()])
    finally:
        S.set_deterministic(False)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert not np.array_equal(outs[0][0], E.astype(np.float32))


# ---- the device loop ----
LOOP_T, LOOP_NB, LOOP_SEED = 100, 3, 9
LOOP_XS = TP.make_kg(SR.N, SR.M, LOOP_T, seed=4)
LOOP_SAMPLERS = [("random", 3, [0, 1]), ("typed", 2, [0, 1, 2]), ("lcwa", 1, [0, 1])]


@pytest.mark.parametrize("det", [False, True], ids=["fp32", "deterministic"])
@pytest.mark.parametrize("kind,n,modes", LOOP_SAMPLERS, ids=[s[0] for s in LOOP_SAMPLERS])
@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("d", SR.LOOP_WIDTHS)
@pytest.mark.parametrize("form", SR.FORMS)
def test_device_loop_equals_replayed_steps(form, d, opt, kind, n, modes, det):
    import skge_amd as S
    from skge_amd import _lib as L
    from skge_amd.device import DeviceKG, SadvLoopRunner, batch_sizes, epoch_records_multi
    from skge_amd.sample import type_index
    code = {"random": L.SKGE_SAMPLER_RANDOM, "typed": L.SKGE_SAMPLER_TYPED,
            "lcwa": L.SKGE_SAMPLER_LCWA}[kind]
    rel_range = len(type_index(LOOP_XS)) if kind == "typed" and 2 in modes else None
    gamma, alpha = 6.0, 1.0
    # (the input conditions hold on every triple of N x N x M: the first batch's
    # tables are on the grid whatever the device draws; tests/test_sadv_ref.py)
    E, R = SR.loop_tables(form, d)
    S.set_deterministic(det)
    try:
        kg = DeviceKG(LOOP_XS, torch.device(DEV))
        a = make_model(form, SR.N, SR.M, d, E, R, gamma, alpha)
        upd_a, _ = make_updaters(a, opt, seed=d)
        r = SadvLoopRunner(a, upd_a, kg, LOOP_NB, seed=LOOP_SEED, sampler=code,
                           negatives=(n, modes, rel_range))
        assert type(r).__name__ == "SadvLoopRunner"
        with torch.cuda.stream(r.stream):
            r.run(1)
        r.synchronize()
        assert int(r.epoch_key.item()) == 1
        got_loss = float(r.loss_total.item())
        # the twin: the same records, batch by batch through _sadv_step
        b = make_model(form, SR.N, SR.M, d, E, R, gamma, alpha)
        upd_b, state = make_updaters(b, opt, seed=d)
        pos, neg = epoch_records_multi(kg, SR.N, SR.M, LOOP_SEED, 0, n, modes, 100, sampler=code,
                                       rel_range=rel_range)
        pos, neg = pos.cpu().numpy().astype(np.int64), neg.cpu().numpy().astype(np.int64)
        sizes = batch_sizes(LOOP_T, LOOP_NB)
        assert len(sizes) == 4 and sizes[-1] == 1      # three batches and a remainder
        start, want_loss = 0, 0.0
        Eb, Rb = E, R
        for bi, c in enumerate(sizes):
            fw, params, state = check_step(
                b, upd_b, state, form, Eb, Rb, pos[start:start + c], neg[start:start + c], modes,
                gamma, alpha, opt, "sadv loop %s d%d %s %s b%d" % (form, d, opt, kind, bi),
                flips=0 if bi == 0 else None)   # (None: sadv_ref.check_param's ceiling)
            want_loss += fw["loss"]
            start += c
            # the next restatement step starts from the twin's own fp32 tables
            Eb, Rb = _np(b.E.data), _np(b.R.data)
            if state["E"] is not None:
                state = {pid: _np(upd_b[pid].p2) for pid in ("E", "R")}
        torch.cuda.synchronize()
        ltol = SR.ATOL + SR.RTOL * abs(want_loss) + LOOP_T * (SR.ATOL + SR.RTOL * 12.0)
        SR._record(np.array([got_loss]), np.array([want_loss]), np.array([ltol]),
                   "sadv loop %s d%d %s %s loss_total" % (form, d, opt, kind))
        for pid in ("E", "R"):
            ga, gb = a.params[pid].data.cpu().numpy(), b.params[pid].data.cpu().numpy()
            if det:
                assert np.array_equal(ga, gb), pid
            else:
                assert np.abs(ga - gb).max() <= 1e-5, (pid, np.abs(ga - gb).max())
            assert np.array_equal(np.asarray(a.params[pid].updateCounts),
                                  np.asarray(b.params[pid].updateCounts))
    finally:
        S.set_deterministic(False)


# ---- the trainer ----
TRAIN_XS = TP.make_kg(SR.N, SR.M, 96, seed=6)


@pytest.mark.parametrize("device_loop", [False, True], ids=["per-batch", "device-loop"])
@pytest.mark.parametrize("form", SR.FORMS)
def test_trainer(form, device_loop, tmp_path):
    import skge_amd as S
    np.random.seed(3)
    sz = (SR.N, SR.N, SR.M)
    m = S.RotatE(sz, 16) if form == "rot" else S.TransE(sz, 16, l1=(form == "l1"))
    smp = S.RandomModeSampler(2, [0, 1, 2], TRAIN_XS, sz)
    losses = []
    tr = S.SelfAdversarialTrainer(m, gamma=4.0, alpha=0.5, samplef=smp.sample, nbatches=4,
                                  max_epochs=5, learning_rate=0.1, param_update=S.AdaGrad,
                                  post_epoch=[lambda t: losses.append(t.loss) or True],
                                  device_loop=device_loop, seed=2)
    tr.fit(TRAIN_XS, [1] * len(TRAIN_XS))
    torch.cuda.synchronize()
    if device_loop:
        assert type(tr._runner).__name__ == "SadvLoopRunner"
    print("sadv trainer %s %s losses %r" % (form, device_loop, losses))
    assert len(losses) == 5 and all(np.isfinite(losses)) and losses[-1] < losses[0]
    E = _np(m.E.data)
    upd = np.asarray(m.E.updateCounts) > 0
    assert upd.any() and np.allclose(np.sqrt((E[upd] ** 2).sum(axis=1)), 1.0, atol=1e-5)
    if form == "rot":
        assert np.allclose(np.abs(SR.RR.cplx(_np(m.R.data))), 1.0, atol=1e-5)
    f = str(tmp_path / "m.pkl")
    m.save(f)
    m2 = S.Model.load(f)
    assert (m2.gamma, m2.alpha) == (4.0, 0.5)
    xs = np.array(TRAIN_XS)
    ev = S.FilteredRankingEval(xs[:10], xs)
    ranks = ev.ranks(m)
    assert ranks.shape == (10, 4) and (ranks >= 1).all()
    ids, sc = S.LinkPredictor(m, xs).tails(xs[:10, 0], xs[:10, 2], k=3, filtered=False)
    assert np.asarray(ids).shape == (10, 3) and np.isfinite(np.asarray(sc)).all()


def test_trainer_refusals_and_fallback():
    import skge_amd as S
    sz = (SR.N, SR.N, SR.M)
    np.random.seed(3)
    smp = S.RandomModeSampler(1, [0, 1], TRAIN_XS, sz)
    for cls, args in ((S.HolE, (sz, 8)), (S.RESCAL, (sz, 8)), (S.DistMult, (sz, 8)),
                      (S.ComplEx, (sz, 8))):
        with pytest.raises(ValueError) as e:
            S.SelfAdversarialTrainer(cls(*args), samplef=smp.sample)
        assert cls.__name__ in str(e.value) and "StochasticTrainer" in str(e.value)
    m = S.TransE(sz, 8, l1=True)
    with pytest.raises(ValueError, match="samplef is None"):
        S.SelfAdversarialTrainer(m)
    with pytest.raises(ValueError, match="K = 66"):
        S.SelfAdversarialTrainer(m, samplef=S.RandomModeSampler(33, [0, 1], TRAIN_XS, sz).sample)
    with pytest.raises(ValueError, match="device_runner"):
        S.SelfAdversarialTrainer(m, samplef=smp.sample, device_runner="pipe")
    tr = S.SelfAdversarialTrainer(m, samplef=smp.sample, nbatches=4, max_epochs=1)
    with pytest.raises(ValueError, match="labelled negatives"):
        tr.fit(TRAIN_XS, [1] * 95 + [-1])
    # StochasticTrainer's RotatE refusal stays as it is
    with pytest.raises(ValueError, match="RotatE has no logistic trainer"):
        S.StochasticTrainer(S.RotatE(sz, 8), samplef=smp.sample).fit(TRAIN_XS, [1] * 96)

    class Mine(S.RandomModeSampler):
        def _sample(self, x, mode):
            return S.RandomModeSampler._sample(self, x, mode)

    mine = Mine(1, [0, 1], TRAIN_XS, sz)
    tr = S.SelfAdversarialTrainer(m, samplef=mine.sample, nbatches=4, max_epochs=1,
                                  device_loop=True)
    with pytest.warns(UserWarning, match="_sample is overridden"):
        tr.fit(TRAIN_XS, [1] * 96)
    assert tr._runner is None and np.isfinite(tr.loss) and tr.loss > 0
