"""CPU judge of tests/sadv_ref.py (the fp64 restatement of the self-adversarial
loss), of the input conditions of every GPU case, and of the host refusals of
skge_sadv_grad / skge_sadv_step / skge_sadv_runner_create and of
SelfAdversarialTrainer (no device: the library loads on a CPU machine, the
tables' pointers are fake and never read on the host)."""
import ctypes

import numpy as np
import pytest

import sadv_ref as SR

FAKE = ctypes.c_void_p(0x1000)


def _small(form, K=5, modes=(0, 1, 2), seed=3, d=8):
    d = d + d % 2
    pos, negK = SR.records(K, modes, seed, n_pos=6)
    trips = SR.case_triples(pos, negK, modes)
    E, R = (SR.rot_tables(d, trips, seed) if form == "rot"
            else SR.transe_tables(form, d, trips, seed))
    return E, R, pos, negK


@pytest.mark.parametrize("form", SR.FORMS)
def test_coefficients_are_the_derivative_with_the_weights_fixed(form):
    modes = (0, 1, 2)
    E, R, pos, negK = _small(form)
    gamma, alpha, h = 3.0, 1.0, 1e-5
    fw = SR.forward(form, E, R, pos, negK, modes, gamma, alpha)
    for j in range(len(pos)):
        K = negK.shape[1]
        want = np.concatenate([[fw["cpos"][j]], fw["cneg"][j]])
        for t in range(1 + K):
            dp = np.zeros(1 + K)
            dp[t] = h
            up = SR.loss_one(form, E, R, pos[j:j + 1], negK[j:j + 1], modes, gamma, fw["w"][j], dp)
            dn = SR.loss_one(form, E, R, pos[j:j + 1], negK[j:j + 1], modes, gamma, fw["w"][j], -dp)
            assert abs((up - dn) / (2 * h) - want[t]) < 1e-8, (j, t)
        # and L_j itself with its own weights
        assert abs(SR.loss_one(form, E, R, pos[j:j + 1], negK[j:j + 1], modes, gamma,
                               fw["w"][j]) - fw["Lj"][j]) < 1e-12


def test_weights_sum_to_one_and_special_cases():
    E, R, pos, negK = _small("l1")
    fw = SR.forward("l1", E, R, pos, negK, (0, 1, 2), 6.0, 1.0)
    kv = fw["valid"].sum(axis=1)
    assert np.allclose(fw["w"].sum(axis=1)[kv > 0], 1.0, atol=1e-14)
    assert np.all(fw["w"][~fw["valid"]] == 0) and np.all(fw["cneg"][~fw["valid"]] == 0)
    fw0 = SR.forward("l1", E, R, pos, negK, (0, 1, 2), 6.0, 0.0)
    for j in range(len(pos)):
        assert np.allclose(fw0["w"][j][fw0["valid"][j]], 1.0 / kv[j], atol=1e-15)
    E, R, pos, negK = _small("l2", K=1, modes=(0,))
    fw1 = SR.forward("l2", E, R, pos, negK, (0,), 0.0, 1.0)
    assert np.all(fw1["w"][fw1["valid"]] == 1.0)


@pytest.mark.parametrize("form", SR.FORMS)
def test_absent_slots_take_no_part(form):
    """K = 4 over (0, 1) with slots 1 and 2 absent == K = 2 of slots 0 and 3."""
    E, R, pos, negK = _small(form, K=4, modes=(0, 1))
    negK = np.abs(negK)
    four = negK.copy()
    four[:, 1:3] = -1
    two = negK[:, [0, 3]]
    fa, ga = SR.gradients(form, E, R, pos, four, (0, 1), 6.0, 1.0)
    fb, gb = SR.gradients(form, E, R, pos, two, (0, 1), 6.0, 1.0)
    assert np.array_equal(fa["Lj"], fb["Lj"]) and np.array_equal(fa["cpos"], fb["cpos"])
    assert np.array_equal(fa["cneg"][:, [0, 3]], fb["cneg"])
    for pid in ("E", "R"):
        assert np.array_equal(ga[pid][1], gb[pid][1]) and np.array_equal(ga[pid][3], gb[pid][3])
        assert np.allclose(ga[pid][0], gb[pid][0], atol=1e-15)


def test_no_valid_slot_leaves_the_positive_alone():
    E, R, pos, negK = _small("rot", K=3, modes=(0, 1, 2))
    none = np.full_like(negK, -1)
    fw, g = SR.gradients("rot", E, R, pos, none, (0, 1, 2), 6.0, 1.0)
    assert np.all(fw["cneg"] == 0) and np.all(fw["w"] == 0)
    assert np.allclose(fw["Lj"], SR.nls(6.0 + fw["pphi"]))
    # the positive's three rows, each occurrence counted once
    assert np.array_equal(g["E"][1], np.unique(pos[:, :2]))
    assert g["E"][3].sum() == 2 * len(pos) and g["R"][3].sum() == len(pos)


def test_stability():
    nphi = -40.0 + np.linspace(-0.5, 0.5, 64)[None, :]
    w = SR.weights(nphi, np.ones_like(nphi, dtype=bool), 8.0)
    assert np.all(np.isfinite(w)) and abs(w.sum() - 1.0) < 1e-13
    for x in (60.0, -100.0):
        assert np.isfinite(SR.nls(x)) and np.isfinite(SR.nls(-x))
    assert SR.nls(-100.0) == pytest.approx(100.0) and SR.nls(60.0) < 1e-25
    assert SR.sigmoid(-800.0) == 0.0 and SR.sigmoid(800.0) == 1.0


def test_counts_are_list_occurrences():
    """c == o under mode 0, c == s under mode 1, one id in two slots, o == s."""
    E, R, _, _ = _small("l1", K=4, modes=(0, 1))
    pos = np.array([[5, 7, 1], [9, 9, 2]])
    negK = np.array([[7, 5, 11, 11], [3, 3, -1, 4]])
    _, g = SR.gradients("l1", E, R, pos, negK, (0, 1), 0.0, 1.0)
    cnt = dict(zip(g["E"][1].tolist(), g["E"][3].tolist()))
    # positive 0: triples (5,7) (7,7) (5,5) (11,7) (5,11); positive 1: (9,9) (3,9) (9,3) (9,4)
    assert cnt == {5: 4, 7: 4, 11: 2, 9: 5, 3: 2, 4: 1}
    assert dict(zip(g["R"][1].tolist(), g["R"][3].tolist())) == {1: 5, 2: 4}


def test_input_conditions_hold_for_every_gpu_case():
    for form, d, K, modes in SR.step_cases():
        E, R, pos, negK, gamma, alpha = SR.build_case(form, d, K, modes)
        SR.check_conditions(form, E, R, pos, negK, modes)
        assert gamma in SR.GAMMAS and alpha in SR.ALPHAS
    seen = {(SR.build_case(f, d, K, m)[4:]) for f, d, K, m in SR.step_cases()}
    assert len(seen) == 4   # every (gamma, alpha) of {0, 6} x {0, 1} is run
    for form in SR.FORMS:
        for d in SR.EDGE_WIDTHS:
            for name in SR.edge_records():
                E, R, pos, negK, modes, n_rel = SR.edge_case(form, d, name)
                assert R.shape[0] == n_rel and pos[:, 2].max() < n_rel
                SR.check_conditions(form, E, R, pos, negK, modes)
        # the device loop's initial tables: every triple of N x N x M
        for d in SR.LOOP_WIDTHS:
            E, R = SR.loop_tables(form, d)
            SR.check_conditions_on(form, E, R, SR.all_triples())


# ---- host refusals (no device) ----

def _table(rows, d, slots, mode=0, post=0, replicas=1):
    from skge_amd import _lib as L
    t = L.SkgeTable()
    t.param = t.state = t.acc_sum = t.acc_cnt = 0x1000
    t.acc_touched = 0x1000 if slots else None
    t.rows, t.width, t.touched_cap = rows, d, 0   # the backstop: no slot fits
    t.acc_mode, t.acc_replicas, t.post, t.lr = mode, replicas, post, 0.1
    return t


def _negs(n=1, modes=(0, 1), rel_range=3):
    from skge_amd import _lib as L
    m = list(modes) + [0] * (8 - len(modes))
    return L.SkgeNegatives(n, len(modes), (L.c_i * 8)(*m), rel_range)


def _call(entry, model=0, d=8, ent=None, rel=None, negs=None, gamma=6.0, alpha=1.0):
    from skge_amd import _lib as L
    lib = L.load()
    ent = _table(11, d, True) if ent is None else ent
    rel = _table(3, d, False) if rel is None else rel
    negs = _negs() if negs is None else negs
    e, r = ctypes.byref(ent), ctypes.byref(rel)
    if entry == "grad":
        rc = lib.skge_sadv_grad(FAKE, model, e, r, d, FAKE, FAKE, 5, negs, gamma, alpha, None, None,
                                None, None)
    elif entry == "step":
        rc = lib.skge_sadv_step(FAKE, model, e, r, d, FAKE, FAKE, 5, negs, gamma, alpha, None)
    else:
        h = lib.skge_sadv_runner_create(FAKE, model, e, r, d, FAKE, 37, FAKE, 128, 5, 7, FAKE,
                                        gamma, alpha, 100, None, None, negs)
        rc = 0 if h else -1
    return rc, lib.skge_last_error().decode()


@pytest.mark.parametrize("entry", ("grad", "step", "runner"))
def test_entry_points_refuse_by_name(entry):
    from skge_amd import _lib as L
    # the positive control ends at the backstop: everything else was accepted
    rc, msg = _call(entry)
    assert rc == -1 and "touched slots" in msg, msg
    cases = [(dict(model=L.SKGE_HOLE), "TransE-L1, TransE-L2 and RotatE"),
             (dict(model=L.SKGE_COMPLEX), "TransE-L1, TransE-L2 and RotatE"),
             (dict(model=4), "TransE-L1, TransE-L2 and RotatE"),
             (dict(model=L.SKGE_ROTATE, d=7), "RotatE needs an even d"),
             (dict(d=1025), "d=1025 unsupported"),
             (dict(alpha=-0.5), "alpha"), (dict(alpha=float("nan")), "finite"),
             (dict(gamma=float("inf")), "finite"),
             (dict(negs=_negs(33, (0, 1))), "at most 64"),
             (dict(negs=_negs(1, (0, 3))), "mode 3"),
             (dict(negs=_negs(0, (0, 1))), "must be >= 1"),
             (dict(negs=_negs(1, (0, 2), rel_range=9)), "rel_range"),
             (dict(ent=_table(11, 8, True, mode=L.SKGE_ACC_I16X4)), "fp32 (or fixed-point)"),
             (dict(ent=_table(11, 8, False, replicas=4)), "single accumulator copy"),
             (dict(rel=_table(3, 8, False, mode=L.SKGE_ACC_I16X4, post=L.SKGE_POST_UNITMOD)),
              "accumulator"),
             (dict(d=7, ent=_table(11, 7, True), rel=_table(3, 7, False, post=L.SKGE_POST_UNITMOD)),
              "SKGE_POST_UNITMOD needs an even width")]
    for kw, text in cases:
        rc, msg = _call(entry, **kw)
        assert rc == -1 and text in msg and "touched slots" not in msg, (kw, msg)
    # the slot refusal names the count needed: (2 + K) * P, K = 2, P = 5 (runner: batch 7)
    rc, msg = _call(entry)
    assert ("28 touched slots" if entry == "runner" else "20 touched slots") in msg, msg


def _standin(cls, **attrs):
    m = object.__new__(cls)
    m.params, m.hyperparams = {}, {}
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def test_trainer_refusals_name_the_model_and_the_trainer():
    import skge_amd as S
    from skge_amd.sample import RandomModeSampler
    xs = [(0, 1, 0), (1, 2, 1), (2, 3, 0)]
    smp = RandomModeSampler(2, [0, 1], xs, (5, 5, 2))
    for cls in (S.HolE, S.RESCAL, S.DistMult, S.ComplEx):
        with pytest.raises(ValueError) as e:
            S.SelfAdversarialTrainer(_standin(cls), samplef=smp.sample)
        assert cls.__name__ in str(e.value) and "StochasticTrainer" in str(e.value)
    te = _standin(S.TransE, l1=True)
    with pytest.raises(ValueError, match="samplef is None"):
        S.SelfAdversarialTrainer(te)
    with pytest.raises(ValueError, match="K = 66"):
        S.SelfAdversarialTrainer(te, samplef=RandomModeSampler(33, [0, 1], xs, (5, 5, 2)).sample)
    with pytest.raises(ValueError, match="1 to 8 modes"):
        S.SelfAdversarialTrainer(te, samplef=RandomModeSampler(1, [0, 1] * 5, xs, (5, 5, 2)).sample)
    with pytest.raises(ValueError, match="device_runner 'pairs'"):
        S.SelfAdversarialTrainer(te, samplef=smp.sample, device_runner="pairs")
    with pytest.raises(ValueError, match="alpha"):
        S.SelfAdversarialTrainer(te, samplef=smp.sample, alpha=-1.0)
    t = S.SelfAdversarialTrainer(_standin(S.RotatE), samplef=smp.sample, gamma=9.0, alpha=0.5)
    assert (t.model.gamma, t.model.alpha) == (9.0, 0.5)
    assert t.model.hyperparams["gamma"] == 9.0 and t.device_negatives is True
    with pytest.raises(ValueError, match="labelled negatives"):
        t.fit(xs, [1, -1, 1])
    # slots: first free slot of the corrupted position's mode, in slot order
    t._n, t._modes = 2, [1, 0]
    t.samplef = lambda xy: [((9, 1, 0), -1.0), ((0, 8, 0), -1.0), ((7, 1, 0), -1.0)]
    assert t._slots(((0, 1, 0), 1.0)) == [8, 9, -1, 7]
