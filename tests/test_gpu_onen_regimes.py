"""The 1-N batch core (csrc/skge_kvsall.hip) in the plan regimes the edge
shapes never reach: kvsall_ref.REGIME_SHAPES, each of which
tests/test_kvsall_ref.py holds against the restated plan -- DQ slices of
several chunks with a ragged last one, one slice forced by the 16 MB cap, a
score row split between k_ova_combine workgroups, more than 256 column tiles
and loss partials, B = 4096, d = 1024 and odd d.  Both regimes against their
fp64 restatements at the project's bar (parity_util: ATOL = RTOL = 1e-5), and
KvsAll bit for bit where a zero relation table makes every sum exact."""
import numpy as np
import pytest
import torch

import kvsall_ref as KR
import onevsall_ref as OR
import parity_util as PU
import test_gpu_kvsall as TK
import test_gpu_onevsall as TO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR = 0.1
M = KR.EDGE_M
CASES = [(model, s[:3]) for s in KR.REGIME_SHAPES for model in s[3]]
CASE_IDS = ["%s-%s" % (model, KR.regime_id(s)) for model, s in CASES]


def check(got, want, what):
    """parity_util.check, and nothing but finite values: its headroom takes a
    NaN's error for none, and an output no workgroup wrote is NaN here."""
    assert np.isfinite(PU._np(got)).all(), what + ": not finite"
    return PU.check(got, want, what)


def cases(keep):
    picked = [(c, i) for c, i in zip(CASES, CASE_IDS) if keep(*c[1])]
    return pytest.mark.parametrize("model,shape", [c for c, _ in picked],
                                   ids=[i for _, i in picked])


@cases(lambda N, B, d: True)
def test_kvsall_scores_exact_on_integer_tables(model, shape):
    """Tables of integers in [-3, 3]: a score's partial sums are integers of
    at most 1024 terms of at most 54, below 2^24, so every summation order is
    exact and the scores equal the integer reference bit for bit."""
    N, B, d = shape
    E, R, batch = KR.build_case(model, N, M, B, d, seed=N + B + d, integer=True)
    want = KR.query_vectors(model, E, R, *batch[:3]) @ E.T
    assert np.abs(want).max() < 2 ** 24
    z = TK.run_grad(model, E, R, batch, 0.0, scores=True)[4]
    assert z.shape == (B, N)
    assert np.array_equal(z.astype(np.float64), want)


_INT = {}
STABLE = [(32801, 2, 2), (8300, 130, 130)]


def ova_integer_case(model, shape):
    """1vsAll on the integer tables of a shape: (z, lse, loss) in fp64 and the
    device's outputs; kept for the shapes the stability test reads again."""
    key = (model, shape)
    if key in _INT:
        return _INT[key]
    N, B, d = shape
    E, R, batch = OR.build_case(model, N, M, B, d, seed=N + B + d, integer=True)
    fw = OR.forward(model, E, R, *batch, 0.0, 0.0)
    out = ((fw["z"], fw["lse"], fw["loss"]), TO.run_grad(model, E, R, batch, 0.0, 0.0, scores=True))
    if shape in STABLE:
        _INT[key] = out
    return out


@cases(lambda N, B, d: True)
def test_onevsall_scores_exact_on_integer_tables(model, shape):
    """As for KvsAll; the raw scores leave through the OVA epilogue."""
    N, B, d = shape
    (want, _, _), got = ova_integer_case(model, shape)
    assert np.abs(want).max() < 2 ** 24
    z = got[5]
    assert z.shape == (B, N)
    assert np.array_equal(z.astype(np.float64), want)


@cases(lambda N, B, d: (N, B, d) in STABLE)
def test_onevsall_stable_across_tiles_and_splits(model, shape):
    """The integer tables where a row's softmax partials come from 257 column
    tiles and 33 combine workgroups (d = 2: small scores, hundreds of ties at
    the row's maximum) or from 65 tiles and 8 workgroups (d = 130: scores in
    the hundreds, far past where exp overflows in fp32).  lse and the loss hold
    the bar; the gradients are finite."""
    N, B, d = shape
    (z, lse, loss), (gE, gR, _, got_loss, got_lse, _) = ova_integer_case(model, shape)
    if d == 130:
        assert np.abs(z).max() > 100
    else:
        # 49 distinct entity rows: each score value about N / 49 times
        assert ((z == z.max(axis=1, keepdims=True)).sum(axis=1) > 500).all()
    what = "regime onevsall stable %s N%d B%d d%d" % (model, N, B, d)
    check(got_lse, lse, what + " lse")
    check(np.array([got_loss]), np.array([loss]), what + " loss")
    assert np.isfinite(gE).all() and np.isfinite(gR).all()


@pytest.mark.parametrize("n3", [0.0, 0.05])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@cases(lambda N, B, d: True)
def test_onevsall_gradients(model, shape, eps, n3):
    """A softmax row sums to one and its entries are about 1 / N, so the
    gradient sums stay at the tables' own scale at every N here."""
    N, B, d = shape
    E, R, batch = OR.build_case(model, N, M, B, d, seed=2 * N + B + d)
    anchor, rel, dirn, target = batch
    seams = KR.split_ids(N, M, B, d)
    assert set(seams[:min(len(seams), B)]) <= set(target.tolist())
    assert anchor[0] == target[0] and (B == 1 or anchor[0] == anchor[1])
    fw, gE, gR, touched = OR.gradients(model, E, R, *batch, eps, n3)
    got_gE, got_gR, got_t, got_loss, got_lse = TO.run_grad(model, E, R, batch, eps, n3)
    what = "regime onevsall grad %s N%d B%d d%d eps%g n3%g" % (model, N, B, d, eps, n3)
    check(got_gE, gE, what + " gE")
    check(got_gR, gR, what + " gR")
    check(np.array([got_loss]), np.array([fw["loss"]]), what + " loss")
    check(got_lse, fw["lse"], what + " lse")
    assert np.array_equal(got_t != 0, touched) and set(got_t.tolist()) <= {0, 1}
    assert (~touched).any() and np.all(got_gR[~touched] == 0)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@cases(lambda N, B, d: N <= 1100)
def test_kvsall_gradients(model, shape, eps):
    """N <= 1100 only: KvsAll's loss is not normalised by N, so at N in the
    thousands a gradient element is a long random walk whose fp32 rounding has
    no measured bound against the bar; those regimes are pinned bit for bit by
    test_kvsall_exact_with_a_zero_relation_table."""
    N, B, d = shape
    E, R, batch = KR.build_case(model, N, M, B, d, seed=2 * N + B + d)
    anchor, rel, dirn, off, ans = batch
    seams = KR.split_ids(N, M, B, d)
    assert set(seams) <= set(ans[off[min(1, B - 1)]:off[min(1, B - 1) + 1]].tolist())
    fw, gE, gR, touched = KR.gradients(model, E, R, *batch, eps)
    got_gE, got_gR, got_t, got_loss = TK.run_grad(model, E, R, batch, eps)
    what = "regime kvsall grad %s N%d B%d d%d eps%g" % (model, N, B, d, eps)
    check(got_gE, gE, what + " gE")
    check(got_gR, gR, what + " gR")
    check(np.array([got_loss]), np.array([fw["loss"]]), what + " loss")
    assert np.array_equal(got_t != 0, touched) and set(got_t.tolist()) <= {0, 1}
    assert (~touched).any() and np.all(got_gR[~touched] == 0)


EXACT = [(model, s[:3]) for s in KR.REGIME_SHAPES + KR.EXACT_EXTRA_SHAPES for model in s[3]
         if s[1] & (s[1] - 1) == 0]


@pytest.mark.parametrize("model,shape", EXACT,
                         ids=["%s-%s" % (model, KR.regime_id(s)) for model, s in EXACT])
def test_kvsall_exact_with_a_zero_relation_table(model, shape):
    """Integer E, R = 0, no smoothing, B a power of two: Q = 0 and z = 0, so
    sigmoid = 1/2 and G = +-1 / (2 B), exactly.  Every partial sum of dq = G E
    is a multiple u = 1 / (2 B) below 2^24 u (3 N < 2^24), and so is every
    partial sum of the chain rule's products into a row of gR (checked below on
    the sums of magnitudes), so the results are exact in any summation, slice
    and atomic order: gR is the fp64 reference's bits, gE is zero (dq o R and
    G^T Q are), the marks match and the loss is N log 2."""
    N, B, d = shape
    E, R, batch = KR.build_case(model, N, M, B, d, seed=3 * N + B + d, integer=True)
    anchor, rel = batch[0], batch[1]
    R = np.zeros_like(R)
    fw, gE, gR, touched = KR.gradients(model, E, R, *batch, 0.0)
    assert np.all(fw["z"] == 0) and np.all(gE == 0) and np.any(gR != 0)
    u = 1.0 / (2 * B)
    assert 3 * N < 2 ** 24 and np.all(fw["dq"] / u == np.round(fw["dq"] / u))
    # a component of gR[p] sums, per query, at most two products of a dq
    # component and an entity component (|E| <= 3)
    mag = np.zeros(M)
    np.add.at(mag, rel, 2 * 3 * np.abs(fw["dq"]).max(axis=1) / u)
    assert mag.max() < 2 ** 24
    assert np.array_equal(gR.astype(np.float32).astype(np.float64), gR)
    got_gE, got_gR, got_t, got_loss = TK.run_grad(model, E, R, batch, 0.0)
    assert np.array_equal(got_gR, gR.astype(np.float32))
    assert np.all(got_gE == 0)
    assert np.array_equal(got_t != 0, touched) and set(got_t.tolist()) <= {0, 1}
    assert abs(fw["loss"] - N * np.log(2.0)) <= 1e-9 * N
    check(np.array([got_loss]), np.array([N * np.log(2.0)]),
             "regime kvsall exact %s N%d B%d d%d loss" % (model, N, B, d))


@pytest.mark.parametrize("model", KR.MODELS)
def test_kvsall_invalid_queries(model):
    """An anchor of N, a relation of M and a direction of 2 score as the zero
    vector: they reach no table row, add N log 2 / B each to the loss and still
    count in 1 / B.  Answer ids of -1 and N inside a valid query's list are no
    answers."""
    N, B, d = 129, 33, 50
    E, R, (a, p, t, off, ans) = KR.build_case(model, N, M, B, d, seed=77)
    a2, p2, t2 = a.copy(), p.copy(), t.copy()
    a2[5], p2[9], t2[12] = N, M, 2
    bad = np.array([5, 9, 12])
    keep = np.setdiff1d(np.arange(B), bad)
    at = off[7] + 1   # inside query 7's list, between two of its answers
    assert off[8] - off[7] >= 2
    ans2 = np.concatenate([ans[:at], [-1, N], ans[at:]]).astype(np.int32)
    off2 = off.copy()
    off2[8:] += 2
    # the reference with and without the invalid queries, on the CPU first
    lists = [ans[off[b]:off[b + 1]] for b in keep]
    offk = np.cumsum([0] + [len(x) for x in lists])
    fk, gEk, gRk, tk = KR.gradients(model, E, R, a[keep], p[keep], t[keep], offk,
                                    np.concatenate(lists), 0.1)
    scale = len(keep) / float(B)
    fw, gE, gR, touched = KR.gradients(model, E, R, a2, p2, t2, off2, ans2, 0.1)
    assert np.allclose(gE, gEk * scale, rtol=1e-12, atol=1e-15)
    assert np.allclose(gR, gRk * scale, rtol=1e-12, atol=1e-15) and np.array_equal(touched, tk)
    want_loss = fk["loss"] * scale + len(bad) * N * np.log(2.0) / B
    assert np.isclose(fw["loss"], want_loss, rtol=1e-12)
    got_gE, got_gR, got_t, got_loss, z = TK.run_grad(model, E, R, (a2, p2, t2, off2, ans2), 0.1,
                                                     scores=True)
    what = "regime kvsall invalid %s" % model
    check(got_gE, gEk * scale, what + " gE")
    check(got_gR, gRk * scale, what + " gR")
    check(np.array([got_loss]), np.array([want_loss]), what + " loss")
    assert np.all(z[bad] == 0)
    check(z[keep], fk["z"], what + " z")
    assert np.array_equal(got_t != 0, tk) and np.all(got_gR[~tk] == 0)


def one_step(regime, model, shape, opt, rparam):
    """One _step batch from seeded tables (and AdaGrad state) at a shape, the
    check of test_three_steps: the update reads gE, gR and the marks from the
    plan's own offsets."""
    import skge_amd as S
    N, B, d = shape
    ref = KR if regime == "kvsall" else OR
    E, R, _ = ref.build_case(model, N, M, B, d, seed=11)
    m = TK.make_model(model, N, M, d, E, R, rparam)
    m.add_hyperparam("label_smoothing", 0.1)
    if regime == "onevsall":
        m.add_hyperparam("n3", 0.05)
    if opt == "sgd":
        upd = {pid: S.SGD(p, LR) for pid, p in m.params.items()}
    else:
        upd = {pid: S.AdaGrad(p, LR) for pid, p in m.params.items()}
        rng = np.random.RandomState(5)
        for pid in ("E", "R"):
            upd[pid].p2.copy_(TK.dev_f32(rng.uniform(0.01, 1.0, size=tuple(m.params[pid].shape))))
    _, _, batch = ref.build_case(model, N, M, B, d, seed=20)
    params = {pid: TK.f64(m.params[pid].data) for pid in ("E", "R")}
    state = {pid: TK.f64(upd[pid].p2) if opt == "adagrad" else None for pid in ("E", "R")}
    bits = m.R.data.cpu().numpy().copy()
    sbits = upd["R"].p2.cpu().numpy().copy() if opt == "adagrad" else None
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    if regime == "kvsall":
        from skge_amd.kvsall import KvsAllQueries
        m._kvsall_step(KvsAllQueries(*batch, N, M), upd, loss)
        fw, new, nstate, grads, pre = KR.step(model, params, state, batch, 0.1, LR, opt, rparam)
    else:
        from skge_amd.onevsall import OneVsAllQueries
        m._onevsall_step(OneVsAllQueries(*batch, N, M), upd, loss)
        fw, new, nstate, grads, pre = OR.step(model, params, state, batch, 0.1, 0.05, LR, opt,
                                              rparam)
    what = "regime %s step %s %s N%d B%d d%d" % (regime, model, opt, N, B, d)
    check(TK.f64(loss), np.array([fw["loss"]]), what + " loss")
    assert all(np.isfinite(TK.f64(m.params[pid].data)).all() for pid in ("E", "R")), what
    PU.check_step(TK.f64(m.E.data), new["E"], params["E"], grads["E"], nstate["E"], LR,
                  what + " E", post="normless1", opt=opt)
    PU.check_step(TK.f64(m.R.data), new["R"], params["R"], grads["R"], nstate["R"], LR,
                  what + " R", post=None, opt=opt)
    if opt == "adagrad":
        for pid in ("E", "R"):
            check(TK.f64(upd[pid].p2), nstate[pid], what + " p2 " + pid)
    idle = np.setdiff1d(np.arange(M), grads["R"][1])
    assert len(idle) > 0
    assert np.array_equal(m.R.data.cpu().numpy()[idle], bits[idle])
    if opt == "adagrad":
        assert np.array_equal(upd["R"].p2.cpu().numpy()[idle], sbits[idle])


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("shape", [(300, 2048, 512), (2501, 600, 2)], ids=KR.regime_id)
@pytest.mark.parametrize("model", KR.MODELS)
@pytest.mark.parametrize("regime", ["kvsall", "onevsall"])
def test_one_step(regime, model, shape, opt):
    """ns = 4, ntd = 4 and 16 row tiles, or a row split in two above 1024
    columns: the gradient buffers lie past partials and row partials of more
    than one slice and tile."""
    one_step(regime, model, shape, opt, 0.01)
