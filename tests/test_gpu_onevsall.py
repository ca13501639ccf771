"""1vsAll training of DistMult and ComplEx on the device (csrc/skge_kvsall.hip:
k_kv_gemm<OVA>, k_ova_combine, k_ova_chain) against the fp64 restatement of
tests/onevsall_ref.py: exact scores on integer tables at the tile edges, the
softmax's stability on scores in the hundreds and thousands, gradients,
invalid queries, three consecutive steps, the trainer and the refusals.
Tolerances are the project's bar (parity_util: ATOL = RTOL = 1e-5); every
check's headroom goes to parity_util.RECORDS."""
import os
import tempfile

import numpy as np
import pytest
import torch

import kvsall_ref as KR
import onevsall_ref as OR
import parity_util as PU

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR = 0.1
CODES = {"distmult": 5, "complex": 6}
SHAPE_IDS = ["N%d-B%d-d%d" % s for s in KR.EDGE_SHAPES]
M = KR.EDGE_M


def dev_i32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=DEV)


def dev_f32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def run_grad(model, E, R, batch, eps, n3, scores=False):
    """skge_onevsall_grad through ctypes: gE, gR, touched, loss, lse (and z)."""
    from skge_amd import _lib as L
    lib = L.lib()
    (N, d), nrel, B = E.shape, R.shape[0], len(batch[0])
    nbytes = lib.skge_onevsall_workspace_bytes(CODES[model], B, N, nrel, d)
    assert nbytes > 0
    # NaN-filled scratch: nothing may be read before it is written
    ws = torch.full((nbytes // 4 + 1,), float("nan"), dtype=torch.float32, device=DEV)
    tE, tR = dev_f32(E), dev_f32(R)
    q = [dev_i32(x) for x in batch]
    gE = torch.full((N, d), float("nan"), dtype=torch.float32, device=DEV)
    gR = torch.full((nrel, d), float("nan"), dtype=torch.float32, device=DEV)
    touched = torch.full((nrel,), -7, dtype=torch.int32, device=DEV)
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    lse = torch.full((B,), float("nan"), dtype=torch.float32, device=DEV)
    z = torch.full((B, N), float("nan"), dtype=torch.float32, device=DEV) if scores else None
    L.check(lib.skge_onevsall_grad(L.stream_ptr(), CODES[model], L.ptr(tE), L.ptr(tR), N, nrel, d,
                                   L.ptr(q[0]), L.ptr(q[1]), L.ptr(q[2]), L.ptr(q[3]), B, eps, n3,
                                   L.ptr(gE), L.ptr(gR), L.ptr(touched), L.ptr(loss), L.ptr(z),
                                   L.ptr(lse), L.ptr(ws), nbytes), "onevsall_grad")
    out = [gE.cpu().numpy(), gR.cpu().numpy(), touched.cpu().numpy(), float(loss.item()),
           lse.cpu().numpy()]
    return out + [z.cpu().numpy()] if scores else out


_INT = {}


def integer_case(model, shape):
    """The integer-table case of a shape and its device outputs, computed once
    and shared by the exactness and the stability tests."""
    key = (model, shape)
    if key not in _INT:
        N, B, d = shape
        E, R, batch = OR.build_case(model, N, M, B, d, seed=N + B + d, integer=True)
        fw, gE, gR, touched = OR.gradients(model, E, R, *batch, 0.0, 0.0)
        _INT[key] = (fw, run_grad(model, E, R, batch, 0.0, 0.0, scores=True))
    return _INT[key]


@pytest.mark.parametrize("shape", KR.EDGE_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("model", OR.MODELS)
def test_scores_exact_on_integer_tables(model, shape):
    """Tables of integers in [-3, 3]: every partial sum of a score is an integer
    below 2^24 (at most 200 terms of at most 18 * 3), so any summation order is
    exact and the scores equal the integer reference bit for bit."""
    N, B, d = shape
    fw, got = integer_case(model, shape)
    assert np.abs(fw["z"]).max() < 2 ** 24
    z = got[5]
    assert z.shape == (B, N)
    assert np.array_equal(z.astype(np.float64), fw["z"])


@pytest.mark.parametrize("shape", [s for s in KR.EDGE_SHAPES if s[2] == 200],
                         ids=[i for i, s in zip(SHAPE_IDS, KR.EDGE_SHAPES) if s[2] == 200])
@pytest.mark.parametrize("model", OR.MODELS)
def test_stable_on_large_scores(model, shape):
    """The integer tables at d = 200: scores far past where exp overflows in
    fp32 (88.7).  lse and the loss hold the bar; the gradients are finite."""
    N, B, d = shape
    fw, (gE, gR, _, loss, lse, z) = integer_case(model, shape)
    assert np.abs(fw["z"]).max() > 100
    what = "onevsall stable %s N%d B%d d%d" % (model, N, B, d)
    PU.check(lse, fw["lse"], what + " lse")
    PU.check(np.array([loss]), np.array([fw["loss"]]), what + " loss")
    assert np.isfinite(gE).all() and np.isfinite(gR).all()


@pytest.mark.parametrize("n3", [0.0, 0.05])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("shape", KR.EDGE_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("model", OR.MODELS)
def test_gradients(model, shape, eps, n3):
    N, B, d = shape
    E, R, batch = OR.build_case(model, N, M, B, d, seed=2 * N + B + d)
    anchor, rel, dirn, target = batch
    if (N, B) == (300, 33):   # the case that must hold every special record
        assert anchor[0] == anchor[1] and target[0] == anchor[0]
        assert all(x[2] == x[3] for x in batch)
        assert target[4:8].tolist() == [0, 299, 127, 128]
        assert set(dirn.tolist()) == {0, 1}
    fw, gE, gR, touched = OR.gradients(model, E, R, *batch, eps, n3)
    got_gE, got_gR, got_t, got_loss, got_lse = run_grad(model, E, R, batch, eps, n3)
    what = "onevsall %s N%d B%d d%d eps%g n3%g" % (model, N, B, d, eps, n3)
    PU.check(got_gE, gE, what + " gE")
    PU.check(got_gR, gR, what + " gR")
    PU.check(np.array([got_loss]), np.array([fw["loss"]]), what + " loss")
    PU.check(got_lse, fw["lse"], what + " lse")
    assert np.array_equal(got_t != 0, touched) and set(got_t.tolist()) <= {0, 1}
    assert (~touched).any() and np.all(got_gR[~touched] == 0)
    if N == 1 and eps == 0.0 and n3 == 0.0:   # one candidate: lse = z, softmax - y = 0
        assert np.all(got_gE == 0) and np.all(got_gR == 0)


@pytest.mark.parametrize("model", OR.MODELS)
def test_invalid_queries(model):
    """A target of -1, a target of N and an anchor of N: everything else equals
    the reference with those queries dropped and B unchanged."""
    N, B, d = 129, 33, 50
    E, R, (a, p, t, g) = OR.build_case(model, N, M, B, d, seed=77)
    a, g = a.copy(), g.copy()
    g[5], g[9], a[12] = -1, N, N
    bad = np.array([5, 9, 12])
    keep = np.setdiff1d(np.arange(B), bad)
    fk, gEk, gRk, tk = OR.gradients(model, E, R, a[keep], p[keep], t[keep], g[keep], 0.1, 0.05)
    scale = len(keep) / float(B)   # the dropped queries still count in 1 / B
    fw, gE, gR, touched = OR.gradients(model, E, R, a, p, t, g, 0.1, 0.05)
    assert np.allclose(gE, gEk * scale, rtol=1e-12, atol=1e-15) and np.array_equal(touched, tk)
    got_gE, got_gR, got_t, got_loss, got_lse = run_grad(model, E, R, (a, p, t, g), 0.1, 0.05)
    what = "onevsall invalid %s" % model
    PU.check(got_gE, gEk * scale, what + " gE")
    PU.check(got_gR, gRk * scale, what + " gR")
    PU.check(np.array([got_loss]), np.array([fk["loss"] * scale]), what + " loss")
    PU.check(got_lse[keep], fk["lse"], what + " lse")
    assert np.isfinite(got_lse).all()
    assert np.array_equal(got_t != 0, tk) and np.all(got_gR[~tk] == 0)


def make_model(model, N, nrel, d, E, R, rparam):
    import skge_amd as S
    np.random.seed(1)
    cls = S.DistMult if model == "distmult" else S.ComplEx
    m = cls((N, N, nrel), d, rparam=rparam)
    m.E.data.copy_(dev_f32(E))
    m.R.data.copy_(dev_f32(R))
    return m


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("rparam", [0.0, 0.01])
@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("model", OR.MODELS)
def test_three_steps(model, opt, rparam):
    """Three consecutive skge_onevsall_step batches, each checked from the
    device state before it; the relation rows no query names keep their bits."""
    import skge_amd as S
    from skge_amd.onevsall import OneVsAllQueries
    N, B, d = 129, 33, 50
    E, R, _ = OR.build_case(model, N, M, B, d, seed=11)
    m = make_model(model, N, M, d, E, R, rparam)
    m.add_hyperparam("label_smoothing", 0.1)
    m.add_hyperparam("n3", 0.05)
    if opt == "sgd":
        upd = {pid: S.SGD(p, LR) for pid, p in m.params.items()}
    else:
        upd = {pid: S.AdaGrad(p, LR) for pid, p in m.params.items()}
        rng = np.random.RandomState(5)
        for pid in ("E", "R"):
            upd[pid].p2.copy_(dev_f32(rng.uniform(0.01, 1.0, size=tuple(m.params[pid].shape))))
    for k in range(3):
        _, _, batch = OR.build_case(model, N, M, B, d, seed=20 + k)
        q = OneVsAllQueries(*batch, N, M)
        params = {pid: f64(m.params[pid].data) for pid in ("E", "R")}
        state = {pid: f64(upd[pid].p2) if opt == "adagrad" else None for pid in ("E", "R")}
        bits = {pid: m.params[pid].data.cpu().numpy().copy() for pid in ("E", "R")}
        sbits = upd["R"].p2.cpu().numpy().copy() if opt == "adagrad" else None
        loss = torch.zeros(1, dtype=torch.float32, device=DEV)
        m._onevsall_step(q, upd, loss)
        fw, new, nstate, grads, pre = OR.step(model, params, state, batch, 0.1, 0.05, LR, opt,
                                              rparam)
        what = "onevsall step %s %s r%g b%d" % (model, opt, rparam, k)
        PU.check(f64(loss), np.array([fw["loss"]]), what + " loss")
        PU.check_step(f64(m.E.data), new["E"], params["E"], grads["E"], nstate["E"], LR,
                      what + " E", post="normless1", opt=opt)
        PU.check_step(f64(m.R.data), new["R"], params["R"], grads["R"], nstate["R"], LR,
                      what + " R", post=None, opt=opt)
        if opt == "adagrad":
            for pid in ("E", "R"):
                PU.check(f64(upd[pid].p2), nstate[pid], what + " p2 " + pid)
        idle = np.setdiff1d(np.arange(M), grads["R"][1])
        assert len(idle) > 0
        assert np.array_equal(m.R.data.cpu().numpy()[idle], bits["R"][idle])
        if opt == "adagrad":
            assert np.array_equal(upd["R"].p2.cpu().numpy()[idle], sbits[idle])


def small_kg():
    """~60 entities, 4 relations, ~300 distinct triples (s, o, p)."""
    rng = np.random.RandomState(4)
    x = np.stack([rng.randint(0, 60, 330), rng.randint(0, 60, 330), rng.randint(0, 4, 330)], axis=1)
    return [tuple(int(v) for v in r) for r in np.unique(x, axis=0)], (60, 60, 4)


def mean_filtered_rank(m, xs):
    import skge_amd as S
    ev = S.FilteredRankingEval(xs, xs)
    _, fpos = ev.positions(m)
    return S.ranking_scores(fpos, fpos)[1][1]


@pytest.mark.parametrize("model", OR.MODELS)
def test_trainer(model):
    import skge_amd as S
    xs, sz = small_kg()
    assert 250 <= len(xs) <= 330
    cls = S.DistMult if model == "distmult" else S.ComplEx

    def fit(fused, epochs):
        np.random.seed(3)
        m = cls(sz, 16, rparam=0.001)
        rank0 = mean_filtered_rank(m, xs)
        seen = []

        def record(tr):
            seen.append((f64(tr.model.E.data), f64(tr.model.R.data), float(tr.loss)))
            return True

        # (KvsAllTrainer's learning rate, for its reason: the two routes add the
        # chain rule's float atomics in different orders and AdaGrad carries the
        # difference through 90 steps, so the step is kept small)
        tr = S.OneVsAllTrainer(m, nbatches=3, max_epochs=epochs, learning_rate=0.05,
                               label_smoothing=0.1, n3=0.05, post_epoch=[record], fused=fused)
        np.random.seed(9)
        tr.fit(xs)
        return m, tr, seen, rank0

    m, tr, fused, rank0 = fit(True, 30)
    _, _, steps, _ = fit(False, 30)
    assert len(fused) == len(steps) == 30
    for ep, (a, b) in enumerate(zip(fused, steps)):
        PU.check(a[0], b[0], "onevsall trainer %s E epoch %d" % (model, ep + 1))
        PU.check(a[1], b[1], "onevsall trainer %s R epoch %d" % (model, ep + 1))
        PU.check(np.array([a[2]]), np.array([b[2]]), "onevsall trainer %s loss epoch %d"
                 % (model, ep + 1))
    assert fused[-1][2] < fused[0][2], (fused[0][2], fused[-1][2])
    assert mean_filtered_rank(m, xs) < rank0
    assert len(tr.queries) == 2 * len(xs) and tr.queries.device is not None
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "m.pkl")
        m.save(path)
        back = S.Model.load(path)
    assert type(back) is cls and back.label_smoothing == 0.1 and back.n3 == 0.05
    for pid in ("E", "R"):
        assert np.array_equal(np.asarray(back.params[pid]), np.asarray(m.params[pid]))


def test_refusals():
    import skge_amd as S
    from skge_amd import _lib as L
    sz = (20, 20, 3)
    np.random.seed(2)
    others = [S.HolE(sz, 8), S.RESCAL(sz, 8), S.TransE(sz, 8), S.RotatE(sz, 8)]
    for m in others:
        name = type(m).__name__
        with pytest.raises(ValueError, match=name) as e:
            S.OneVsAllTrainer(m)
        assert "DistMult" in str(e.value) and "ComplEx" in str(e.value)
    m = S.DistMult(sz, 8)
    xs = [(i % 20, (3 * i + 1) % 20, i % 3) for i in range(40)]
    with pytest.raises(ValueError, match="samplef"):
        S.OneVsAllTrainer(m, samplef=S.RandomModeSampler(1, [0, 1], xs, sz).sample)
    with pytest.raises(ValueError, match="device_loop"):
        S.OneVsAllTrainer(m, device_loop=True)
    with pytest.raises(ValueError, match="device_runner"):
        S.OneVsAllTrainer(m, device_runner="pairs")
    with pytest.raises(ValueError, match="n3"):
        S.OneVsAllTrainer(m, n3=-1.0)
    S.set_deterministic(True)
    try:
        with pytest.raises(ValueError, match="deterministic"):
            S.OneVsAllTrainer(m)
    finally:
        S.set_deterministic(False)
    with pytest.raises(ValueError, match="y != 1"):
        S.OneVsAllTrainer(m, nbatches=2).fit(xs, [1] * 39 + [-1])
    # more than 4096 queries in a batch: the error names nbatches
    big = S.DistMult((5000, 5000, 1), 2, init="device_nunif")
    many = [(i, (i + 1) % 5000, 0) for i in range(5000)]
    with pytest.raises(ValueError, match="nbatches") as e:
        S.OneVsAllTrainer(big, nbatches=2, max_epochs=1).fit(many)
    assert "4096" in str(e.value)
    # the C entry points, with live tables: 0..3 and 7 not supported, 4 unknown
    lib = L.lib()
    E, R = m.E.data, m.R.data
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    f = torch.zeros(20 * 8, dtype=torch.float32, device=DEV)

    def grad(code, n3=0.0, d=8, B=2, ws=640):
        return lib.skge_onevsall_grad(L.stream_ptr(), code, L.ptr(E), L.ptr(R), 20, 3, d, L.ptr(z),
                                      L.ptr(z), L.ptr(z), L.ptr(z), B, 0.0, n3, L.ptr(f), L.ptr(f),
                                      L.ptr(z), L.ptr(f), None, None, L.ptr(f), ws)

    for code, want in ((0, -3), (1, -3), (2, -3), (3, -3), (7, -3), (4, -1)):
        rc = grad(code)
        assert rc == want, (code, rc)
        assert str(code).encode() in lib.skge_last_error()
    assert grad(5, n3=-0.1) == -1 and b"N3" in lib.skge_last_error()
    assert grad(5, n3=float("nan")) == -1 and b"N3" in lib.skge_last_error()
    # the size limits, ComplEx's even d and a workspace one byte short
    assert grad(5, B=4097) == -3 and b"4097" in lib.skge_last_error()
    assert grad(5, d=1025) == -3 and b"1025" in lib.skge_last_error()
    assert grad(6, d=3) == -1 and b"even" in lib.skge_last_error()
    need = KR.plan("onevsall", 2, 20, 3, 8).total
    assert lib.skge_onevsall_workspace_bytes(5, 2, 20, 3, 8) == need
    assert grad(5, ws=need - 1) == -1 and str(need).encode() in lib.skge_last_error()
    torch.cuda.synchronize()
