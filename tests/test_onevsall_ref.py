"""CPU checks of 1vsAll: the fp64 restatement's gradients against central
differences of its own loss, the N3 gradient at a zero row, OneVsAllQueries on
a hand-written KG, the trainer's refusals, and the three entry points in the
header, the library and the ctypes table."""
import os
import re

import numpy as np
import pytest

import kvsall_ref as KR
import onevsall_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("skge_onevsall_workspace_bytes", "skge_onevsall_grad", "skge_onevsall_step")


def fd_case(direction):
    """N = 6, M = 3, d = 4; queries 0 and 1 repeat an anchor, 1 and 2 share a
    relation, query 0's target is its own anchor, queries 3 and 4 are equal."""
    rng = np.random.RandomState(7)
    E = rng.uniform(-1, 1, size=(6, 4))
    R = rng.uniform(-1, 1, size=(3, 4))
    anchor = np.array([2, 2, 4, 5, 5])
    rel = np.array([0, 1, 1, 2, 2])
    dirn = {"tail": np.zeros(5, dtype=int), "head": np.ones(5, dtype=int),
            "mixed": np.array([0, 1, 1, 0, 0])}[direction]
    target = np.array([2, 0, 5, 1, 1])
    return E, R, (anchor, rel, dirn, target)


@pytest.mark.parametrize("n3", [0.0, 0.05])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("direction", ["tail", "head", "mixed"])
@pytest.mark.parametrize("model", OR.MODELS)
def test_gradients_match_central_differences(model, direction, eps, n3):
    """h = 1e-5 in fp64; tolerance 1e-7 + 1e-5 |g|: truncation ~ h^2, round-off
    ~ 2^-52 |L| / h = 2e-9 for |L| <= 100.  (|x|^3 is twice differentiable, so
    the central difference holds its order with N3 too.)"""
    E, R, batch = fd_case(direction)
    fw, gE, gR, touched = OR.gradients(model, E, R, *batch, eps, n3)
    assert abs(fw["loss"]) <= 100
    assert (fw["l_n3"] > 0) == (n3 > 0) and abs(fw["loss"] - fw["l_ce"] - fw["l_n3"]) < 1e-15
    h = 1e-5
    for name, P, g in (("E", E, gE), ("R", R, gR)):
        num = np.zeros_like(P)
        for i in np.ndindex(*P.shape):
            keep = P[i]
            P[i] = keep + h
            up = OR.loss(model, E, R, *batch, eps, n3)
            P[i] = keep - h
            dn = OR.loss(model, E, R, *batch, eps, n3)
            P[i] = keep
            num[i] = (up - dn) / (2 * h)
        err = np.abs(num - g)
        assert np.all(err <= 1e-7 + 1e-5 * np.abs(g)), (name, float(err.max()))
    assert touched.tolist() == [True, True, True]
    assert np.any(gR != 0)


def test_loss_definition_term_by_term():
    """L_ce restated with an explicit softmax and logs; G rows sum to 0."""
    E, R, batch = fd_case("mixed")
    fw = OR.forward("complex", E, R, *batch, 0.1)
    p = np.exp(fw["z"]) / np.exp(fw["z"]).sum(axis=1, keepdims=True)
    want = -(fw["y"] * np.log(p)).sum() / 5
    assert abs(fw["l_ce"] - want) < 1e-12
    assert np.isclose(fw["y"][0, 2], 0.9 + 0.1 / 6) and np.isclose(fw["y"][0, 0], 0.1 / 6)
    assert np.allclose(fw["y"].sum(axis=1), 1.0) and np.abs(fw["G"].sum(axis=1)).max() < 1e-15
    assert np.allclose(fw["lse"], np.log(np.exp(fw["z"]).sum(axis=1)))


@pytest.mark.parametrize("model", OR.MODELS)
def test_n3_gradient_is_zero_not_nan_at_a_zero_row(model):
    E, R, batch = fd_case("mixed")
    E[2] = 0.0   # the anchor of queries 0 and 1 and the target of query 0
    R[2] = 0.0
    assert np.all(OR.n3_grad(model, E[2:3]) == 0) and np.all(OR.n3_norm(model, E[2:3]) == 0)
    fw, gE, gR, _ = OR.gradients(model, E, R, *batch, 0.0, 0.05)
    assert np.isfinite(gE).all() and np.isfinite(gR).all() and np.isfinite(fw["loss"])
    _, gE0, gR0, _ = OR.gradients(model, E, R, *batch, 0.0, 0.0)
    assert np.array_equal(gE[2], gE0[2]) and np.array_equal(gR[2], gR0[2])


def test_invalid_queries_contribute_nothing():
    E, R, (a, p, t, g) = OR.build_case("complex", 40, 7, 9, 6, seed=3)
    g2, a2 = g.copy(), a.copy()
    g2[1], g2[4], a2[6] = -1, 40, 40
    fw, gE, gR, touched = OR.gradients("complex", E, R, a2, p, t, g2, 0.1, 0.05)
    keep = np.array([0, 2, 3, 5, 7, 8])
    fk, gEk, gRk, tk = OR.gradients("complex", E, R, a[keep], p[keep], t[keep], g[keep], 0.1, 0.05)
    # the same queries, but 1 / B counts the dropped ones
    assert np.allclose(gE * 9, gEk * 6) and np.allclose(gR * 9, gRk * 6)
    assert np.isclose(fw["loss"] * 9, fk["loss"] * 6) and np.array_equal(touched, tk)
    assert not touched[1::2].any() and np.all(gR[~touched] == 0)
    assert np.all(fw["G"][[1, 4, 6]] == 0)


def test_build_case_holds_its_special_records():
    E, R, (a, p, t, g) = OR.build_case("distmult", 300, 7, 33, 8, seed=1)
    assert a[0] == a[1] and g[0] == a[0]
    assert (a[2], p[2], t[2], g[2]) == (a[3], p[3], t[3], g[3])
    assert g[4:8].tolist() == [0, 299, 127, 128]
    assert set(t.tolist()) == {0, 1} and np.all(p % 2 == 0)
    _, _, (_, _, _, g) = OR.build_case("distmult", 128, 7, 33, 8, seed=1)
    assert g[4:7].tolist() == [0, 127, 127]


def test_build_case_puts_targets_at_the_split_seams():
    """Where k_ova_combine splits a row: the first column of workgroup 1, the
    last of the last workgroup (in its element tail when N is no multiple of
    4), the last of workgroup 0 and column 0, as far as the queries reach; the
    records of the unsplit shapes stay."""
    for N, B, d in ((2501, 600, 2), (8300, 130, 130)):
        chunk = KR.plan("onevsall", B, N, 7, d).chunk
        _, _, (a, p, t, g) = OR.build_case("distmult", N, 7, B, d, seed=1)
        assert {chunk, N - 1, chunk - 1, 0} <= set(g.tolist())
        assert N % 4 == 0 or (N & ~3) in g.tolist()
        assert a[0] == a[1] and g[0] == a[0]
        assert (a[2], p[2], t[2], g[2]) == (a[3], p[3], t[3], g[3])
        assert g[4:8].tolist() == [0, N - 1, 127, 128]
    _, _, (a, p, t, g) = OR.build_case("distmult", 1025, 7, 3, 2, seed=1)
    assert g.tolist() == [515, 516, 1024] and a[0] == a[1] == 515
    _, _, (a, p, t, g) = OR.build_case("distmult", 32801, 7, 2, 2, seed=1)
    assert g.tolist() == [32800, 996] and a[0] == a[1] == 32800
    # the owner of every seam target: each workgroup of a split is some query's
    for N, B, d, want in ((1025, 3, 2, {0, 1}), (2501, 600, 2, {0, 1}),
                          (8300, 130, 130, set(range(8)))):
        chunk = KR.plan("onevsall", B, N, 7, d).chunk
        _, _, (_, _, _, g) = OR.build_case("complex", N, 7, B, d, seed=2)
        assert {int(x) // chunk for x in g} == want


def test_plan_equals_the_library_workspace():
    """kvsall_ref.plan restates kv_plan for this regime too: the same bytes at
    every shape of the suites, the benchmark's and both sides of the plan's
    thresholds."""
    from skge_amd import _lib as L
    lib = L.load()
    for B, N, nrel, d in KR.plan_grid():
        for code in (5, 6) if d % 2 == 0 else (5,):
            want = lib.skge_onevsall_workspace_bytes(code, B, N, nrel, d)
            assert want > 0 and KR.plan("onevsall", B, N, nrel, d).total == want, (B, N, nrel, d)


# (s, o, p): a duplicated triple, a self-loop (3, 3, 0), entity 4 only ever an object
KG = [(0, 1, 0), (0, 2, 0), (0, 1, 0), (3, 3, 0), (1, 4, 1), (2, 4, 1)]
SZ = (5, 5, 2)


def test_queries_order_and_counts():
    from skge_amd.onevsall import OneVsAllQueries
    q = OneVsAllQueries.from_triples(KG, SZ)
    assert len(q) == 12   # one per triple and direction: the duplicate stays
    got = list(zip(q.dir.tolist(), q.rel.tolist(), q.anchor.tolist(), q.target.tolist()))
    assert got == ([(0, p, s, o) for s, o, p in KG] + [(1, p, o, s) for s, o, p in KG])
    assert all(a.dtype == np.int32 for a in (q.anchor, q.rel, q.dir, q.target))
    tail = OneVsAllQueries.from_triples(KG, SZ, directions=("tail",))
    head = OneVsAllQueries.from_triples(KG, SZ, directions=("head",))
    assert len(tail) == len(head) == 6 and np.all(tail.dir == 0) and np.all(head.dir == 1)
    assert tail.target.tolist() == [o for _, o, _ in KG]
    rev = OneVsAllQueries.from_triples(KG, SZ, directions=("head", "tail"))
    assert rev.dir.tolist() == [1] * 6 + [0] * 6
    with pytest.raises(ValueError, match="sideways"):
        OneVsAllQueries.from_triples(KG, SZ, directions=("sideways",))
    with pytest.raises(ValueError, match="outside"):
        OneVsAllQueries.from_triples([(0, 5, 0)], SZ)


def test_queries_batch_round_trips():
    from skge_amd.onevsall import OneVsAllQueries
    q = OneVsAllQueries.from_triples(KG, SZ)
    whole = q.batch(np.arange(len(q)))
    for name in ("anchor", "rel", "dir", "target"):
        assert np.array_equal(getattr(whole, name), getattr(q, name)), name
    b = q.batch([11, 0, 2, 0])
    assert b.anchor.tolist() == [4, 0, 0, 0] and b.target.tolist() == [2, 1, 1, 1]
    assert b.dir.tolist() == [1, 0, 0, 0] and b.rel.tolist() == [1, 0, 0, 0]
    assert len(q.batch([])) == 0
    assert b.batch([0]).target.tolist() == [2] and b.device is None


def test_header_library_and_ctypes_name_the_entry_points():
    from skge_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "skge_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = L.load()
    for f in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % f, src), f
        assert hasattr(lib, f), f
        assert f in L.SIGNATURES, f
    assert len(L.SIGNATURES["skge_onevsall_grad"][1]) == 22
    assert len(L.SIGNATURES["skge_onevsall_step"][1]) == 15
    assert lib.skge_abi_version() == 2


def test_entry_points_refuse_without_a_gpu():
    """Model codes 0..3 and 7: SKGE_ENOTSUP, by name; 4: SKGE_EINVAL; the size
    limits, the smoothing and the N3 weight, each naming what was asked."""
    from skge_amd import _lib as L
    lib = L.load()
    grad = lambda model, N=10, M=2, d=4, B=3, eps=0.0, n3=0.0: lib.skge_onevsall_grad(
        None, model, None, None, N, M, d, None, None, None, None, B, eps, n3, None, None, None,
        None, None, None, None, 0)
    step = lambda model, d=4, B=3, n3=0.0: lib.skge_onevsall_step(
        None, model, None, None, d, None, None, None, None, B, 0.0, n3, None, None, 0)
    names = {0: b"TransE-L1", 1: b"TransE-L2", 2: b"HolE", 3: b"RESCAL", 7: b"RotatE"}
    for code, name in names.items():
        for call in (grad, step):
            assert call(code) == -3, code
            msg = lib.skge_last_error()
            assert name in msg and b"DistMult" in msg and b"ComplEx" in msg, msg
        assert lib.skge_onevsall_workspace_bytes(code, 3, 10, 2, 4) == 0
    for call in (grad, step):
        assert call(4) == -1 and b"unknown model 4" in lib.skge_last_error()
    assert grad(5, B=4097) == -3 and b"4097" in lib.skge_last_error()
    assert grad(5, d=1025) == -3 and b"1025" in lib.skge_last_error()
    assert grad(5, B=0) == -1 and grad(5, N=0) == -1 and grad(5, M=0) == -1
    assert grad(6, d=5) == -1 and b"even" in lib.skge_last_error()
    assert grad(5, eps=1.0) == -1 and b"smoothing" in lib.skge_last_error()
    for bad in (-0.5, float("inf"), float("nan")):
        for call in (grad, step):
            assert call(5, n3=bad) == -1 and b"N3" in lib.skge_last_error(), bad
    # a finite weight, however large, passes the N3 check (and fails the next one)
    assert grad(5, n3=3.2e38) == -1 and b"NULL" in lib.skge_last_error()
    assert grad(5) == -1 and b"NULL" in lib.skge_last_error()
    assert lib.skge_onevsall_workspace_bytes(5, 4097, 10, 2, 4) == 0
    # G is indexed in size_t: B N past 2^31 elements
    big = lib.skge_onevsall_workspace_bytes(5, 4096, 1 << 20, 2, 4)
    assert big > 4 * 4096 * (1 << 20)
    assert lib.skge_onevsall_workspace_bytes(6, 3, 10, 2, 4) > 0


def test_trainer_refusals_name_their_reason():
    """The trainer's refusals that need no device."""
    import skge_amd as S
    from skge_amd import onevsall

    class Fake(S.Model):   # a model object without device tables
        model_code = None

        def __init__(self, code):
            self.model_code = code
            self.params, self.hyperparams = {}, {}

    for cls_name, code in (("HolE", 2), ("RESCAL", 3), ("TransE", 0), ("RotatE", 7)):
        m = type(cls_name, (Fake,), {})(code)
        with pytest.raises(ValueError, match=cls_name) as e:
            S.OneVsAllTrainer(m)
        assert "DistMult" in str(e.value) and "ComplEx" in str(e.value)
    m = type("ComplEx", (Fake,), {})(6)
    with pytest.raises(ValueError, match="samplef"):
        S.OneVsAllTrainer(m, samplef=lambda x: x)
    with pytest.raises(ValueError, match="device_loop"):
        S.OneVsAllTrainer(m, device_loop=True)
    with pytest.raises(ValueError, match="device_runner"):
        S.OneVsAllTrainer(m, device_runner="pipe")
    with pytest.raises(ValueError, match="label_smoothing"):
        S.OneVsAllTrainer(m, label_smoothing=1.0)
    for bad in (-0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="n3"):
            S.OneVsAllTrainer(m, n3=bad)
    S.set_deterministic(True)
    try:
        with pytest.raises(ValueError, match="deterministic"):
            S.OneVsAllTrainer(m)
    finally:
        S.set_deterministic(False)
    assert onevsall.MAX_BATCH == 4096
    # the refusals of fit(): a model with sz reaches them without a device
    m.sz = (20, 20, 3)
    xs = [(i % 20, (3 * i + 1) % 20, i % 3) for i in range(40)]
    with pytest.raises(ValueError, match="y != 1") as e:
        S.OneVsAllTrainer(m, nbatches=2).fit(xs, [1] * 39 + [-1])
    assert "labelled negatives" in str(e.value)
    big = type("DistMult", (Fake,), {})(5)
    big.sz = (5000, 5000, 1)
    many = [(i, (i + 1) % 5000, 0) for i in range(5000)]
    with pytest.raises(ValueError, match="nbatches") as e:
        S.OneVsAllTrainer(big, nbatches=2, max_epochs=1).fit(many)
    assert "4096" in str(e.value) and "5000" in str(e.value)
    with pytest.raises(ValueError, match="nbatches"):
        S.OneVsAllTrainer(m, nbatches=81).fit(xs)
    # the model refusal names the regime that was asked for
    with pytest.raises(ValueError, match="1vsAll"):
        S.OneVsAllTrainer(type("HolE", (Fake,), {})(2))
