"""CPU checks of KvsAll: the fp64 restatement's gradients against central
differences of its own loss, KvsAllQueries on a hand-written KG, and the three
entry points in the header, the library and the ctypes table."""
import os
import re

import numpy as np
import pytest

import kvsall_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("skge_kvsall_workspace_bytes", "skge_kvsall_grad", "skge_kvsall_step")


def fd_case(model, direction):
    """N = 6, M = 3, d = 4; queries 0 and 1 repeat an anchor, 1 and 2 share a
    relation, query 0 answers with its own anchor (a self-loop)."""
    rng = np.random.RandomState(7)
    E = rng.uniform(-1, 1, size=(6, 4))
    R = rng.uniform(-1, 1, size=(3, 4))
    anchor = np.array([2, 2, 4, 5])
    rel = np.array([0, 1, 1, 2])
    dirn = {"tail": np.zeros(4, dtype=int), "head": np.ones(4, dtype=int),
            "mixed": np.array([0, 1, 1, 0])}[direction]
    lists = [[2, 3], [0], [1, 4, 5], []]
    off = np.cumsum([0] + [len(x) for x in lists])
    ans = np.array([e for x in lists for e in x])
    return E, R, (anchor, rel, dirn, off, ans)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("direction", ["tail", "head", "mixed"])
@pytest.mark.parametrize("model", KR.MODELS)
def test_gradients_match_central_differences(model, direction, eps):
    """h = 1e-5 in fp64; tolerance 1e-7 + 1e-5 |g|: truncation ~ h^2, round-off
    ~ 2^-52 |L| / h = 2e-9 for |L| <= 100."""
    E, R, batch = fd_case(model, direction)
    fw, gE, gR, touched = KR.gradients(model, E, R, *batch, eps)
    assert abs(fw["loss"]) <= 100
    h = 1e-5
    for name, P, g in (("E", E, gE), ("R", R, gR)):
        num = np.zeros_like(P)
        for i in np.ndindex(*P.shape):
            keep = P[i]
            P[i] = keep + h
            up = KR.loss(model, E, R, *batch, eps)
            P[i] = keep - h
            dn = KR.loss(model, E, R, *batch, eps)
            P[i] = keep
            num[i] = (up - dn) / (2 * h)
        err = np.abs(num - g)
        assert np.all(err <= 1e-7 + 1e-5 * np.abs(g)), (name, float(err.max()))
    assert touched.tolist() == [True, True, True]
    assert np.any(gR != 0)


def test_untouched_relation_rows_have_zero_gradient():
    E, R, batch = KR.build_case("complex", 40, KR.EDGE_M, 9, 6, seed=3)
    _, _, gR, touched = KR.gradients("complex", E, R, *batch, 0.1)
    assert not touched[1::2].any() and touched.any()
    assert np.all(gR[~touched] == 0)


def test_label_smoothing_and_loss_definition():
    """L restated term by term with logs (not the softplus form)."""
    E, R, batch = fd_case("distmult", "mixed")
    fw = KR.forward("distmult", E, R, *batch, 0.1)
    s = KR.sigmoid(fw["z"])
    want = -(fw["y"] * np.log(s) + (1 - fw["y"]) * np.log(1 - s)).sum() / 4
    assert abs(fw["loss"] - want) < 1e-12
    assert np.isclose(fw["y"][0, 2], 0.9 + 0.1 / 6) and np.isclose(fw["y"][0, 0], 0.1 / 6)


def test_invalid_queries_score_as_zero():
    """An anchor of N, a relation of M and a direction of 2: the gradients are
    those of the batch without the three queries, with B unchanged, and each of
    the three adds N log 2 / B to the loss.  Answer ids of -1 and N are no
    answers."""
    N, M, B, d = 40, 7, 9, 6
    E, R, (a, p, t, off, ans) = KR.build_case("complex", N, M, B, d, seed=3)
    a2, p2, t2 = a.copy(), p.copy(), t.copy()
    a2[1], p2[4], t2[6] = N, M, 2
    bad = [1, 4, 6]
    keep = np.setdiff1d(np.arange(B), bad)
    # -1 and N inside query 0's list
    ans2 = np.concatenate([ans[:1], [-1, N], ans[1:]]).astype(np.int32)
    off2 = off.copy()
    off2[1:] += 2
    assert off[1] - off[0] >= 1 and not KR.valid(a2, p2, t2, N, M)[bad].any()
    fw, gE, gR, touched = KR.gradients("complex", E, R, a2, p2, t2, off2, ans2, 0.1)
    lists = [ans[off[b]:off[b + 1]] for b in keep]
    offk = np.cumsum([0] + [len(x) for x in lists])
    fk, gEk, gRk, tk = KR.gradients("complex", E, R, a[keep], p[keep], t[keep], offk,
                                    np.concatenate(lists), 0.1)
    scale = len(keep) / float(B)
    assert np.allclose(gE, gEk * scale, rtol=1e-12, atol=1e-15)
    assert np.allclose(gR, gRk * scale, rtol=1e-12, atol=1e-15) and np.array_equal(touched, tk)
    assert np.isclose(fw["loss"], fk["loss"] * scale + 3 * N * np.log(2.0) / B, rtol=1e-12)
    assert np.all(fw["z"][bad] == 0) and np.all(fw["Q"][bad] == 0)
    assert np.array_equal(fw["y"][0], KR.forward("complex", E, R, a, p, t, off, ans, 0.1)["y"][0])


def test_plan_equals_the_library_workspace():
    """plan() restates kv_plan: the same bytes at every shape of the suites,
    the benchmark's and both sides of the plan's thresholds."""
    from skge_amd import _lib as L
    lib = L.load()
    grid = KR.plan_grid()
    assert len(set(grid)) > 150
    for B, N, M, d in grid:
        for code in (5, 6) if d % 2 == 0 else (5,):
            want = lib.skge_kvsall_workspace_bytes(code, B, N, M, d)
            assert want > 0 and KR.plan("kvsall", B, N, M, d).total == want, (B, N, M, d)
    # the thresholds are inside the grid: both values of each choice occur
    plans = [KR.plan("onevsall", *g) for g in grid]
    assert {p.ns == 1 for p, g in zip(plans, grid) if g[1] > KR.KC} == {False, True}
    assert {p.nsplit for p in plans} >= {1, 2, 3}
    assert {p.kslice for p in plans} >= {32, 64, 96}


def test_bench_shape_plans_to_the_regimes():
    N, B, d = KR.BENCH_SHAPE
    p = KR.plan("onevsall", B, N, KR.BENCH_M, d)
    # (the 16 MB cap, 40 slices, binds before the 512 workgroups' 64)
    assert (p.kslice, p.ns, p.nsplit, p.chunk, p.nby) == (1024, 40, 2, 20472, 320)
    assert all(KR.PREDICATES[k](p, N, B, d) for k in
               ("kslice > 32", "nsplit > 1", "chunk > 1024", "nby > 256", "nbx nby > 256"))


@pytest.mark.parametrize("shape", KR.REGIME_SHAPES, ids=KR.regime_id)
def test_regime_shape_meets_its_predicates(shape):
    N, B, d, models, (values, preds) = shape
    assert d % 2 == 0 or models == ("distmult",)
    p = KR.plan("onevsall", B, N, KR.EDGE_M, d)
    kv = KR.plan("kvsall", B, N, KR.EDGE_M, d)
    assert kv[:7] == p[:7] and (kv.nsplit, kv.chunk) == (0, 0)
    got = dict(p._asdict(), last=KR.last_slice(p, N))
    assert {k: got[k] for k in values} == values
    for k in preds:
        assert KR.PREDICATES[k](p, N, B, d), k
    assert B <= 4096 and d <= 1024 and 3 * N < 2 ** 24


def test_regime_shapes_cover_what_edge_shapes_do_not():
    def met(shapes):
        out = set()
        for s in shapes:
            N, B, d = s[:3]
            p = KR.plan("onevsall", B, N, KR.EDGE_M, d)
            out |= {k for k, f in KR.PREDICATES.items() if f(p, N, B, d)}
        return out

    assert met(KR.REGIME_SHAPES) == set(KR.PREDICATES)
    assert KR.GAP == ["kslice > 32", "ns == 1 < chunks", "nsplit > 1", "chunk > 1024",
                      "nby > 256", "nbx nby > 256"]
    assert not met(KR.EDGE_SHAPES) & set(KR.GAP)
    # every claimed predicate is claimed by name somewhere, not met by accident
    claimed = {k for s in KR.REGIME_SHAPES for k in s[4][1]}
    assert claimed == set(KR.PREDICATES)
    # the exact test's extra shapes keep the slices of the shapes they stand for:
    # several chunks each, the last one ragged past one chunk
    for (N, B, d, _), want in zip(KR.EXACT_EXTRA_SHAPES, ((96, 342, 65), (64, 130, 44))):
        assert B & (B - 1) == 0
        p = KR.plan("kvsall", B, N, KR.EDGE_M, d)
        assert (p.kslice, p.ns, KR.last_slice(p, N)) == want
        assert KR.PREDICATES["last slice past one chunk"](p, N, B, d)


def test_build_case_puts_answers_at_the_split_seams():
    for N, B, d in ((1025, 3, 2), (2501, 600, 2), (32801, 2, 2)):
        ids = KR.split_ids(N, KR.EDGE_M, B, d)
        chunk = KR.plan("onevsall", B, N, KR.EDGE_M, d).chunk
        assert ids[:4] == [chunk, N - 1, chunk - 1, 0] and (N & ~3) in ids
        _, _, (a, p, t, off, ans) = KR.build_case("distmult", N, KR.EDGE_M, B, d, seed=1)
        assert set(ids) <= set(ans[off[1]:off[2]].tolist())
        assert a[0] == a[1] and a[0] in ans[off[0]:off[1]]
    assert KR.split_ids(8300, KR.EDGE_M, 130, 130) == [1040, 8299, 1039, 0]
    assert all(KR.split_ids(N, KR.EDGE_M, B, d) == [] for N, B, d in KR.EDGE_SHAPES)


# (s, o, p): duplicated triples, a self-loop (3, 3, 0), entity 4 only ever an object
KG = [(0, 1, 0), (0, 2, 0), (0, 1, 0), (3, 3, 0), (1, 4, 1), (2, 4, 1), (2, 4, 1), (0, 4, 0)]
SZ = (5, 5, 2)


def test_queries_order_and_answers():
    from skge_amd.kvsall import KvsAllQueries
    q = KvsAllQueries.from_triples(KG, SZ)
    got = [(int(t), int(p), int(a), q.ans[q.off[i]:q.off[i + 1]].tolist())
           for i, (t, p, a) in enumerate(zip(q.dir, q.rel, q.anchor))]
    assert got == [
        (0, 0, 0, [1, 2, 4]), (0, 0, 3, [3]), (0, 1, 1, [4]), (0, 1, 2, [4]),
        (1, 0, 1, [0]), (1, 0, 2, [0]), (1, 0, 3, [3]), (1, 0, 4, [0]), (1, 1, 4, [1, 2]),
    ]
    assert q.off[0] == 0 and q.off[-1] == len(q.ans) and len(q) == 9
    assert all(a.dtype == np.int32 for a in (q.anchor, q.rel, q.dir, q.off, q.ans))
    # entity 4 anchors no tail query
    assert 4 not in q.anchor[q.dir == 0].tolist()


def test_queries_single_direction_and_refusals():
    from skge_amd.kvsall import KvsAllQueries
    both = KvsAllQueries.from_triples(KG, SZ)
    tail = KvsAllQueries.from_triples(KG, SZ, directions=("tail",))
    head = KvsAllQueries.from_triples(KG, SZ, directions=("head",))
    assert len(tail) + len(head) == len(both) and len(tail) == 4
    assert np.all(tail.dir == 0) and np.all(head.dir == 1)
    with pytest.raises(ValueError, match="sideways"):
        KvsAllQueries.from_triples(KG, SZ, directions=("sideways",))
    with pytest.raises(ValueError, match="outside"):
        KvsAllQueries.from_triples([(0, 5, 0)], SZ)


def test_queries_batch_round_trips():
    from skge_amd.kvsall import KvsAllQueries
    q = KvsAllQueries.from_triples(KG, SZ)
    whole = q.batch(np.arange(len(q)))
    for name in ("anchor", "rel", "dir", "off", "ans"):
        assert np.array_equal(getattr(whole, name), getattr(q, name)), name
    ids = [8, 0, 3, 0]
    b = q.batch(ids)
    assert b.off.tolist() == [0, 2, 5, 6, 9] and b.ans.tolist() == [1, 2, 1, 2, 4, 4, 1, 2, 4]
    assert b.anchor.tolist() == [4, 0, 2, 0] and b.dir.tolist() == [1, 0, 0, 0]
    assert len(q.batch([])) == 0 and q.batch([]).off.tolist() == [0]
    # a batch of a batch
    assert b.batch([1]).ans.tolist() == [1, 2, 4]


def test_header_library_and_ctypes_name_the_entry_points():
    from skge_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "skge_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = L.load()
    for f in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % f, src), f
        assert hasattr(lib, f), f
        assert f in L.SIGNATURES, f
    assert len(L.SIGNATURES["skge_kvsall_grad"][1]) == 21
    assert len(L.SIGNATURES["skge_kvsall_step"][1]) == 15
    assert lib.skge_abi_version() == 2


def test_entry_points_refuse_without_a_gpu():
    """Model codes 0..3 and 7: SKGE_ENOTSUP, by name; 4: SKGE_EINVAL; the size
    limits, each naming what was asked."""
    from skge_amd import _lib as L
    lib = L.load()
    grad = lambda model, N=10, M=2, d=4, B=3, eps=0.0: lib.skge_kvsall_grad(
        None, model, None, None, N, M, d, None, None, None, B, None, None, eps, None, None, None,
        None, None, None, 0)
    step = lambda model, d=4, B=3: lib.skge_kvsall_step(
        None, model, None, None, d, None, None, None, B, None, None, 0.0, None, None, 0)
    names = {0: b"TransE-L1", 1: b"TransE-L2", 2: b"HolE", 3: b"RESCAL", 7: b"RotatE"}
    for code, name in names.items():
        for call in (grad, step):
            assert call(code) == -3, code
            msg = lib.skge_last_error()
            assert name in msg and b"DistMult" in msg and b"ComplEx" in msg, msg
        assert lib.skge_kvsall_workspace_bytes(code, 3, 10, 2, 4) == 0
    for call in (grad, step):
        assert call(4) == -1 and b"unknown model 4" in lib.skge_last_error()
    assert grad(5, B=4097) == -3 and b"4097" in lib.skge_last_error()
    assert grad(5, d=1025) == -3 and b"1025" in lib.skge_last_error()
    assert grad(5, B=0) == -1 and grad(5, N=0) == -1 and grad(5, M=0) == -1
    assert grad(6, d=5) == -1 and b"even" in lib.skge_last_error()
    assert grad(5, eps=1.0) == -1 and b"smoothing" in lib.skge_last_error()
    assert grad(5) == -1 and b"NULL" in lib.skge_last_error()
    assert lib.skge_kvsall_workspace_bytes(5, 4097, 10, 2, 4) == 0
    # G is indexed in size_t: B N past 2^31 elements
    big = lib.skge_kvsall_workspace_bytes(5, 4096, 1 << 20, 2, 4)
    assert big > 4 * 4096 * (1 << 20)
    assert lib.skge_kvsall_workspace_bytes(6, 3, 10, 2, 4) > 0


def test_trainer_refusals_name_their_reason():
    """The trainer's refusals that need no device."""
    import skge_amd as S
    from skge_amd import kvsall

    class Fake(S.Model):   # a model object without device tables
        model_code = None

        def __init__(self, code):
            self.model_code = code
            self.params, self.hyperparams = {}, {}

    for cls_name, code in (("HolE", 2), ("RESCAL", 3), ("TransE", 0), ("RotatE", 7)):
        m = type(cls_name, (Fake,), {})(code)
        with pytest.raises(ValueError, match=cls_name) as e:
            S.KvsAllTrainer(m)
        assert "DistMult" in str(e.value) and "ComplEx" in str(e.value)
    m = type("DistMult", (Fake,), {})(5)
    with pytest.raises(ValueError, match="samplef"):
        S.KvsAllTrainer(m, samplef=lambda x: x)
    with pytest.raises(ValueError, match="device_loop"):
        S.KvsAllTrainer(m, device_loop=True)
    with pytest.raises(ValueError, match="device_runner"):
        S.KvsAllTrainer(m, device_runner="pipe")
    with pytest.raises(ValueError, match="label_smoothing"):
        S.KvsAllTrainer(m, label_smoothing=1.0)
    S.set_deterministic(True)
    try:
        with pytest.raises(ValueError, match="deterministic"):
            S.KvsAllTrainer(m)
    finally:
        S.set_deterministic(False)
    assert kvsall.MAX_BATCH == 4096
