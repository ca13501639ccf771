"""CPU checks of tests/rotate_ref.py (the fp64 RotatE restatement), of the
cases the GPU tests rely on, and of the host-side refusals of
SKGE_POST_UNITMOD and of model code 7 that need no device."""
import ctypes

import numpy as np
import pytest

import rotate_ref as RR

N, M, D = 12, 3, 10


def _tables(seed=0):
    rs = np.random.RandomState(seed)
    E = rs.uniform(-1, 1, (N, D))
    R = RR.unitmod_rows(rs.uniform(-1, 1, (M, D)))
    return E, R


def test_gradients_match_central_differences():
    E, R = _tables(1)
    trip = np.array([[0, 1, 2], [3, 3, 0], [5, 7, 1]])
    m = np.abs(RR.cplx(E[trip[:, 0]]) * RR.cplx(R[trip[:, 2]]) - RR.cplx(E[trip[:, 1]]))
    assert m.min() > 1e-2   # every component well away from the kink
    gs, go, gr = RR.triple_grads(E, R, trip)
    h = 1e-6
    for i, (s, o, p) in enumerate(trip):
        for tab, row, g in ((E, s, gs[i]), (E, o, go[i]), (R, p, gr[i])):
            for k in range(D):
                keep = tab[row, k]
                tab[row, k] = keep + h
                up = RR.scores(E, R, trip[i:i + 1])[0]
                tab[row, k] = keep - h
                dn = RR.scores(E, R, trip[i:i + 1])[0]
                tab[row, k] = keep
                want = (up - dn) / (2 * h)
                if s == o and tab is E:   # one row in both places: the two gradients add
                    assert abs(want - (gs[i][k] + go[i][k])) < 1e-6
                else:
                    assert abs(want - g[k]) < 1e-6


def test_unit_relation_identity_and_rotation_invariance():
    E, R = _tables(2)
    s, o, r = RR.cplx(E[0]), RR.cplx(E[1]), RR.cplx(R[0])
    np.testing.assert_allclose(np.abs(s * r - o), np.abs(s - np.conj(r) * o), atol=1e-14)
    np.testing.assert_allclose(np.abs(s * r), np.abs(s), atol=1e-14)


def test_unit_vector_is_zero_where_the_modulus_is():
    E, R = _tables(3)
    E[1] = RR.inter(RR.cplx(E[0]) * RR.cplx(R[0]))   # o = s * r exactly on component 0 ...
    gs, go, gr = RR.triple_grads(E, R, [[0, 1, 0]])
    u = RR.cplx(E[0]) * RR.cplx(R[0]) - RR.cplx(E[1])
    assert np.all(u == 0)
    assert np.all(gs == 0) and np.all(go == 0) and np.all(gr == 0)


def test_unitmod_is_idempotent_and_maps_zero_to_one():
    rs = np.random.RandomState(4)
    X = rs.uniform(-2, 2, (5, 8))
    X[2, 4:6] = 0.0
    Y = RR.unitmod_rows(X.copy())
    np.testing.assert_allclose(np.abs(RR.cplx(Y)), 1.0, atol=1e-15)
    assert tuple(Y[2, 4:6]) == (1.0, 0.0)
    np.testing.assert_allclose(RR.unitmod_rows(Y.copy()), Y, atol=1e-15)
    # the package's host restatement (used by init) agrees, by rows too
    from skge_amd.param import unitmod
    np.testing.assert_allclose(unitmod(X.copy()), Y, atol=1e-15)
    Z = X.copy()
    unitmod(Z, [2, 3])
    np.testing.assert_allclose(Z[[2, 3]], Y[[2, 3]], atol=1e-15)
    np.testing.assert_array_equal(Z[[0, 1, 4]], X[[0, 1, 4]])
    with pytest.raises(ValueError):
        unitmod(np.ones((2, 3)))


def test_segment_mean_and_list_order():
    """One violating pair with sp == sn and pp == pn: the entity list is
    (sp, op, sn, on), the relation list (pp, pn), each id's rows averaged."""
    E, R = _tables(5)
    pos, neg = np.array([[0, 1, 2]]), np.array([[0, 4, 2]])
    ps, ns, nv, g = RR.pairwise_gradients(E, R, pos, neg, 100.0)
    assert nv == 1
    gsp, gop, grp = RR.triple_grads(E, R, pos)
    gsn, gon, grn = RR.triple_grads(E, R, neg)
    np.testing.assert_array_equal(g["E"][1], [0, 1, 4])
    np.testing.assert_allclose(g["E"][0][0], (-gsp[0] + gsn[0]) / 2)
    np.testing.assert_allclose(g["E"][0][1], -gop[0])
    np.testing.assert_allclose(g["E"][0][2], gon[0])
    np.testing.assert_array_equal(g["R"][1], [2])
    np.testing.assert_allclose(g["R"][0][0], (-grp[0] + grn[0]) / 2)
    # strict >: a pair at the margin exactly does not violate
    assert RR.pairwise_gradients(E, R, pos, pos, 0.0)[2] == 0


def test_step_projects_both_tables():
    E, R = _tables(6)
    params = {"E": E.copy(), "R": R.copy()}
    state = {k: np.zeros_like(v) for k, v in params.items()}
    pos, neg = RR.pairs(N, M, 8, 3)
    for opt in ("sgd", "adagrad"):
        _, _, nv, g = RR.pairwise_step(params, state, pos, neg, 0.1, 100.0, opt)
        assert nv == 8
        np.testing.assert_allclose(np.abs(RR.cplx(params["R"][g["R"][1]])), 1.0, atol=1e-14)
        np.testing.assert_allclose((params["E"][g["E"][1]] ** 2).sum(axis=1), 1.0, atol=1e-14)


@pytest.mark.parametrize("d", RR.WIDTHS)
def test_cases_the_gpu_test_relies_on(d):
    """Judged here, on the CPU: the score error bound is under half the bar,
    20-80% of the pairs violate, no decision is within 1e-5 of the margin."""
    E, R, pos, neg, scale, margin, seed = RR.case(d)
    assert RR.score_error_bound(E, R, np.concatenate([pos, neg])).max() <= RR.ERR_BAR
    ps, ns = RR.scores(E, R, pos), RR.scores(E, R, neg)
    gap = ns + margin - ps
    assert 0.2 <= (gap > 0).mean() <= 0.8
    assert np.abs(gap).min() > RR.GAP
    assert np.array_equal(E.astype(np.float32).astype(np.float64), E)   # held in fp32


def test_int_helpers():
    E = np.array([[1, 2, 0, -1], [1, 5, 3, -1], [1, 2, 0, -1]], dtype=np.int64)
    R = np.array([[0, 1, 1, 0]], dtype=np.int64)      # (i, 1)
    qt = RR.int_query(E, R, 0, 0, True)               # (1 + 2i) i = -2 + i; (0 - i)
    np.testing.assert_array_equal(qt, [-2, 1, 0, -1])
    qh = RR.int_query(E, R, 0, 0, False)              # conj(i) (1 + 2i) = 2 - i
    np.testing.assert_array_equal(qh, [2, -1, 0, -1])
    np.testing.assert_array_equal(RR.int_scores(np.array([1, 2, 0, -1]), E), [0, -6, 0])
    with pytest.raises(AssertionError):
        RR.int_scores(np.array([0, 0, 0, 0]), E)


# ---------------------------------------------------------------------------
# host-side refusals: no device is needed, nothing is dereferenced (the pattern
# of tests/test_runner_args.py: fake pointers, refused before the first HIP call)
# ---------------------------------------------------------------------------

T, N_ENT, N_REL, DW = 37, 11, 3, 8
FAKE = ctypes.c_void_p(0x1000)


def _table(L, rows, mode, slots, post):
    t = L.SkgeTable()
    t.param = t.state = t.acc_sum = t.acc_cnt = 0x1000
    t.acc_touched = 0x1000 if slots else None
    t.rows, t.width, t.touched_cap = rows, DW, 0
    t.acc_mode, t.acc_replicas = mode, 1
    t.post = post
    t.lr = 0.1
    return t


def _create(L, runner, post_rel):
    lib = L.load()
    packed = runner in ("pipe", "pipe_dp")
    mode = L.SKGE_ACC_I16X4 if packed else L.SKGE_ACC_F32
    ent = ctypes.byref(_table(L, N_ENT, mode, True, L.SKGE_POST_NORMALIZE))
    rel = ctypes.byref(_table(L, N_REL, mode, False, post_rel))
    tail = (FAKE, T, FAKE, 128, 5, 7, FAKE)
    if runner == "epoch":
        h = lib.skge_runner_create(None, 1, ent, rel, DW, *tail, 1.0, 100, None, None)
    elif runner == "pipe":
        h = lib.skge_pipe_runner_create(FAKE, ent, rel, DW, *tail, 1.0, 100, None)
    elif runner == "pipe_dp":
        h = lib.skge_pipe_runner_create_ex(FAKE, ent, rel, DW, *tail, 1.0, 100, None, 1)
    elif runner == "hole_pipe":
        h = lib.skge_hole_pipe_runner_create(FAKE, 0, ent, rel, DW, *tail, 1.0, 100, None)
    else:
        h = lib.skge_pair_runner_create(FAKE, L.SKGE_ROTATE, 0, ent, rel, DW, *tail, 1.0, 100, None)
    return h, lib.skge_last_error().decode()


@pytest.mark.parametrize("runner", ["epoch", "pipe", "pipe_dp", "hole_pipe"])
def test_unitmod_post_is_refused_by_name_where_it_is_not_applied(runner):
    from skge_amd import _lib as L
    h, err = _create(L, runner, L.SKGE_POST_UNITMOD)
    assert not h
    assert "SKGE_POST_UNITMOD" in err, err
    # the control: the same call with no projection passes this check and ends
    # at the backstop of test_runner_args.py (slot capacity / stream)
    h, err = _create(L, runner, L.SKGE_POST_NONE)
    assert not h
    assert "SKGE_POST_UNITMOD" not in err, err


def test_pair_runner_takes_rotate_and_its_post():
    """The pair loop serves model code 7 with a unit-modulus relation table: the
    call passes every argument check and ends at the backstop (an entity table
    with slot records and no capacity)."""
    from skge_amd import _lib as L
    h, err = _create(L, "pair", L.SKGE_POST_UNITMOD)
    assert not h
    assert "touched slots" in err, err


def test_host_refusals_of_rotate_name_it():
    from skge_amd import _lib as L
    lib = L.load()
    assert L.SKGE_ROTATE == 7 and L.SKGE_POST_UNITMOD == 3
    # skge_step_path reports no path for RotatE (one form at every width)
    assert lib.skge_step_path(L.SKGE_ROTATE, 1, 8, 3, 10) < 0
    assert "RotatE" in lib.skge_last_error().decode()
    assert lib.skge_step_path(4, 0, 8, 3, 10) < 0          # code 4 stays unassigned
    assert "RotatE" not in lib.skge_last_error().decode()
    # an odd width, at the pair loop's create
    ent = ctypes.byref(_table(L, N_ENT, L.SKGE_ACC_F32, True, 0))
    rel = ctypes.byref(_table(L, N_REL, L.SKGE_ACC_F32, False, 0))
    h = lib.skge_pair_runner_create(FAKE, L.SKGE_ROTATE, 0, ent, rel, 7, FAKE, T, FAKE, 128, 5, 7,
                                    FAKE, 1.0, 100, None)
    assert not h
    assert "RotatE needs an even d" in lib.skge_last_error().decode()
    # the triple (logistic) loop
    ent = ctypes.byref(_table(L, N_ENT, L.SKGE_ACC_F32, True, 0))
    rel = ctypes.byref(_table(L, N_REL, L.SKGE_ACC_F32, False, 0))
    h = lib.skge_triple_runner_create(FAKE, L.SKGE_ROTATE, ent, rel, DW, FAKE, T, FAKE, 128, 5, 7,
                                      FAKE, 100, None)
    assert not h
    assert "RotatE" in lib.skge_last_error().decode()
