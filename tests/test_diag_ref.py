"""CPU checks for DistMult and ComplEx: the fp64 reference (tests/diag_ref.py)
against finite differences and its own identities, the facade's constructor
rules, the library's host-side argument checks for the model codes 5 and 6
(code 4 stays refused) and the runners' refusal texts."""
import ctypes

import numpy as np
import pytest

import diag_ref as DR
from oracle import skge_oracle as O


def _rows(model, d, seed):
    rs = np.random.RandomState(seed)
    return rs.randn(d), rs.randn(d), rs.randn(d)


@pytest.mark.parametrize("model", DR.MODELS)
@pytest.mark.parametrize("d", [2, 8, 50])
def test_gradients_match_finite_differences(model, d):
    s, r, o = _rows(model, d, 1)
    h = 1e-6
    for name, grad, at in (("s", DR.d_s(model, r, o), 0), ("r", DR.d_r(model, s, o), 1),
                           ("o", DR.d_o(model, s, r), 2)):
        fd = np.zeros(d)
        for k in range(d):
            hi = [s.copy(), r.copy(), o.copy()]
            lo = [s.copy(), r.copy(), o.copy()]
            hi[at][k] += h
            lo[at][k] -= h
            fd[k] = (DR.phi(model, *hi) - DR.phi(model, *lo)) / (2 * h)
        # phi is linear in each argument: the central difference is exact up to
        # rounding, |phi| eps / h ~ 1e-9 here
        np.testing.assert_allclose(grad, fd, rtol=0, atol=1e-7, err_msg="%s d/d%s" % (model, name))


@pytest.mark.parametrize("model", DR.MODELS)
def test_query_vector_identities(model):
    s, r, o = _rows(model, 50, 2)
    want = DR.phi(model, s, r, o)
    for q, x in ((DR.q_tail(model, s, r), o), (DR.q_head(model, r, o), s),
                 (DR.q_rel(model, s, o), r)):
        np.testing.assert_allclose(q.dot(x), want, rtol=1e-13, atol=1e-13)


def test_complex_with_zero_imaginary_parts_is_distmult():
    rs = np.random.RandomState(3)
    re = rs.randn(3, 25)
    x = np.zeros((3, 50))
    x[:, 0::2] = re
    np.testing.assert_allclose(DR.phi("complex", *x), DR.phi("distmult", *re), rtol=1e-13)
    np.testing.assert_allclose(DR.d_s("complex", x[1], x[2])[0::2], DR.d_s("distmult", re[1], re[2]))
    assert np.all(DR.d_s("complex", x[1], x[2])[1::2] == 0)


def test_pairwise_step_reduces_to_hole_conventions():
    """the contribution lists, the mean and rparam's place are HolE's: with the
    same pairs the gradient's row indices are the oracle's HolE indices"""
    E, R = DR.tables("distmult", 40, 5, 8, 4)
    pos, neg = DR.forced_pairs(40, 5, 64, 5)
    _, _, nv, g = DR.pairwise_gradients("distmult", E, R, pos, neg, 0.2, rparam=0.01)
    _, _, nvh, gh = O.hole_pairwise_gradients(E, R, pos, neg, 10.0, rparam=0.01)
    assert nv > 0 and nvh == len(pos)
    _, _, nva, ga = DR.pairwise_gradients("distmult", E, R, pos, neg, 10.0, rparam=0.01)
    assert nva == nvh
    for pid in ("E", "R"):
        np.testing.assert_array_equal(ga[pid][1], gh[pid][1])


def test_odd_width_raises_for_complex_only():
    import skge_amd as S
    with pytest.raises(ValueError, match="even"):
        S.ComplEx((10, 10, 3), 7, init="unused")
    with pytest.raises(ValueError, match="even"):
        DR.d_s("complex", np.zeros(3), np.zeros(3))
    assert S.DistMult.model_code == 5 and S.ComplEx.model_code == 6
    assert S.DistMult.rel_id == S.ComplEx.rel_id == "R"


# ---- the library's host-side checks (no GPU: they precede the first launch) ----

def test_step_path_takes_5_and_6_and_refuses_4():
    from skge_amd import _lib as L
    lib = L.load()
    for model in (L.SKGE_DISTMULT, L.SKGE_COMPLEX):
        for logistic in (0, 1):
            for d, km in ((8, 1), (50, 1), (130, 3), (200, 4)):
                assert lib.skge_step_path(model, logistic, d, 18, 100) == \
                    L.SKGE_PATH_GENERIC | km << 8
    assert lib.skge_step_path(4, 0, 8, 18, 100) == -1
    assert b"model" in lib.skge_last_error()
    assert lib.skge_step_path(7, 0, 8, 18, 100) == -1
    assert lib.skge_step_path(L.SKGE_COMPLEX, 0, 7, 18, 100) == -1
    assert b"even" in lib.skge_last_error()
    assert lib.skge_step_path(L.SKGE_DISTMULT, 0, 7, 18, 100) == L.SKGE_PATH_GENERIC | 1 << 8
    for f in (lib.skge_pair_step_workspace_bytes, lib.skge_triple_step_workspace_bytes):
        assert f(L.SKGE_DISTMULT, 256, 18, 200) == 0 and f(L.SKGE_COMPLEX, 256, 18, 200) == 0


def _topk(lib, **kw):
    import test_topk_ref as TT
    return TT._call(lib, **kw)


def test_topk_argument_checks_pass_5_and_6():
    """reached as test_topk_ref._call reaches them: a good call but for the
    workspace, which is checked after the model code"""
    from skge_amd import _lib as L
    lib = L.load()
    for model in (L.SKGE_DISTMULT, L.SKGE_COMPLEX):
        assert _topk(lib, model=model, ws_bytes=64) == -1
        assert b"workspace" in lib.skge_last_error()
        assert _topk(lib, model=model, nq=0, ws=None, ws_bytes=0) == 0
    assert _topk(lib, model=4, ws_bytes=64) == -1 and b"model" in lib.skge_last_error()
    assert _topk(lib, model=L.SKGE_COMPLEX, d=7, ws_bytes=64) == -1
    assert b"even" in lib.skge_last_error()


def test_score_argument_checks_pass_5_and_6():
    from skge_amd import _lib as L
    lib = L.load()
    host = lambda ct, m: ctypes.cast((ct * m)(), ctypes.c_void_p)
    E, R, trip, out = (host(ctypes.c_float, 128), host(ctypes.c_float, 16),
                       host(ctypes.c_int, 12), host(ctypes.c_float, 4))
    call = lambda model, d, ws, nb: lib.skge_score(None, model, E, R, 16, 2, d, trip, 4, ws, nb, out)
    for model in (L.SKGE_DISTMULT, L.SKGE_COMPLEX):
        assert lib.skge_score_workspace_bytes(model, 4, 2, 8) == 256
        assert call(model, 8, None, 0) == -1 and b"workspace" in lib.skge_last_error()
        assert lib.skge_score(None, model, E, R, 16, 2, 8, trip, 0, None, 0, out) == 0
    assert lib.skge_score_workspace_bytes(4, 4, 2, 8) == 0
    assert call(4, 8, None, 0) == -1 and b"model" in lib.skge_last_error()
    assert lib.skge_score_workspace_bytes(L.SKGE_COMPLEX, 4, 2, 7) == 0
    assert call(L.SKGE_COMPLEX, 7, None, 0) == -1 and b"even" in lib.skge_last_error()


def test_subgraph_rank_refuses_the_new_codes():
    from skge_amd import _lib as L
    lib = L.load()
    P = lambda n: ctypes.cast((ctypes.c_char * n)(), ctypes.c_void_p)
    for model in (4, L.SKGE_DISTMULT, L.SKGE_COMPLEX):
        rc = lib.skge_subgraph_rank(None, model, P(512), P(512), 4, 4, P(512), 2, P(64), 1, P(64),
                                    P(64), P(64), P(64), P(4096), 4096, P(64), P(64))
        assert rc == -1 and b"model" in lib.skge_last_error(), model


# ---- the runners' refusals ----

@pytest.mark.parametrize("runner", ["pipe", "epoch", "hole_pipe"])
@pytest.mark.parametrize("cls", ["DistMult", "ComplEx"])
def test_runner_refusals_name_pairs(cls, runner):
    """refused before anything touches the device"""
    import skge_amd as S
    from skge_amd.device import make_runner
    m = getattr(S, cls).__new__(getattr(S, cls))
    with pytest.raises(ValueError, match="'pairs'"):
        make_runner(m, None, None, 3, runner=runner)
    from skge_amd.dp import DataParallelRunner
    with pytest.raises(ValueError, match="'pairs'"):
        DataParallelRunner(m, None, None, 3)


# ---- the evaluation tests' inputs meet the cap with the reference alone ----

EVAL_CASES = [(model, N, M, d) for model in DR.MODELS for N, M in ((63, 3), (512, 18))
              for d in (8, 50)]
NQ, TOPK = 40, 5


@pytest.mark.parametrize("model,N,M,d", EVAL_CASES)
def test_envelope_leaves_at_most_one_percent_unforced(model, N, M, d):
    """tests/test_gpu_diag.py asserts the sandwich on these inputs; here the
    share of it that the envelope leaves open (a rank with lo != hi, a top-k
    place without a forced member) is at most 1%, test_topk_ref's cap."""
    E, R, test, known = DR.eval_case(model, N, M, d, NQ, 100 + d + N)
    lo, hi = DR.rank_envelope(model, E, R, test, known)
    rlo, rhi = DR.relation_envelope(model, E, R, test, known)
    open_ranks = int((lo != hi).sum()) + int((rlo != rhi).sum())
    total = lo.size + rlo.size
    forced = places = 0
    for s, o, p in test.tolist():
        for slot in ("tail", "head", "rel"):
            f, n = DR.topk_forced(model, E, R, s, o, p, slot, TOPK)
            forced += len(f)
            places += n
    share = (open_ranks + (places - forced)) / float(total + places)
    print("%s N=%d M=%d d=%d: open share %.4f" % (model, N, M, d, share))
    assert share <= 0.01
