"""CPU checks of the integer-exact references for DistMult and ComplEx (the
"distmult" / "complex" branches of eval_ref._int_query_vectors and
relation_ref.int_relation_scores): they agree with tests/diag_ref.py evaluated
in fp64 on the same integer tables, the models' identities hold in them, and
the cases of tests/test_gpu_diag_exact.py are not vacuous.  The case lists of
that file live here, so that they are judged without a GPU."""
import functools

import numpy as np
import pytest

import diag_ref as DR
import eval_ref as X
import relation_ref as RR
import topk_ref as T

# (d, N, nq): eval_ref._COMMON's edges without its two large-N cases (past the
# query vector the ranking tile is HolE's) -- d < 4, the scalar tail, the 32-dim
# chunk boundary, 64 / 65, N = 1, d = 1024; ComplEx at the nearest even widths
CASES = {"distmult": [(1, 300, 97), (3, 129, 33), (31, 63, 31), (32, 64, 32), (33, 65, 33),
                      (65, 128, 97), (33, 1, 31), (1024, 130, 33)],
         "complex": [(2, 300, 97), (30, 63, 31), (32, 64, 32), (34, 65, 33), (66, 128, 97),
                     (34, 1, 31), (1024, 130, 33)]}
INT_CASES = [(m,) + c for m in DR.MODELS for c in CASES[m]]
POOL_CASES = [(m,) + c for m in DR.MODELS for c in CASES[m] if c[0] in (32, 33, 34, 65, 66)]
M_ENT, M_REL = 3, 40


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def entity_case(model, d, N, nq):
    """(E, R, test, known): eval_ref.make_int_case, M = 3"""
    return _frozen(*X.make_int_case(model, d, N, nq, X.case_seed("diag", model, d, N, nq),
                                    M=M_ENT))


@functools.lru_cache(maxsize=None)
def relation_case(model, d, N, nq):
    """(E, R, test, known): relation_ref.make_int_case, M = 40"""
    return _frozen(*RR.make_int_case(model, d, N, M_REL, nq,
                                     X.case_seed("diag-rel", model, d, N, nq)))


def test_case_lists_are_the_issues():
    assert [c[0] for c in CASES["complex"]] == [2, 30, 32, 34, 66, 34, 1024]
    assert all(c[0] % 2 == 0 for c in CASES["complex"])
    assert len(INT_CASES) == 15 and len(POOL_CASES) == 8


@pytest.mark.parametrize("model,d,N,nq", INT_CASES)
def test_int_scores_agree_with_the_fp64_reference(model, d, N, nq):
    """int64 and fp64 agree exactly: every value is an integer below 2^53"""
    E, R, test, known = entity_case(model, d, N, nq)
    assert np.abs(E).max() <= 3 and np.abs(R).max() <= 3 and 54 * d < 2 ** 24
    for s, o, p in test[:12].tolist():
        for direction in ("tail", "head"):
            got = X.int_scores(model, E, R, s, o, p, direction)
            want = DR.entity_scores(model, E, R, s, o, p, direction)
            assert got.dtype == np.int64 and np.array_equal(got, want), (s, o, p, direction)
            assert np.abs(got).max() <= 54 * d
        assert X.int_scores(model, E, R, s, o, p, "tail")[o] == DR.phi(model, E[s], R[p], E[o])
    E, R, test, known = relation_case(model, d, N, nq)
    sc = RR.int_relation_scores(model, E, R, test[:12, :2])
    for i, (s, o, p) in enumerate(test[:12].tolist()):
        assert np.array_equal(sc[i], DR.relation_scores(model, E, R, s, o))
    q = test[:12, [0, 2]]
    assert np.array_equal(T.int_query_scores(model, E, R, q, "tail")[0],
                          DR.entity_scores(model, E, R, q[0, 0], 0, q[0, 1], "tail"))


@pytest.mark.parametrize("model,d,N,nq", INT_CASES)
def test_exact_cases_are_not_vacuous(model, d, N, nq):
    """ties occur, ranks spread, and the filter moves some of them"""
    E, R, test, known = entity_case(model, d, N, nq)
    want = X.exact_ranks(model, E, R, X.eval_order(test), known)
    assert want.shape == (nq, 4) and (want >= 1).all() and (want <= N).all()
    assert (want[:, 1] <= want[:, 0]).all() and (want[:, 3] <= want[:, 2]).all()
    if N == 1:
        assert (want == 1).all()
        return
    assert len(np.unique(want[:, 0])) > 3 and len(np.unique(want[:, 2])) > 3
    assert (want[:, 1] < want[:, 0]).any() or (want[:, 3] < want[:, 2]).any()
    s, o, p = (int(v) for v in test[0])
    sc = X.int_scores(model, E, R, s, o, p, "tail")
    if d <= 66:
        assert len(np.unique(sc)) < N      # exact ties: the top-k order is pinned by ids
    E, R, test, known = relation_case(model, d, N, nq)
    rw = RR.exact_relation_ranks(model, E, R, X.eval_order(test), known)
    assert len(np.unique(rw[:, 0])) > 3 and (rw[:, 1] < rw[:, 0]).any()


def test_unknown_model_is_still_refused():
    E = np.ones((4, 2))
    with pytest.raises(ValueError, match="unknown model"):
        X.int_scores("simple", E, E, 0, 1, 2, "tail")
    with pytest.raises(ValueError, match="unknown model"):
        RR.int_relation_scores("simple", E, E, [(0, 1)])
    with pytest.raises(ValueError, match="even"):
        X.int_scores("complex", np.ones((4, 3)), np.ones((4, 3)), 0, 1, 2, "tail")
    with pytest.raises(AssertionError):     # entries past [-3, 3]: the bound is not met
        X.int_diag_mul("distmult", np.full((1, 4), 4), np.ones((1, 4), dtype=np.int64), False)


# ---- the identities, in the integer references ----

def real_halves(E, R):
    """the DistMult tables on the real halves of ComplEx tables"""
    return E[:, 0::2].copy(), R[:, 0::2].copy()


def zero_imag(E, R):
    E, R = E.copy(), R.copy()
    E[:, 1::2] = 0
    R[:, 1::2] = 0
    return E, R


def conj_rows(R):
    R = R.copy()
    R[:, 1::2] *= -1
    return R


@pytest.mark.parametrize("d", [66, 130])
def test_complex_with_zero_imaginary_parts_is_distmult(d):
    E, R, test, known = X.make_int_case("complex", d, 70, 40, X.case_seed("diag-zero", d))
    Ez, Rz = zero_imag(E, R)
    Er, Rr = real_halves(E, R)
    q = X.eval_order(test)
    np.testing.assert_array_equal(X.exact_ranks("complex", Ez, Rz, q, known),
                                  X.exact_ranks("distmult", Er, Rr, q, known))
    for direction in T.DIRECTIONS:
        qq = q[:, [0, 2]] if direction == "tail" else q[:, [1, 2]]
        np.testing.assert_array_equal(T.int_query_scores("complex", Ez, Rz, qq, direction),
                                      T.int_query_scores("distmult", Er, Rr, qq, direction))
    np.testing.assert_array_equal(RR.int_relation_scores("complex", Ez, Rz, q[:, :2]),
                                  RR.int_relation_scores("distmult", Er, Rr, q[:, :2]))


@pytest.mark.parametrize("model", DR.MODELS)
@pytest.mark.parametrize("d", [66, 130])
def test_swapping_s_and_o_under_the_conjugate_relation(model, d):
    """phi(s, r, o) = phi(o, conj(r), s): the tail scores of (s, ?, p) under R
    are the head scores of (?, s, p) under conj(R) (DistMult: R itself)"""
    E, R, test, known = X.make_int_case(model, d, 70, 40, X.case_seed("diag-swap", model, d))
    Rc = conj_rows(R) if model == "complex" else R
    rs = np.random.RandomState(d)
    s, r, o = E[rs.randint(70, size=50)], R[rs.randint(3, size=50)], E[rs.randint(70, size=50)]
    rc = conj_rows(r) if model == "complex" else r
    np.testing.assert_array_equal(DR.phi(model, s, r, o), DR.phi(model, o, rc, s))
    q = X.eval_order(test)
    want = X.exact_ranks(model, E, R, q, known)
    swapped = X.exact_ranks(model, E, Rc, q[:, [1, 0, 2]], known[:, [1, 0, 2]])
    np.testing.assert_array_equal(swapped[:, [2, 3, 0, 1]], want)
    if model == "complex":      # and the conjugate matters: without it the columns differ
        plain = X.exact_ranks(model, E, R, q[:, [1, 0, 2]], known[:, [1, 0, 2]])
        assert (plain[:, [2, 3, 0, 1]] != want).any()


def test_column_permuted_triples_reach_the_library_row_major():
    """test[:, [1, 0, 2]] is a column-major array; the facade hands the library
    a pointer to 3 consecutive ints per triple, so it has to lay them out
    itself (found by test_gpu_diag_exact's swap test: m.score read other ids)"""
    from skge_amd.linkpred import host_triples
    from skge_amd.util import triples_array
    test = np.arange(30, dtype=np.int32).reshape(10, 3)
    swapped = test[:, [1, 0, 2]]
    assert not swapped.flags["C_CONTIGUOUS"]
    for f in (host_triples, triples_array):
        for arr in (swapped, swapped.astype(np.int64), test[::2], test.T[:, :3].T):
            out = f(arr)
            assert out.flags["C_CONTIGUOUS"] and out.shape == arr.shape
            assert np.array_equal(out, arr)
            assert np.array_equal(np.frombuffer(out.tobytes(), dtype=out.dtype),
                                  np.asarray(arr).reshape(-1))
