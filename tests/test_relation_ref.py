"""CPU checks of tests/relation_ref.py (the references of
tests/test_gpu_relations.py) and of the relation entry points' ABI."""
import functools
import os
import re

import numpy as np
import pytest

import relation_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["skge_relrank_workspace_bytes", "skge_relrank", "skge_reltopk_workspace_bytes",
       "skge_reltopk"]
# the large cases are scored once, on the GPU test's side; here the small ones
SMALL = [c for c in RR.INT_CASES if c[3] * c[4] <= 300000 and c[1] <= 130]


@functools.lru_cache(maxsize=None)
def _int(model, d, N, M, nq):
    E, R, test, known = RR.int_case(model, d, N, M, nq)
    return E, R, test, known, RR.exact_relation_ranks(model, E, R, test, known)


@functools.lru_cache(maxsize=None)
def _float(model, d, scale):
    E, R, test, known = RR.float_case(model, d, scale)
    return E, R, test, known, RR.relation_rank_envelope(model, E, R, test, known)


@pytest.mark.parametrize("model,d,N,M,nq", SMALL)
def test_int_scores_equal_the_rounded_oracle_scores(model, d, N, M, nq):
    E, R, test = _int(model, d, N, M, nq)[:3]
    sc = RR.int_relation_scores(model, E, R, test[:8, :2])
    for i, (s, o, _) in enumerate(test[:8].tolist()):
        want = np.rint(RR.oracle_relation_scores(model, E, R, s, o)).astype(np.int64)
        np.testing.assert_array_equal(sc[i], want)
    if model == "transe":
        sc2 = RR.int_relation_scores(model, E, R, test[:8, :2], l2=True)
        for i, (s, o, _) in enumerate(test[:8].tolist()):
            want = np.rint(RR.oracle_relation_scores(model, E, R, s, o, l1=False)).astype(np.int64)
            np.testing.assert_array_equal(sc2[i], want)


@pytest.mark.parametrize("model,d,N,M,nq", [c for c in SMALL if c[4] <= 100])
def test_envelope_contains_the_exact_ranks(model, d, N, M, nq):
    E, R, test, known, exact = _int(model, d, N, M, nq)
    lo, hi = RR.relation_rank_envelope(model, E, R, test, known)
    assert (lo <= exact).all() and (exact <= hi).all()


@pytest.mark.parametrize("model,d,N,M,nq", [c for c in RR.INT_CASES if c[3] >= 8])
def test_int_cases_filter_moves_ranks(model, d, N, M, nq):
    """Not vacuous: with M >= 8 the filtered rank differs from the raw rank for
    at least one query in ten (the reference alone)."""
    exact = _int(model, d, N, M, nq)[4]
    moved = (exact[:, 0] != exact[:, 1]).mean()
    assert moved >= 0.1, moved
    assert (exact[:, 1] <= exact[:, 0]).all() and (exact >= 1).all() and (exact <= M).all()


@pytest.mark.parametrize("model,d,scale", RR.FLOAT_CASES)
def test_float_cases_pin_most_ranks(model, d, scale):
    """Not vacuous: lo == hi for at least nine in ten entries."""
    lo, hi = _float(model, d, scale)[4]
    assert (lo <= hi).all()
    assert (lo == hi).mean() >= 0.9, (lo == hi).mean()
    assert (lo[:, 0] != lo[:, 1]).any()      # the filter moves ranks here too


def test_triple_generator_density():
    rs = np.random.RandomState(5)
    test, known = RR.relation_triples(rs, 400, 20, 2000)
    kr = RR.known_relations(test, known, 20)
    n = np.array([len(x) for x in kr])
    assert 0.65 < (n > 0).mean() < 0.85             # three in four
    assert 7 < n[n > 0].mean() < 12                 # about half of the 19 others
    for (s, o, p), x in zip(test.tolist(), kr):
        assert p not in x.tolist() and (np.diff(x) > 0).all()
    assert {tuple(t) for t in test.tolist()} <= {tuple(t) for t in known.tolist()}


def test_topk_reference_orders_pads_and_excludes():
    E, R, test, known = RR.int_case("hole", 5, 50, 12, 9)
    pairs = test[:, :2]
    sc = RR.int_relation_scores("hole", E, R, pairs)
    ids, val = RR.exact_relation_topk("hole", E, R, pairs, 20)
    assert (ids[:, 12:] == -1).all() and np.isneginf(val[:, 12:]).all()
    for i in range(len(pairs)):
        assert sorted(ids[i, :12].tolist()) == list(range(12))
        assert (val[i, :12] == sc[i, ids[i, :12]]).all()
        s0, s1, e0, e1 = val[i, :11], val[i, 1:12], ids[i, :11], ids[i, 1:12]
        assert ((s0 > s1) | ((s0 == s1) & (e0 < e1))).all()
    excl = RR.pair_relations(pairs, known)
    ids2, _ = RR.exact_relation_topk("hole", E, R, pairs, 20, excl)
    for i, ex in enumerate(excl):
        assert len(ex) >= 1 and not set(ids2[i].tolist()) & set(ex.tolist())
        assert (ids2[i] >= 0).sum() == 12 - len(ex)


# ----------------------------------------------------------------------------
# the C ABI, without a GPU
# ----------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "skge_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(skge_[a-z0-9_]+)\s*\(", src))
    from skge_amd import _lib as L
    lib = L.load()
    for f in NEW:
        assert f in declared and f in L.SIGNATURES and hasattr(lib, f), f
    assert lib.skge_abi_version() == 2


def test_bad_arguments_are_refused_without_a_gpu():
    import ctypes
    from skge_amd import _lib as L
    lib = L.load()
    rc = lib.skge_relrank(None, 0, None, None, 5, 3, 8, None, 1, None, None, None, 0, None)
    assert rc == -1 and b"NULL" in lib.skge_last_error()
    rc = lib.skge_reltopk(None, 0, None, None, 5, 3, 8, None, 1, 10, None, None, None, 0, None,
                          None)
    assert rc == -1 and b"NULL" in lib.skge_last_error()
    # non-NULL host pointers: refused on sizes before anything touches the device
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for model, N, M, d, nq in ((0, 5, 3, 1025, 1), (0, 5, 0, 8, 1), (7, 5, 3, 8, 1), (0, 5, 3, 8, -1)):
        assert lib.skge_relrank(None, model, p, p, N, M, d, p, nq, None, None, p, 1 << 20, p) == -1
        assert lib.skge_last_error()
        assert lib.skge_reltopk(None, model, p, p, N, M, d, p, nq, 10, None, None, p, 1 << 20, p,
                                p) == -1
    for k in (0, 129):
        assert lib.skge_reltopk(None, 0, p, p, 5, 3, 8, p, 1, k, None, None, p, 1 << 20, p, p) == -1
        assert b"k =" in lib.skge_last_error()
    # a workspace that is too small, and a filter with no id array
    assert lib.skge_relrank(None, 0, p, p, 5, 3, 8, p, 1, None, None, p, 8, p) == -1
    assert b"workspace" in lib.skge_last_error()
    assert lib.skge_relrank(None, 0, p, p, 5, 3, 8, p, 1, p, None, p, 1 << 20, p) == -1
    assert lib.skge_reltopk(None, 0, p, p, 5, 3, 8, p, 1, 5, p, None, p, 1 << 20, p, p) == -1
    # nq == 0 is legal and launches nothing
    assert lib.skge_relrank(None, 0, p, p, 5, 3, 8, p, 0, None, None, None, 0, p) == 0
    assert lib.skge_reltopk(None, 3, p, p, 5, 3, 8, p, 0, 5, None, None, None, 0, p, p) == 0
    # the workspace functions: positive, and RESCAL's is its score matrix
    assert lib.skge_relrank_workspace_bytes(100, 8, 5, L.SKGE_RESCAL) >= 100 * 5 * 4
    assert lib.skge_relrank_workspace_bytes(100, 8, 5, L.SKGE_HOLE) >= 100 * 8 * 4 + 100 * 8
    assert lib.skge_reltopk_workspace_bytes(100, 8, 10, 5, L.SKGE_TRANSE_L1) >= 100 * 8 * 4
    assert lib.skge_reltopk_workspace_bytes(100, 8, 129, 5, L.SKGE_TRANSE_L1) == 0
