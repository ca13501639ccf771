"""CPU checks of tests/pool_ref.py (the references of tests/test_gpu_pools.py),
of the pool entry points' ABI and of the Python host checks on pools."""
import functools
import os
import re

import numpy as np
import pytest

import eval_ref as X
import pool_ref as PR
import topk_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["skge_rank_pools_workspace_bytes", "skge_rank_pools", "skge_topk_pools_workspace_bytes",
       "skge_topk_pools"]
# the large cases are scored once, on the GPU test's side; here the small ones
SMALL = [c for c in PR.INT_CASES if c[3] * c[4] <= 40000 and c[2] <= 130]


@functools.lru_cache(maxsize=None)
def _int(model, kind, d, N, nq):
    E, R, test, known, pools, vp = PR.int_case(model, kind, d, N, nq)
    return E, R, test, known, pools, vp, PR.exact_pool_ranks(model, E, R, test, known, pools, vp)


@functools.lru_cache(maxsize=None)
def _float(model, d, scale):
    E, R, test, known, pools, vp = PR.float_case(model, d, scale)
    return E, R, test, known, pools, vp, PR.pool_rank_envelope(model, E, R, test, known, pools, vp)


# ----------------------------------------------------------------------------
# the reference against eval_ref
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("model,kind,d,N,nq", [c for c in SMALL if c[1] != "big"])
def test_pool_minus_one_and_full_pool_equal_exact_ranks(model, kind, d, N, nq):
    E, R, test, known = _int(model, kind, d, N, nq)[:4]
    want = X.exact_ranks(model, E, R, test, known)
    nv = 2 * len(test)
    got = PR.exact_pool_ranks(model, E, R, test, known, [], np.full(nv, -1))
    np.testing.assert_array_equal(got, want)
    got = PR.exact_pool_ranks(model, E, R, test, known, [np.arange(3), np.arange(N)],
                              np.ones(nv, dtype=np.int64))
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("model,kind,d,N,nq", [c for c in SMALL if c[4] <= 40])
def test_envelope_contains_the_exact_ranks(model, kind, d, N, nq):
    E, R, test, known, pools, vp, exact = _int(model, kind, d, N, nq)
    lo, hi = PR.pool_rank_envelope(model, E, R, test, known, pools, vp)
    assert (lo <= exact).all() and (exact <= hi).all()


def test_empty_pool_gives_rank_one_and_true_entity_outside_adds_nothing():
    E, R, test, known = X.make_int_case("hole", 5, 40, 12, 3)
    pools = [np.zeros(0, dtype=np.int64), np.arange(40), np.setdiff1d(np.arange(40), test[:, :2])]
    nv = 2 * len(test)
    assert (PR.exact_pool_ranks("hole", E, R, test, known, pools, np.zeros(nv)) == 1).all()
    full = PR.exact_pool_ranks("hole", E, R, test, known, pools, np.full(nv, 1))
    # pool 2 is everything but the test triples' own entities: the ranks lose
    # exactly those entities that score above
    less = PR.exact_pool_ranks("hole", E, R, test, known, pools, np.full(nv, 2))
    assert (less <= full).all() and (less < full).any()


# ----------------------------------------------------------------------------
# the conditions the inputs must meet, by the reference alone
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("model,d,scale", PR.FLOAT_CASES)
def test_float_cases_pin_most_ranks(model, d, scale):
    """Not vacuous: at least 0.9 of the envelope entries have hi == lo, and no
    width exceeds 2."""
    lo, hi = _float(model, d, scale)[6]
    assert (lo <= hi).all()
    assert (lo == hi).mean() >= 0.9, (lo == hi).mean()
    assert (hi - lo).max() <= 2, (hi - lo).max()


@pytest.mark.parametrize("model,d,scale", PR.FLOAT_CASES)
def test_float_cases_pools_filter_and_membership_matter(model, d, scale):
    E, R, test, known, pools, vp, (lo, hi) = _float(model, d, scale)
    ulo, uhi = X.rank_envelope(model, E, R, test, known)
    assert (hi[:, 0::2] < ulo[:, 0::2]).any()          # typed < untyped, certainly
    assert (hi[:, 1::2] < lo[:, 0::2]).any()           # the filter moves a rank, certainly
    # without the membership test some filtered rank would leave the envelope:
    # the all-entity decrement exceeds what the pool allows
    dec_all = ulo[:, 0::2] - uhi[:, 1::2]              # known answers certainly above, all
    dec_max = hi[:, 0::2] - lo[:, 1::2]                # at most this many are pool members
    assert (dec_all > dec_max).any()


@pytest.mark.parametrize("model,kind,d,N,nq",
                         [c for c in PR.INT_CASES if c[1] in PR.RESTRICTING and c[3] >= 63])
def test_int_cases_pool_moves_ranks(model, kind, d, N, nq):
    """On every case whose pools hold fewer than all entities the pool moves
    some rank (typed < untyped); from 16 queries up the filter moves one too;
    and on the hand-made pools some known answer OUTSIDE its vector's pool
    scores above the true entity, so a library that subtracts without the
    membership test fails."""
    E, R, test, known, pools, vp, exact = _int(model, kind, d, N, nq)
    untyped = PR.exact_pool_ranks(model, E, R, test, known, [], np.full(2 * nq, -1))
    assert (exact <= untyped).all() and (exact < untyped).any()
    assert (exact >= 1).all() and (exact[:, 1::2] <= exact[:, 0::2]).all()
    if nq >= 16 and kind != "many":
        assert (exact[:, 0::2] != exact[:, 1::2]).any()
    if kind in PR.HAND_MADE and nq >= 16:
        assert PR.known_above_outside(model, E, R, test, known, pools, vp) > 0


def test_case_tables_cover_the_edges():
    ds = {c[2] for c in PR.INT_CASES}
    assert {1, 3, 31, 32, 33, 65, 1024} <= ds
    kinds = {c[1] for c in PR.INT_CASES}
    assert kinds == {"typed", "sizes", "mixed", "groups", "big", "many", "all", "full"}
    assert {c[4] for c in PR.INT_CASES} >= {1}
    E, R, test, known, pools, vp = PR.int_case("transe", "sizes", 3, 300, 64)
    assert tuple(len(p) for p in pools) == PR.POOL_SIZES
    assert len(set(pools[4].tolist()) & set(pools[7].tolist())) > 0        # pools overlap
    true = np.asarray(test)[:, [1, 0]].reshape(-1)
    outside = [t not in set(pools[g].tolist()) for g, t in zip(vp.tolist(), true.tolist())]
    assert any(outside)                                                   # a true entity outside
    E, R, test, known, pools, vp = PR.int_case("transe", "groups", 65, 300, 97)
    counts = np.bincount(vp + 1)
    assert counts.tolist() == [1, 1, 63, 64, 65]
    assert (np.diff(vp) != 0).sum() > 50                                  # shuffled
    E, R, test, known, pools, vp = PR.int_case("transe", "big", 8, 5000, 2048)
    assert len(pools) == 1 and len(pools[0]) == 4500
    E, R, test, known, pools, vp = PR.int_case("transe", "many", 4, 130, 5)
    assert len(pools) == 200 > len(vp)
    E, R, test, known, pools, vp = PR.int_case("transe", "mixed", 33, 130, 33)
    assert (vp == -1).any() and (vp >= 0).any()


def test_topk_reference_selects_pool_members_only():
    E, R, test, known, pools, vp = PR.int_case("hole", "sizes", 3, 300, 64)
    for direction in T.DIRECTIONS:
        q = np.asarray(test)[:, [0, 2]] if direction == "tail" else np.asarray(test)[:, [1, 2]]
        qp = PR.topk_query_pool("sizes", vp, direction)
        excl = T.known_answers(q, known, direction)
        ids, val = PR.exact_pool_topk("hole", E, R, q, direction, 70, excl, pools, qp)
        sc = T.int_query_scores("hole", E, R, q, direction)
        for i, g in enumerate(qp.tolist()):
            got = ids[i][ids[i] >= 0]
            want = np.setdiff1d(pools[g], excl[i])
            assert len(got) == min(70, len(want)) and set(got.tolist()) <= set(want.tolist())
            assert (ids[i, len(got):] == -1).all() and np.isneginf(val[i, len(got):]).all()
            assert (val[i, :len(got)] == sc[i, got]).all()
            s, e = val[i, :len(got)], got
            assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (e[:-1] < e[1:]))).all()
    qp = PR.topk_query_pool("groups", np.zeros((97, 2), dtype=np.int64), "tail")
    assert np.bincount(qp + 1).tolist() == [0, 1, 31, 32, 33]


# ----------------------------------------------------------------------------
# the C ABI, without a GPU
# ----------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "skge_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(skge_[a-z0-9_]+)\s*\(", body))
    from skge_amd import _lib as L
    lib = L.load()
    for f in NEW:
        assert f in declared and f in L.SIGNATURES and hasattr(lib, f), f
    assert len(L.SIGNATURES["skge_rank_pools"][1]) == 19
    assert len(L.SIGNATURES["skge_topk_pools"][1]) == 20
    text = " ".join(src[src.index("candidate pools"):].replace("*", " ").lower().split())
    assert "not range-checked" in text          # the header says so
    assert lib.skge_abi_version() == 2


def test_bad_arguments_are_refused_without_a_gpu():
    import ctypes
    from skge_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 24

    def rank(model=0, N=5, d=8, nq=1, off=p, ent=p, n_pools=2, vp=p, E=p, ws=p, nb=big, out=p):
        return lib.skge_rank_pools(None, model, E, p, N, d, p, nq, off, ent, n_pools, vp, p, p, p,
                                   p, ws, nb, out)

    def topk(model=0, N=5, d=8, nq=1, k=5, off=p, ent=p, n_pools=2, qp=p, E=p, ws=p, nb=big,
             direction=0, xoff=None, xent=None):
        return lib.skge_topk_pools(None, model, E, p, N, d, p, nq, direction, k, off, ent, n_pools,
                                   qp, xoff, xent, ws, nb, p, p)

    for fn in (rank, topk):
        for kw, word in (({"E": None}, b"NULL"), ({"model": 4}, b"model"), ({"model": -1}, b"model"),
                         ({"d": 1025}, b"1024"), ({"n_pools": -1}, b"n_pools"),
                         ({"off": None}, b"NULL"), ({"ent": None}, b"NULL"),
                         ({"nb": 8}, b"workspace"), ({"ws": None}, b"workspace"),
                         ({"nq": -1}, b"sizes"), ({"N": 0}, b"sizes")):
            assert fn(**kw) == -1, kw
            assert word in lib.skge_last_error(), (kw, lib.skge_last_error())
    assert rank(vp=None) == -1 and b"NULL" in lib.skge_last_error()
    assert rank(out=None) == -1 and b"NULL" in lib.skge_last_error()
    assert topk(qp=None) == -1 and b"NULL" in lib.skge_last_error()
    assert topk(direction=2) == -1 and b"direction" in lib.skge_last_error()
    assert topk(xoff=p) == -1 and b"excl_ent" in lib.skge_last_error()
    for k in (0, 129):
        assert topk(k=k) == -1 and b"k =" in lib.skge_last_error()
    # nq == 0 is legal and launches nothing; no pools at all is legal
    assert rank(nq=0, ws=None, nb=0) == 0
    assert topk(nq=0, ws=None, nb=0) == 0
    assert rank(nq=0, n_pools=0, off=None, ent=None, ws=None, nb=0) == 0
    # the workspace functions
    assert lib.skge_rank_pools_workspace_bytes(100, 8, 6) >= 200 * 8 * 4 + 200 * 12 + 200 * 4
    assert lib.skge_rank_pools_workspace_bytes(100, 8, 6) >= lib.skge_rank_known_workspace_bytes(100, 8)
    assert lib.skge_rank_pools_workspace_bytes(100, 8, -1) == 0
    assert lib.skge_topk_pools_workspace_bytes(100, 8, 10, 50, 6) >= 100 * 8 * 4 + 100 * 10 * 8
    assert lib.skge_topk_pools_workspace_bytes(100, 8, 129, 50, 6) == 0
    assert (lib.skge_rank_pools_workspace_bytes(100, 8, 100000) >
            lib.skge_rank_pools_workspace_bytes(100, 8, 6) + 100000 * 4 - 1024)


# ----------------------------------------------------------------------------
# the Python host checks, without a GPU
# ----------------------------------------------------------------------------

def test_pool_csr_sorts_lists_and_checks_arrays():
    import skge_amd as S
    off, ent = S.pool_csr([[5, 1, 5, 3], (), np.array([0, 2, 9]), {7}], 10)
    assert off.dtype == np.int64 and ent.dtype == np.int32
    assert off.tolist() == [0, 3, 3, 6, 7] and ent.tolist() == [1, 3, 5, 0, 2, 9, 7]
    off2, ent2 = S.pool_csr((off, ent), 10)                 # a CSR passes through
    assert off2.tolist() == off.tolist() and ent2.tolist() == ent.tolist()
    assert S.pool_csr([], 10)[0].tolist() == [0]
    with pytest.raises(ValueError, match=r"pool 1 holds id 10, out of range for 10"):
        S.pool_csr([[1], [3, 10]], 10)
    with pytest.raises(ValueError, match=r"pool 0 holds id -1"):
        S.pool_csr([np.array([-1, 2])], 10)
    with pytest.raises(ValueError, match=r"pool 2 is not ascending and unique \(id 2 after 4\)"):
        S.pool_csr([[1], [2], np.array([4, 2])], 10)
    with pytest.raises(ValueError, match=r"pool 0 is not ascending and unique \(id 4 after 4\)"):
        S.pool_csr([np.array([4, 4])], 10)
    with pytest.raises(ValueError, match="not a CSR"):
        S.pool_csr((np.array([0, 3]), np.array([1, 2])), 10)
    # adjacent pools may repeat or step down across their boundary
    assert S.pool_csr([np.array([4, 6]), np.array([1, 6])], 10)[1].tolist() == [4, 6, 1, 6]
    from skge_amd.eval import check_pool_ids
    assert check_pool_ids([-1, 0, 2], 3, "x").dtype == np.int32
    with pytest.raises(ValueError, match=r"tail_pool: entry 1 names pool 3, outside -1 \.\. 2"):
        check_pool_ids([0, 3], 3, "tail_pool")
    with pytest.raises(ValueError, match="names pool -2"):
        check_pool_ids([-2], 3, "head_pool")


def test_typed_pools_map_tail_to_range_and_head_to_domain():
    import skge_amd as S
    rs = np.random.RandomState(4)
    test, known = X.random_triples(rs, 50, 4, 30)
    ev = S.FilteredRankingEval(test, known)
    pools, tp, hp = ev.typed_pools(4)
    want = PR.type_pools_of(known, 4)
    assert len(pools) == 8
    for a, b in zip(pools, want):
        assert a.tolist() == b.tolist()
    order = X.eval_order(test)
    assert tp.tolist() == (2 * order[:, 2] + 1).tolist() and hp.tolist() == (2 * order[:, 2]).tolist()
    np.testing.assert_array_equal(np.stack([tp, hp], axis=1).reshape(-1), PR.typed_vec_pool(order))
    for (s, o, p), t, h in zip(order.tolist(), tp.tolist(), hp.tolist()):
        assert o in pools[t].tolist() and s in pools[h].tolist()      # the test triples are known
    # a type_index dict and a triple array give the index of those triples
    train = known[::2]
    for types in (S.type_index(train.tolist()), train):
        got = ev.typed_pools(4, types)[0]
        for a, b in zip(got, PR.type_pools_of(train, 4)):
            assert a.tolist() == b.tolist()
    # DeviceKG.pools' layout (device.py): the same lists as a CSR
    off, ent = S.pool_csr(pools, 50)
    kn = np.asarray(known, dtype=np.int64)
    keys = np.unique(np.concatenate([(2 * kn[:, 2]) * 50 + kn[:, 0],
                                     (2 * kn[:, 2] + 1) * 50 + kn[:, 1]]))
    assert off.tolist() == np.searchsorted(keys, np.arange(9) * 50).tolist()
    assert ent.tolist() == (keys % 50).tolist()
    with pytest.raises(ValueError, match="relation 3 is out of range for 3"):
        ev.typed_pools(3)
