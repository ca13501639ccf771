"""Device nearest neighbours (skge_neighbours through skge_amd.Neighbours)
against the references of tests/neighbours_ref.py:

(a) integer tables, where every sum is below 2^24 and the contract's fp32
    arithmetic is reproduced exactly on the host, so ids and values must EQUAL
    exact_neighbours -- both metrics, the three query forms, at the edges of
    the kernels (d = 1, the scalar tail, the 32-dim chunk boundary, many
    chunks; N around the 32-row MFMA tile and the 128-row LDS tile, N = 1,
    several slices; query counts ragged against the query block) and for k on
    both sides of the 16 / 32 / 128 list layouts and above N - 1;
(b) ties, a zero row, repeated query rows and self-exclusion, by construction;
(c) float tables, inside neighbours_envelope's derived fp32 bounds;
(d) every-row mode against rows = arange(N), bit for bit;
(e) the facade.
"""
import functools
import os

import numpy as np
import pytest
import torch

import neighbours_ref as NR

pytestmark = pytest.mark.gpu

# (N, d, nq of the rows / query forms)
CASES_A = [(300, 1, 97), (129, 3, 33), (31, 31, 31), (32, 32, 33), (33, 33, 97), (127, 65, 31),
           (128, 200, 33), (1, 33, 31), (2, 3, 33), (129, 1024, 31), (4500, 8, 97)]
KS = (1, 2, 10, 64, 128)
FORMS = ("all", "rows", "query")


@functools.lru_cache(maxsize=None)
def _carrier():
    """A tiny model: the device an array table is put on."""
    import skge_amd as S
    return S.TransE((4, 4, 2), 4, init="device_nunif")


def _nn(table, metric):
    import skge_amd as S
    return S.Neighbours(_carrier(), table=np.asarray(table, dtype=np.float32), metric=metric)


def _ask(nn, form, kw, k):
    if form == "query":
        ids, sims = nn.query(kw["vectors"], k=k)
        n = len(kw["vectors"])
    else:
        ids, sims = nn.topk(k=k, **kw)
        n = len(kw["rows"]) if "rows" in kw else nn._table().shape[0]
    assert ids.dtype == np.int64 and sims.dtype == np.float32
    assert ids.shape == sims.shape == (n, k)
    return ids, sims


def _assert_equal(got, want, msg):
    np.testing.assert_array_equal(got[0], want[0], err_msg="ids, " + msg)
    np.testing.assert_array_equal(got[1].astype(np.float64), want[1], err_msg="values, " + msg)


# ---------------------------------------------------------------------------
# (a) exact equality on integer tables
# ---------------------------------------------------------------------------

def _ks(N):
    return KS + ((N,) if N <= 128 else ())          # k = N > N - 1 pads


@functools.lru_cache(maxsize=None)
def _int_case(N, d, nq):
    rs = np.random.RandomState(1000 * d + N)
    tab = NR.make_int_table(N, d, 7 * N + d)
    rows = rs.randint(N, size=nq)
    vec = rs.randint(-3, 4, size=(nq, d)).astype(np.float64)
    vec[0] = tab[N - 1]
    tab.setflags(write=False)
    return tab, {"all": {}, "rows": {"rows": rows}, "query": {"vectors": vec}}


@functools.lru_cache(maxsize=None)
def _int_ref(N, d, nq, metric, form):
    """The reference's full order up to the largest k asked: every smaller
    k's result is its first k columns, padding included."""
    tab, forms = _int_case(N, d, nq)
    ids, val = NR.exact_neighbours(tab, metric, max(_ks(N)), **forms[form])
    ids.setflags(write=False)
    val.setflags(write=False)
    return ids, val


@pytest.mark.parametrize("N,d,nq", CASES_A)
@pytest.mark.parametrize("metric", NR.METRICS)
def test_int_tables_exact(metric, N, d, nq):
    tab, forms = _int_case(N, d, nq)
    nn = _nn(tab, metric)
    for form in FORMS:
        ids, val = _int_ref(N, d, nq, metric, form)
        for k in _ks(N):
            got = _ask(nn, form, forms[form], k)
            _assert_equal(got, (ids[:, :k], val[:, :k]), "%s k=%d" % (form, k))
        if form != "query":
            assert (ids[:, N - 1:] == -1).all() and (ids[:, :N - 1] >= 0).all()   # self is out
    if d >= 31 and N >= 31:
        c, dd = _int_ref(N, d, nq, "cosine", "all"), _int_ref(N, d, nq, "dot", "all")
        assert (c[0] != dd[0]).any()     # the two metrics order differently


# ---------------------------------------------------------------------------
# (b) ties, a zero row, repeated rows, self-exclusion: by construction
# ---------------------------------------------------------------------------
N_B, D_B = 300, 5


def _table_b(seed):
    return NR.make_int_table(N_B, D_B, seed)


@pytest.mark.parametrize("metric", NR.METRICS)
def test_duplicate_rows_come_in_id_order(metric):
    """Copies of one row sit in every 128-row tile (and, with 300 queries of
    k = 10, in different slices): equal values meet inside a tile, across
    tiles and across slices, and come back in ascending id."""
    tab = _table_b(31)
    copies = [3, 120, 127, 128, 200, 255, 256, 299]
    tab[copies] = 3 * np.abs(tab[3]) + 1          # long, so that its copies are each other's best
    nn = _nn(tab, metric)
    for k in (10, 64):
        ids, sims = _ask(nn, "rows", {"rows": np.array(copies)}, k)
        _assert_equal((ids, sims), NR.exact_neighbours(tab, metric, k, rows=copies), "k=%d" % k)
        if metric == "cosine":
            for i, c in enumerate(copies):
                others = [x for x in copies if x != c]
                assert ids[i, :7].tolist() == others
                assert len(set(sims[i, :7].tolist())) == 1
    ids, sims = _ask(nn, "all", {}, 10)
    _assert_equal((ids, sims), NR.exact_neighbours(tab, metric, 10), "all rows")
    # identical table: every row's neighbours are the lowest other ids
    tab[:] = tab[0]
    ids, sims = _ask(_nn(tab, metric), "all", {}, 5)
    for i in (0, 2, 4, 5, 299):
        assert ids[i].tolist() == [x for x in range(6) if x != i][:5]
    assert (sims == sims[0, 0]).all()


def test_zero_rows_have_cosine_zero_and_keep_the_id_order():
    tab = _table_b(32)
    tab[[7, 130]] = 0.0
    nn = _nn(tab, "cosine")
    # a zero query: cosine 0 with everything, the lowest other ids
    ids, sims = _ask(nn, "rows", {"rows": [7, 130]}, 6)
    assert ids[0].tolist() == [0, 1, 2, 3, 4, 5] and ids[1].tolist() == [0, 1, 2, 3, 4, 5]
    assert (sims == 0.0).all()
    ids, sims = _ask(nn, "query", {"vectors": np.zeros((1, D_B))}, 3)
    assert ids[0].tolist() == [0, 1, 2] and (sims == 0.0).all()
    # a zero row among the candidates scores exactly 0, between the positives and the negatives
    k = 128
    got = _ask(nn, "all", {}, k)
    want = NR.exact_neighbours(tab, "cosine", k)
    _assert_equal(got, want, "all rows")
    hit = (got[0] == 7) | (got[0] == 130)
    assert hit.any() and (got[1][hit] == 0.0).all()


@pytest.mark.parametrize("metric", NR.METRICS)
def test_repeated_rows_and_self_exclusion(metric):
    tab = _table_b(33)
    nn = _nn(tab, metric)
    rows = np.array([3, 17, 3, 299, 17, 3])
    ids, sims = _ask(nn, "rows", {"rows": rows}, 10)
    for i, j in ((0, 2), (0, 5), (1, 4)):
        assert (ids[i] == ids[j]).all() and (sims[i] == sims[j]).all()
    _assert_equal((ids, sims), NR.exact_neighbours(tab, metric, 10, rows=rows), "rows")
    assert not (ids == rows[:, None]).any()
    # every-row mode: no row is its own neighbour, even at k = N - 1
    ids, _ = _ask(nn, "all", {}, 128)
    assert not (ids == np.arange(N_B)[:, None]).any()
    small = tab[:40]
    ids, sims = _ask(_nn(small, metric), "all", {}, 40)
    assert (ids[:, 39] == -1).all() and np.isneginf(sims[:, 39]).all()
    for i in range(40):
        assert sorted(ids[i, :39].tolist()) == [x for x in range(40) if x != i]
    # query mode excludes nothing: a vector equal to a row finds that row
    ids, sims = _ask(nn, "query", {"vectors": tab[[3, 299]]}, 10)
    _assert_equal((ids, sims), NR.exact_neighbours(tab, metric, 10, vectors=tab[[3, 299]]), "query")
    if metric == "cosine":
        assert ids[0, 0] == 3 and ids[1, 0] == 299


# ---------------------------------------------------------------------------
# (c) float tables inside the derived fp32 envelope
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _float_ref(N, d, seed, metric, k):
    tab = NR.make_float_table(N, d, seed)
    forms = NR.float_query_forms(tab, seed)
    return tab, forms, {f: NR.neighbours_envelope(tab, metric, k, **kw) for f, kw in forms.items()}


@pytest.mark.parametrize("k", NR.FLOAT_KS)
@pytest.mark.parametrize("N,d,seed", NR.FLOAT_CASES)
@pytest.mark.parametrize("metric", NR.METRICS)
def test_float_tables_inside_envelope(metric, N, d, seed, k):
    """Every forced row is returned, every returned row is allowed, every
    returned value is within its pair's bound of the fp64 value, and the rows
    follow the contract's order on the returned values.  The forced rows are
    nearly all of the result (test_neighbours_ref.py shows it on the CPU)."""
    tab, forms, env = _float_ref(N, d, seed, metric, k)
    nn = _nn(tab, metric)
    for form in FORMS:
        sc, tau, forced, allowed, excl = env[form]
        ids, sims = _ask(nn, form, forms[form], k)
        assert (ids >= 0).all()
        rows = np.arange(len(sc))[:, None]
        got = np.zeros_like(forced)
        got[rows, ids] = True
        assert (got.sum(axis=1) == k).all()      # distinct ids
        err = np.abs(sims.astype(np.float64) - sc[rows, ids])
        print("%s d=%d k=%d %s: forced %d of %d, max err / tau %.3f"
              % (metric, d, k, form, forced.sum(), got.sum(), (err / tau[rows, ids]).max()))
        assert not (forced & ~got).any(), np.argwhere(forced & ~got)[:5].tolist()
        assert not (got & ~allowed).any(), np.argwhere(got & ~allowed)[:5].tolist()
        assert (err <= tau[rows, ids]).all()
        s0, s1, e0, e1 = sims[:, :-1], sims[:, 1:], ids[:, :-1], ids[:, 1:]
        assert ((s0 > s1) | ((s0 == s1) & (e0 < e1))).all()
        if excl is not None:
            assert not (ids == np.array([e[0] for e in excl])[:, None]).any()
        assert forced.sum() >= 0.98 * got.sum()


# ---------------------------------------------------------------------------
# (d) every-row mode against rows = arange(N)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("metric", NR.METRICS)
def test_all_rows_equals_rows_arange(metric):
    N, d, seed = NR.FLOAT_CASES[1]
    nn = _nn(NR.make_float_table(N, d, seed), metric)
    for k in (10, 20, 100):
        a = nn.topk(k=k)
        b = nn.topk(k=k, rows=np.arange(N))
        assert (a[0] == b[0]).all()
        assert a[1].tobytes() == b[1].tobytes()


# ---------------------------------------------------------------------------
# (e) the facade
# ---------------------------------------------------------------------------

def _model(cls, N, M, d, seed):
    np.random.seed(seed)
    return cls((N, N, M), d)


def test_facade_tables_of_a_model():
    import skge_amd as S
    m = _model(S.TransE, 60, 7, 12, 5)
    E, R = np.asarray(m.params["E"]), np.asarray(m.params["R"])
    for table, tab in (("E", E), ("R", R)):
        nn = S.Neighbours(m, table=table) if table != "E" else S.Neighbours(m)
        ids, sims = nn.topk(k=4)
        assert ids.shape == sims.shape == (len(tab), 4)
        assert ids.dtype == np.int64 and sims.dtype == np.float32
        sc, tau, forced, allowed, _ = NR.neighbours_envelope(tab, "cosine", 4)
        rows = np.arange(len(tab))[:, None]
        got = np.zeros_like(forced)
        got[rows, ids] = True
        assert not (forced & ~got).any() and not (got & ~allowed).any()
        assert (np.abs(sims - sc[rows, ids]) <= tau[rows, ids]).all()
    # default k = 10; one vector is one query; metric="dot"
    ids, sims = S.Neighbours(m, metric="dot").query(E[5])
    assert ids.shape == (1, 10)
    sc, tau, forced, allowed, _ = NR.neighbours_envelope(E, "dot", 10, vectors=E[5:6])
    assert not (forced[0] & ~np.isin(np.arange(60), ids[0])).any() and allowed[0, ids[0]].all()
    # the table is read at each call
    nn = S.Neighbours(m)
    m.params["E"].data[1] = m.params["E"].data[0] * 2
    after = nn.topk(k=3, rows=[0])
    assert after[0][0, 0] == 1 and abs(after[1][0, 0] - 1.0) < 1e-6


def test_facade_rescal_w_is_viewed_as_m_by_d_squared():
    import skge_amd as S
    m = _model(S.RESCAL, 30, 9, 6, 6)
    W = np.asarray(m.params["W"])
    assert W.shape == (9, 6, 6)
    ids, sims = S.Neighbours(m, table="R").topk(k=3)
    assert ids.shape == (9, 3)
    flat = W.reshape(9, 36)
    sc, tau, forced, allowed, _ = NR.neighbours_envelope(flat, "cosine", 3)
    rows = np.arange(9)[:, None]
    got = np.zeros_like(forced)
    got[rows, ids] = True
    assert not (forced & ~got).any() and not (got & ~allowed).any()
    assert (np.abs(sims - sc[rows, ids]) <= tau[rows, ids]).all()


def test_facade_subgraph_embeddings_as_the_table():
    import skge_amd as S
    rs = np.random.RandomState(8)
    trip = sorted({(int(rs.randint(10)), int(rs.randint(50)), int(rs.randint(3)))
                   for _ in range(150)})
    m = _model(S.TransE, 50, 3, 16, 7)
    SA, _ = S.Subgraphs.from_triples(trip, 1).embed(m)
    assert torch.is_tensor(SA) and SA.is_cuda and SA.shape[0] > 5
    ids, sims = S.Neighbours(m, table=SA).topk(k=5)
    tab = SA.cpu().numpy()
    sc, tau, forced, allowed, _ = NR.neighbours_envelope(tab, "cosine", 5)
    rows = np.arange(len(tab))[:, None]
    got = np.zeros_like(forced)
    got[rows, ids] = True
    assert not (forced & ~got).any() and not (got & ~allowed).any()
    assert (np.abs(sims - sc[rows, ids]) <= tau[rows, ids]).all()


def test_golden_table_top5_against_costheta():
    """The reference's own cosTheta values (tools/gen_golden_neighbours.py)
    bound the device's top-5 of the fixture's table, and shared_role tags the
    neighbours with the fixture's relation."""
    import skge_amd as S
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "neighbours",
                             "neighbours_ref.npz"))
    tab, cos = z["T"], z["cos"]
    _, tau, excl = NR.float_scores(tab, "cosine")
    forced, allowed = NR.envelope_of(cos, tau, 5, excl)
    ids, sims = _ask(_nn(tab, "cosine"), "all", {}, 5)
    rows = np.arange(40)[:, None]
    got = np.zeros_like(forced)
    got[rows, ids] = True
    assert not (forced & ~got).any() and not (got & ~allowed).any()
    assert (np.abs(sims - cos[rows, ids]) <= tau[rows, ids]).all()
    assert ids[4, 0] == 17 and ids[17, 0] == 4          # row 17 is twice row 4
    for name in ("train", "test"):
        np.testing.assert_array_equal(S.shared_role(ids, z[name]), z["role_" + name][rows, ids])
