"""CPU checks for nearest neighbours in embedding space: the references of
tests/neighbours_ref.py against the fixture made by the reference's own
eval-embeddings.py (tools/gen_golden_neighbours.py), skge_amd.shared_role
against its tag matrices, the fp32 bound on the GPU tests' float cases, and
the argument errors of skge_neighbours and of the facade (no GPU needed)."""
import os
import types

import numpy as np
import pytest

import neighbours_ref as NR
import topk_ref as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "neighbours",
                      "neighbours_ref.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def test_fp64_cosines_match_costheta(golden):
    cos = NR.cosines64(golden["T"])
    assert cos.shape == golden["cos"].shape == (40, 40)
    assert np.abs(cos - golden["cos"]).max() <= 1e-12
    # the fixture's values are cosTheta's, not cosineMatrix's integer truncation
    assert (np.abs(golden["cos"]) % 1 != 0).sum() > 1500
    sc, tau, _ = NR.float_scores(golden["T"], "cosine")
    assert np.abs(sc - golden["cos"]).max() <= 1e-12
    assert tau.max() < 1e-5


def test_role_matrix_matches_the_reference_graphs(golden):
    for name in ("train", "test"):
        want = golden["role_" + name]
        np.testing.assert_array_equal(NR.shared_role_matrix(golden[name], 40), want)


def test_shared_role_matches_the_golden_tags(golden):
    from skge_amd.neighbours import shared_role
    N = 40
    ids = np.tile(np.arange(N), (N, 1))            # every entity as everyone's "neighbour"
    for name in ("train", "test"):
        want = golden["role_" + name]
        np.testing.assert_array_equal(shared_role(ids, golden[name]), want)
        np.testing.assert_array_equal(shared_role(ids, [tuple(t) for t in golden[name].tolist()]),
                                      want)
        rows = np.array([5, 0, 39, 5, 17])
        got = shared_role(ids[rows][:, ::-1], golden[name], rows=rows)
        np.testing.assert_array_equal(got, want[rows][:, ::-1])
    # the ENTITY ID is tested, not the rank index: permuted columns follow the ids
    perm = np.random.RandomState(3).permutation(N)
    np.testing.assert_array_equal(shared_role(ids[:, perm], golden["train"]),
                                  golden["role_train"][:, perm])
    # padding
    pad = np.full((N, 3), -1, dtype=np.int64)
    assert not shared_role(pad, golden["train"]).any()
    mixed = np.stack([ids[:, 0], pad[:, 0]], axis=1)
    np.testing.assert_array_equal(shared_role(mixed, golden["train"]),
                                  np.stack([golden["role_train"][:, 0], np.zeros(N, bool)], axis=1))
    assert shared_role(np.zeros((0, 4), dtype=np.int64), golden["train"]).shape == (0, 4)
    with pytest.raises(ValueError):
        shared_role(ids, golden["train"], rows=[1, 2])


def test_exact_reference_by_hand():
    # rows 0 and 2 equal, row 3 zero, row 1 orthogonal to row 0
    tab = np.array([[3, 4], [4, -3], [3, 4], [0, 0], [6, 8]], dtype=np.float64)
    ids, sims = NR.exact_neighbours(tab, "cosine", 4, rows=[0])
    r5, r10 = np.float32(1) / np.sqrt(np.float32(25)), np.float32(1) / np.sqrt(np.float32(100))
    assert ids.tolist() == [[2, 4, 1, 3]]
    assert sims[0, 0] == float((np.float32(25) * r5) * r5)
    assert sims[0, 1] == float((np.float32(50) * r5) * r10)
    assert sims[0, 2] == 0.0 and sims[0, 3] == 0.0      # orthogonal, zero row: by id
    ids, sims = NR.exact_neighbours(tab, "dot", 6, rows=[0])
    assert ids.tolist() == [[4, 2, 1, 3, -1, -1]]
    assert sims[0, :4].tolist() == [50.0, 25.0, 0.0, 0.0] and np.isneginf(sims[0, 4:]).all()
    ids, _ = NR.exact_neighbours(tab, "dot", 2, vectors=tab[:1])     # nothing excluded
    assert ids.tolist() == [[4, 0]]
    ids, _ = NR.exact_neighbours(tab, "dot", 1)                      # every row, self excluded
    assert ids[:, 0].tolist() == [4, 0, 4, 0, 0]


@pytest.mark.parametrize("N,d,seed", NR.FLOAT_CASES)
@pytest.mark.parametrize("metric", NR.METRICS)
def test_fp32_chain_is_inside_the_bound(N, d, seed, metric):
    """The contract's arithmetic restated in NumPy stays within tau of the
    fp64 value on every float case the GPU tests use, and the envelope built
    from tau pins nearly the whole result: it is not vacuous."""
    tab = NR.make_float_table(N, d, seed)
    for form, kw in NR.float_query_forms(tab, seed).items():
        got = NR.chain32(tab, metric, **kw).astype(np.float64)
        sc, tau, excl = NR.float_scores(tab, metric, **kw)
        err = np.abs(got - sc)
        print("%s d=%d %s: max err / tau %.3f, max tau %.3g" % (metric, d, form,
                                                                (err / tau).max(), tau.max()))
        assert (err <= tau).all()
        assert tau.max() < 2e-4 * max(1.0, np.abs(sc).max())
        for k in NR.FLOAT_KS:
            forced, allowed = NR.envelope_of(sc, tau, k, excl)
            ids, _ = T.topk_of_scores(got, k, excl)
            rows = np.arange(len(sc))[:, None]
            ret = np.zeros_like(forced)
            ret[rows, ids] = True
            assert not (forced & ~ret).any() and not (ret & ~allowed).any()
            assert forced.sum() >= 0.98 * ret.sum()


def test_argument_errors_are_reported_without_a_gpu():
    from skge_amd import _lib as L
    lib = L.load()
    one = np.zeros(64, dtype=np.float32)
    p = one.ctypes.data           # a host address: never dereferenced, nothing is launched

    def call(T=p, N=4, d=4, Q=None, rows=None, nq=4, metric=0, k=2, ws=p, nbytes=1 << 30,
             ids=p, sims=p):
        return lib.skge_neighbours(None, T, N, d, Q, rows, nq, metric, k, ws, nbytes, ids, sims)

    assert lib.skge_neighbours_workspace_bytes(4, 4, 4, 2) > 0
    assert lib.skge_neighbours_workspace_bytes(4, 4, 4, 129) == 0
    for kw, text in [(dict(T=None), b"NULL"), (dict(ids=None), b"NULL"), (dict(sims=None), b"NULL"),
                     (dict(N=0), b"bad sizes"), (dict(d=0), b"bad sizes"), (dict(nq=-1), b"bad sizes"),
                     (dict(k=0), b"k = 0"), (dict(k=129), b"k = 129"), (dict(metric=2), b"metric"),
                     (dict(Q=p, rows=p), b"not both"), (dict(nq=3), b"nq == N"),
                     (dict(ws=None), b"workspace"), (dict(nbytes=8), b"workspace")]:
        assert call(**kw) == -1, kw
        assert text in lib.skge_last_error(), (kw, lib.skge_last_error())
    assert call(Q=p, nq=0) == 0        # no queries: nothing to do


def _fake_model():
    import torch
    E = types.SimpleNamespace(data=torch.zeros(6, 4))
    R = types.SimpleNamespace(data=torch.zeros(2, 4))
    return types.SimpleNamespace(params={"E": E, "R": R}, device=torch.device("cpu"), d=4)


def test_facade_refusals_come_before_any_launch():
    import skge_amd as S
    m = _fake_model()
    with pytest.raises(ValueError, match="metric"):
        S.Neighbours(m, metric="l1")
    with pytest.raises(ValueError, match="table"):
        S.Neighbours(m, table="X")
    with pytest.raises(ValueError, match="table"):
        S.Neighbours(m, table=np.zeros(5))
    nn = S.Neighbours(m)
    for k in (0, 129, 2.0, True):
        with pytest.raises(ValueError, match="k must be"):
            nn.topk(k=k)
        with pytest.raises(ValueError, match="k must be"):
            nn.query(np.zeros((1, 4)), k=k)
    with pytest.raises(ValueError, match="row 6"):
        nn.topk(k=2, rows=[0, 6])
    with pytest.raises(ValueError, match="row -1"):
        nn.topk(k=2, rows=[-1])
    with pytest.raises(ValueError, match="width 4"):
        nn.query(np.zeros((3, 5)), k=2)
    with pytest.raises(ValueError, match="width 4"):
        S.Neighbours(m, table="R").query(np.zeros(3), k=2)
    # empty queries: empty results, no launch
    for ids, sims in (nn.topk(k=3, rows=[]), nn.query(np.zeros((0, 4)), k=3)):
        assert ids.shape == sims.shape == (0, 3)
        assert ids.dtype == np.int64 and sims.dtype == np.float32
