"""CPU checks of the subgraph contract.

(a) tests/subgraph_ref.py, the NumPy restatement, against
    tests/golden/subgraphs/subgraphs_transe.npz, recorded from the
    reference's own Experiment.make_subgraphs (tools/gen_golden_subgraphs.py):
    the grouping exactly, SA and SV to 1e-12.
(b) skge_amd.Subgraphs.from_triples (numpy sort + run boundaries) against the
    restatement (plain Python): the same grouping and metadata.
(c) the restatement's ranks on a hand-made case.
"""
import os

import numpy as np
import pytest

import subgraph_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "subgraphs", "subgraphs_transe.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE)


@pytest.mark.parametrize("mincard", [0, 2])
def test_restatement_matches_the_reference(golden, mincard):
    z = golden
    pre = "m%d_" % mincard
    groups = G.group(z["triples"], mincard)
    assert len(groups) == len(z[pre + "kind"])
    for key in ("kind", "ent", "rel", "size"):
        np.testing.assert_array_equal([g[key] for g in groups], z[pre + key], err_msg=key)
    off, ent = G.csr(groups)
    np.testing.assert_array_equal(off, z[pre + "mem_off"])
    np.testing.assert_array_equal(ent, z[pre + "mem_ent"])
    sizes = set(z[pre + "size"].tolist())
    assert 3 in sizes                             # count > 2: a real variance
    if mincard == 0:
        assert {1, 2} <= sizes                    # count <= 2: SV = SA
    else:
        assert min(sizes) == 3                    # count > mincard is strict
        assert {1, 2} <= set(golden["m0_size"].tolist())     # ... and dropped groups exist
    SA, SV = G.embed(z["E"], groups)
    np.testing.assert_allclose(SA, z[pre + "avg"], rtol=0, atol=1e-12)
    # the reference closes its LAST group of each kind after its loop, around
    # the previous kept group's mean (skge/base.py:188-197, a bug the contract
    # does not keep).  For mincard 2 the fixture's KG keeps that branch from
    # running; for mincard 0 every group is kept, so the two rows it wrote
    # (m0_stale) are checked against the bug's own formula instead.
    stale = z["m0_stale"].tolist() if mincard == 0 else []
    ok = np.ones(len(groups), dtype=bool)
    ok[stale] = False
    np.testing.assert_allclose(SV[ok], z[pre + "var"][ok], rtol=0, atol=1e-12)
    for i in stale:
        rows = z["E"][groups[i]["entities"]]
        n, prev = len(rows), SA[i - 1]
        want = ((rows - prev) ** 2).sum(axis=0) / (n - 1) if n > 2 else prev
        np.testing.assert_allclose(z[pre + "var"][i], want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("mincard", [0, 1, 2, 5])
def test_from_triples_gives_the_restatements_grouping(golden, mincard):
    from skge_amd.subgraphs import SUBTYPE, Subgraphs
    trip = golden["triples"]
    groups = G.group(trip, mincard)
    sg = Subgraphs.from_triples([tuple(t) for t in trip.tolist()], mincard)
    assert sg.get_Nsubgraphs() == len(groups) == len(sg.subgraphs)
    off, ent = G.csr(groups)
    assert sg.mem_off.dtype == np.int64 and sg.mem_ent.dtype == np.int32
    np.testing.assert_array_equal(sg.mem_off, off)
    np.testing.assert_array_equal(sg.mem_ent, ent)
    np.testing.assert_array_equal(sg.kind, [g["kind"] for g in groups])
    for i, (m, g) in enumerate(zip(sg.subgraphs, groups)):
        assert m.subId == i
        assert m.subType == (SUBTYPE.SPO if g["kind"] == G.SPO else SUBTYPE.POS)
        assert (m.ent, m.rel, m.size, m.entities) == (g["ent"], g["rel"], g["size"],
                                                      g["entities"])
        assert sg.subgraph_id(m.subType, m.ent, m.rel) == i
    assert sg.subgraph_id(SUBTYPE.SPO, 45, 0) == -1
    # an ndarray and the reference's ((s, o, p), y) pairs group alike
    sg2 = Subgraphs.from_triples(trip, mincard)
    sg3 = Subgraphs.from_triples([(tuple(t), 1.0) for t in trip.tolist()], mincard)
    for other in (sg2, sg3):
        np.testing.assert_array_equal(other.mem_ent, sg.mem_ent)
        np.testing.assert_array_equal(other.anchor, sg.anchor)


def test_from_triples_edge_cases():
    from skge_amd.subgraphs import Subgraphs
    assert Subgraphs.from_triples([], 0).get_Nsubgraphs() == 0
    assert Subgraphs.from_triples([(0, 1, 0)], 1).get_Nsubgraphs() == 0
    sg = Subgraphs.from_triples([(0, 1, 0)], 0)
    assert [(m.subType.name, m.ent, m.rel, m.entities) for m in sg.subgraphs] == \
        [("SPO", 0, 0, [1]), ("POS", 1, 0, [0])]


def test_unsupported_branches_raise_before_any_device_work():
    import skge_amd as S
    sg = S.Subgraphs.from_triples([(0, 1, 0)], 0)
    with pytest.raises(NotImplementedError, match="base.py:174"):
        sg.embed(None, sub_algo="hole")
    ev = S.SubgraphRankingEval([(0, 1, 0)], sg)
    with pytest.raises(NotImplementedError, match="base.py:790.*50.*ten"):
        ev.ranks(None, sub_dist="kl")
    with pytest.raises(ValueError):
        ev.ranks(None, sub_dist="median")


def test_scores_summary():
    import skge_amd as S
    pos = {0: {"head": [1, 2], "tail": [4]}, 3: {"head": [4], "tail": [1]}}
    head, tail = S.subgraph_ranking_scores(pos, topk=2)
    assert head == pytest.approx(((1 + 0.5 + 0.25) / 3, 7 / 3, 200 / 3))
    assert tail == pytest.approx(((0.25 + 1) / 2, 2.5, 50.0))


@pytest.mark.parametrize("model", ["transe", "hole", "rescal"])
def test_restatement_scores_are_the_models_scores(model):
    """scores() against the model's score written out per row, and the fp32
    chains of chain_scores() against scores() within fp32 rounding."""
    rs = np.random.RandomState(3)
    n, d, S = 9, 7, 5
    E = rs.uniform(-1, 1, (n, d)).astype(np.float32)
    R = rs.uniform(-1, 1, (3, d * d if model == "rescal" else d)).astype(np.float32)
    X = rs.uniform(-1, 1, (S, d)).astype(np.float32)
    E64, R64, X64 = (a.astype(np.float64) for a in (E, R, X))
    s, o, p = 2, 6, 1

    def one(sub, obj):       # the model's score of (sub, p, obj), vectors in
        if model == "transe":
            return -np.abs(sub + R64[p] - obj).sum()
        if model == "hole":
            return R64[p] @ G._ccorr(sub, obj)
        return sub @ R64[p].reshape(d, d) @ obj

    for direction in G.DIRECTIONS:
        want = np.array([one(E64[s], x) if direction == "tail" else one(x, E64[o]) for x in X64])
        got = G.scores(model, E, R, X, s, o, p, direction)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
        chain = G.chain_scores(model, E, R, X, s, o, p, direction)
        assert chain.dtype == np.float32
        np.testing.assert_allclose(chain, want, rtol=0, atol=1e-5)


def test_restatement_ranks_by_hand():
    """Four subgraphs with scores 3, 5, 5, 1 for every query."""
    groups = [{"kind": G.SPO, "ent": 0, "rel": 0, "size": 2, "entities": [7, 8]},
              {"kind": G.SPO, "ent": 1, "rel": 0, "size": 2, "entities": [8, 9]},
              {"kind": G.POS, "ent": 8, "rel": 0, "size": 2, "entities": [0, 1]},
              {"kind": G.POS, "ent": 9, "rel": 0, "size": 1, "entities": [1]}]
    sc = np.array([3.0, 5.0, 5.0, 1.0])
    fn = lambda s, o, p, direction: sc
    # (0, 8, 0): tail skips subgraph 0; 8 is in 1 (score 5, tied first) -> 1.
    #            head skips subgraph 2; 0 is in no other subgraph -> 3 + 1, not found.
    # (1, 7, 0): tail skips 1; 7 is in 0 (score 3), above it only 2 -> 2.
    #            head skips nothing; 1 is in 2 (5) and 3 (1): the best, 5 -> 1.
    # (5, 9, 1): nothing skipped; tail 9 is in 1 -> 1; head 5 is nowhere -> 4 + 1.
    got = G.ranks(fn, groups, [(0, 8, 0), (1, 7, 0), (5, 9, 1)])
    np.testing.assert_array_equal(got, [[1, 4, 1, 0], [2, 1, 1, 1], [1, 5, 1, 0]])
