"""Device subgraph embeddings and ranks (skge_subgraph_embed / _rank through
skge_amd.Subgraphs and SubgraphRankingEval) against tests/subgraph_ref.py.

(a) SA / SV against the fp64 restatement within the project's fp32 bar
    (parity_util), for every row layout of the kernel (d % 4 != 0, one wave's
    width, the workload's d = 200, and the wider register layouts), group sizes
    1, 2, 3 and a group long enough to be split into pieces (the split
    threshold shrunk through SKGE_SUBGRAPH_SPLIT), bit-equal between runs;
(b) ranks EQUAL to the restatement's explicit sort over the device's own
    fp32 scores, recomputed on the host in the device's order of operations
    (subgraph_ref.chain_scores), on a KG with an exact tie, an answer in no
    subgraph, an answer only in the skipped subgraph and queries that skip
    nothing;
(c) the facade: 'var', positions(), a given table, attach;
(d) argument errors.
"""
import functools

import numpy as np
import pytest
import torch

import parity_util as PU
import subgraph_ref as G

pytestmark = pytest.mark.gpu

N_ENT, N_REL = 64, 4
HUB = 23            # members of the long group (p = 0, s = 0)
SPLIT = 4           # SKGE_SUBGRAPH_SPLIT for the split runs: 6 pieces, the last of 3
MODELS = ["transe", "hole", "rescal"]


@functools.lru_cache(maxsize=None)
def _kg():
    """(triples, queries): entities 0 .. 39 at random, and by construction
    - (p 0, s 0) with objects 1 .. 23: the long group;
    - (p 1, s 10) and (p 1, s 11) with the same objects 20, 21, 22, in the
      same order: equal embeddings, an exact score tie;
    - (p 2, s 12) with objects 40, 41, 42, which occur nowhere else: the tail
      answer of (12, 40, 2) lies only in the subgraph that query skips;
    - entity 63 occurs in no triple: an answer in no subgraph."""
    rs = np.random.RandomState(5)
    twins = [(s, o, 1) for o in (20, 21, 22) for s in (10, 11)]
    trip = [(0, o, 0) for o in range(1, 1 + HUB)]
    trip += [(12, o, 2) for o in (40, 41, 42)]
    seen = set(trip + twins)
    while len(trip) < 125 - len(twins):
        t = (int(rs.randint(1, 10)), int(rs.randint(24, 40)), int(rs.randint(N_REL)))
        if t not in seen:
            seen.add(t)
            trip.append(t)
    order = rs.permutation(len(trip))
    # the twins keep their order (members keep the triples' order, and equal
    # bits need the same order of additions)
    trip = np.concatenate([np.array(trip, dtype=np.int64)[order], np.array(twins)])
    inside = trip[rs.permutation(len(trip))[:78]]
    outside = np.stack([rs.randint(0, N_ENT, 18), rs.randint(0, N_ENT, 18),
                        rs.randint(0, N_REL, 18)], axis=1)
    special = np.array([(12, 40, 2),      # the answer only in the skipped subgraph
                        (0, 63, 0),       # the tail answer in no subgraph
                        (63, 5, 3),       # the head answer in no subgraph, nothing to skip
                        (10, 20, 1)])     # best score shared by two subgraphs
    q = np.concatenate([special, inside, outside])
    for a in (trip, q):
        a.setflags(write=False)
    return trip, q


def _model(name, d, seed):
    """A model whose tables hold fp32 uniform(-1, 1) values; returns it and
    the tables as float32 arrays."""
    import skge_amd as S
    m = {"transe": S.TransE, "hole": S.HolE, "rescal": S.RESCAL}[name](
        (N_ENT, N_ENT, N_REL), d, init="device_nunif")
    rid = "W" if name == "rescal" else "R"
    rs = np.random.RandomState(seed)
    E = rs.uniform(-1, 1, tuple(m.params["E"].shape)).astype(np.float32)
    R = rs.uniform(-1, 1, tuple(m.params[rid].shape)).astype(np.float32)
    m.params["E"].data.copy_(torch.from_numpy(E))
    m.params[rid].data.copy_(torch.from_numpy(R))
    return m, E, R.reshape(N_REL, -1)


# ---------------------------------------------------------------------------
# (a) embeddings
# ---------------------------------------------------------------------------

# d: 8 and 200 take 16-byte loads, 50 does not, 64 is one wave's width; 130,
# 300, 1001 and 1024 are the wider register layouts (scalar 4 and 16 per
# lane, 2 and 4 float4 per lane)
@pytest.mark.parametrize("split", [SPLIT, None])
@pytest.mark.parametrize("d,mincard", [(8, 0), (8, 2), (50, 0), (50, 2), (64, 0), (64, 2),
                                       (200, 0), (200, 2), (130, 0), (300, 0), (1001, 0),
                                       (1024, 0)])
def test_embeddings_match_the_restatement(monkeypatch, d, mincard, split):
    import skge_amd as S
    if split is None:
        monkeypatch.delenv("SKGE_SUBGRAPH_SPLIT", raising=False)
    else:
        monkeypatch.setenv("SKGE_SUBGRAPH_SPLIT", str(split))
    trip, _ = _kg()
    groups = G.group(trip, mincard)
    sizes = [g["size"] for g in groups]
    assert HUB in sizes and HUB > 5 * SPLIT and 3 in sizes
    if mincard == 0:
        assert 1 in sizes and 2 in sizes
    m, E, _ = _model("transe", d, 100 + d)
    sg = S.Subgraphs.from_triples(trip, mincard)
    assert sg.get_Nsubgraphs() == len(groups)
    SA, SV = sg.embed(m, variance=True)
    want_a, want_v = G.embed(E, groups)
    what = "subgraphs d=%d mincard=%d split=%s " % (d, mincard, split)
    PU.check(SA, want_a, what + "SA")
    PU.check(SV, want_v, what + "SV")
    # the same bits on every run, and SA does not depend on asking for SV
    SA2, SV2 = sg.embed(m, variance=True)
    assert torch.equal(SA, SA2) and torch.equal(SV, SV2)
    SA3, none = sg.embed(m)
    assert none is None and torch.equal(SA, SA3)
    small = [i for i, n in enumerate(sizes) if n <= 2]
    assert torch.equal(SV[small], SA[small])      # the reference's quirk, exactly


def test_a_short_workspace_leaves_long_groups_unsplit(monkeypatch):
    """The workspace of 0 members holds two pieces; the long group needs six,
    so it runs unsplit and still meets the bar."""
    import skge_amd as S
    from skge_amd import _lib as L
    monkeypatch.setenv("SKGE_SUBGRAPH_SPLIT", str(SPLIT))
    trip, _ = _kg()
    groups = G.group(trip, 2)
    m, E, _ = _model("transe", 8, 3)
    sg = S.Subgraphs.from_triples(trip, 2)
    off, ent, _, _ = sg.device_arrays(m.device, N_ENT)
    n = len(groups)
    SA = torch.empty((n, 8), dtype=torch.float32, device=m.device)
    SV = torch.empty_like(SA)
    lib = L.lib()
    nbytes = lib.skge_subgraph_embed_workspace_bytes(n, 8, 0)
    assert 0 < nbytes < lib.skge_subgraph_embed_workspace_bytes(n, 8, len(sg.mem_ent))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=m.device)
    L.check(lib.skge_subgraph_embed(L.stream_ptr(), L.ptr(m.params["E"].data), N_ENT, 8,
                                    L.ptr(off), L.ptr(ent), n, L.ptr(SA), L.ptr(SV), L.ptr(ws),
                                    nbytes), "embed")
    want_a, want_v = G.embed(E, groups)
    PU.check(SA, want_a, "subgraphs short workspace SA")
    PU.check(SV, want_v, "subgraphs short workspace SV")


# ---------------------------------------------------------------------------
# (b) ranks
# ---------------------------------------------------------------------------

MINCARD = 2


@pytest.mark.parametrize("sub_dist", ["avg", "var"])
@pytest.mark.parametrize("d", [8, 50])
@pytest.mark.parametrize("model", MODELS)
def test_ranks_equal_the_restatement(model, d, sub_dist):
    import skge_amd as S
    trip, q = _kg()
    groups = G.group(trip, MINCARD)
    S_n = len(groups)
    assert 30 <= S_n <= 60 and len(q) >= 100
    m, E, R = _model(model, d, 7 * d + len(model))
    sg = S.Subgraphs.from_triples(trip, MINCARD)
    SA, SV = sg.embed(m, variance=True)
    X = (SV if sub_dist == "var" else SA).cpu().numpy()
    ev = S.SubgraphRankingEval(q, sg)
    tail, head, ftail, fhead = ev.ranks(m, sub_dist)
    # the evaluator's order: by relation, then insertion order
    qs = np.array([(s, o, p) for p, sos in ev.idx.items() for (s, o) in sos])
    assert sorted(map(tuple, qs.tolist())) == sorted(map(tuple, q.tolist()))
    want = G.ranks(lambda s, o, p, dr: G.chain_scores(model, E, R, X, s, o, p, dr), groups, qs)
    got = np.stack([tail, head, ftail, fhead], axis=1)
    np.testing.assert_array_equal(got, want)

    # what the KG was built to hold
    row = {tuple(t): i for i, t in reversed(list(enumerate(qs.tolist())))}
    i = row[(12, 40, 2)]         # the answer only in the skipped subgraph
    assert G.skip_id(groups, G.SPO, 12, 2) >= 0
    assert (got[i, 0], got[i, 2]) == (S_n - 1 + 1, 0)
    i = row[(0, 63, 0)]          # the answer in no subgraph; the hub is skipped
    assert (got[i, 0], got[i, 2]) == (S_n - 1 + 1, 0)
    i = row[(63, 5, 3)]          # nothing skipped, the head answer in no subgraph
    assert G.skip_id(groups, G.SPO, 63, 3) == -1 and G.skip_id(groups, G.POS, 5, 3) == -1
    assert (got[i, 1], got[i, 3]) == (S_n + 1, 0)
    a, b = G.skip_id(groups, G.SPO, 10, 1), G.skip_id(groups, G.SPO, 11, 1)
    assert a >= 0 and b >= 0 and np.array_equal(X[a], X[b])       # the exact tie
    assert (got[:, 2:] == 1).any() and (got[:, :2] > 1).any()
    skips = np.array([[G.skip_id(groups, G.SPO, s, p), G.skip_id(groups, G.POS, o, p)]
                      for s, o, p in qs.tolist()])
    assert (skips == -1).any() and (skips >= 0).any()
    # found answers rank within the eligible subgraphs
    elig = S_n - (skips >= 0)
    assert (got[:, :2][got[:, 2:] == 1] <= elig[got[:, 2:] == 1]).all()


def test_the_tied_query_ranks_first_among_equals():
    """Subgraphs (SPO, 10, 1) and (SPO, 11, 1) have the same members, 20 among
    them, and so the same row.  (10, 20, 1) and (11, 20, 1) skip one of the
    twins, (5, 20, 1) neither: there the two best containing subgraphs tie,
    and neither counts against the other."""
    import skge_amd as S
    trip, _ = _kg()
    groups = G.group(trip, MINCARD)
    m, E, R = _model("transe", 8, 1)
    sg = S.Subgraphs.from_triples(trip, MINCARD)
    SA, _ = sg.embed(m)
    X = SA.cpu().numpy()
    a, b = G.skip_id(groups, G.SPO, 10, 1), G.skip_id(groups, G.SPO, 11, 1)
    q = np.array([(10, 20, 1), (11, 20, 1), (5, 20, 1)])
    tail, _, found, _ = S.SubgraphRankingEval(q, sg).ranks(m, table=SA)
    for i, (s, o, p) in enumerate(q.tolist()):
        sc = G.chain_scores("transe", E, R, X, s, o, p, "tail")
        assert sc[a] == sc[b]
        skip = G.skip_id(groups, G.SPO, s, p)
        have = [j for j in range(len(groups)) if j != skip and o in groups[j]["entities"]]
        best = max(sc[j] for j in have)
        above = sum(1 for j in range(len(groups)) if j != skip and sc[j] > best)
        assert (tail[i], found[i]) == (1 + above, 1)


# ---------------------------------------------------------------------------
# (c) the facade
# ---------------------------------------------------------------------------

def test_positions_tables_and_attach():
    import skge_amd as S
    trip, q = _kg()
    m, _, _ = _model("hole", 8, 2)
    sg = S.Subgraphs.from_triples(trip, MINCARD)
    ev = S.SubgraphRankingEval([tuple(t) for t in q.tolist()], sg)
    pos = ev.positions(m, "avg")
    tail, head, _, _ = ev.last_ranks
    assert set(pos) == set(q[:, 2].tolist())
    assert all(set(v) == {"head", "tail"} for v in pos.values())
    assert sum(len(v["head"]) for v in pos.values()) == len(q) == ev.sz
    assert [x for p in pos for x in pos[p]["tail"]] == tail.tolist()
    assert [x for p in pos for x in pos[p]["head"]] == head.tolist()
    assert all(isinstance(x, int) for x in pos[q[0, 2]]["head"])
    hs, ts = S.subgraph_ranking_scores(pos, topk=5)
    assert hs == pytest.approx(S.compute_scores(head, 5))
    assert ts == pytest.approx(S.compute_scores(tail, 5))
    # a given table is the table ranked; attach sets the model's SA / SV
    SA, SV = sg.embed(m, variance=True, attach=True)
    assert m.SA is SA and m.SV is SV
    assert ev.positions(m, "avg", table=SA) == pos
    pos_v = ev.positions(m, "var", table=SV)
    assert pos_v == ev.positions(m, "var") and pos_v != pos
    with pytest.raises(ValueError):
        ev.ranks(m, table=SA[:, :4])
    # ids are checked on the host
    with pytest.raises(ValueError, match="out of range"):
        S.SubgraphRankingEval([(0, N_ENT, 0)], sg).ranks(m)
    with pytest.raises(ValueError, match="out of range"):
        S.Subgraphs.from_triples([(0, N_ENT, 0)], 0).embed(m)


# ---------------------------------------------------------------------------
# (d) argument errors: SKGE_EINVAL, nothing launched
# ---------------------------------------------------------------------------

def test_argument_errors():
    from skge_amd import _lib as L
    lib = L.lib()
    dev = torch.device("cuda:0")
    f = torch.zeros(64, dtype=torch.float32, device=dev)
    i32 = torch.zeros(64, dtype=torch.int32, device=dev)
    i64 = torch.zeros(64, dtype=torch.int64, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    st, P = L.stream_ptr(), L.ptr

    def embed(E=f, d=8, off=i64, ent=i32, S=1, SA=f):
        return lib.skge_subgraph_embed(st, P(E), 4, d, P(off), P(ent), S, P(SA), None, P(ws),
                                       ws.numel())

    out = torch.full((4,), -7, dtype=torch.int32, device=dev)
    none = torch.full((4,), -1, dtype=torch.int32, device=dev)      # nothing to skip

    def rank(E=f, R=f, X=f, d=8, S=1, nq=1):
        return lib.skge_subgraph_rank(st, 0, P(E), P(R), 4, d, P(X), S, P(i32), nq, P(none),
                                      P(none), P(i64), P(i32), P(ws), ws.numel(), P(out),
                                      P(out[2:]))

    for call, text in ((lambda: embed(d=1025), b"1024"), (lambda: embed(E=None), b"NULL"),
                       (lambda: embed(SA=None), b"NULL"), (lambda: embed(off=None), b"NULL"),
                       (lambda: embed(S=0), b"S > 0"), (lambda: rank(d=1025), b"1024"),
                       (lambda: rank(E=None), b"NULL"), (lambda: rank(R=None), b"NULL"),
                       (lambda: rank(X=None), b"NULL"), (lambda: rank(S=0), b"S > 0")):
        assert call() == -1
        assert text in lib.skge_last_error()
    torch.cuda.synchronize()
    assert out.tolist() == [-7] * 4           # nothing ran
    # the same calls with good arguments: one empty subgraph, one query whose
    # answers it does not hold
    assert embed() == 0 and rank() == 0
    torch.cuda.synchronize()
    assert out.tolist() == [2, 2, 0, 0] and int(f.abs().sum().item()) == 0
