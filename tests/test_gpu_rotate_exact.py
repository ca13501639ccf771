"""RotatE evaluation on the device against an int64 reference: on the tables
below every fp32 product, difference, square, square root and partial sum is
an exact small integer, so nothing here is a tolerance -- ranks, ids and scores
must EQUAL the reference, exact ties and their id order included.

The tables.  E holds Gaussian integers in [-3, 3], R components from
{1, -1, i, -i}.  A modulus |q_j - e_j| is an integer when the difference is
purely real or purely imaginary, so per component j all rows sit on one line
(im = c_j or re = c_j) and every query vector must land on it too: where the
relation's component is +-1 any row does (-1 only on a line through 0), and
where it is +-i the query's anchor holds the one value of the line that the
rotation maps back onto it (for im = c: (c, c) under i, (-c, c) under -i) -- a
non-trivial complex product.  Each test triple has anchors of its own.  That
every modulus is an integer is asserted on the CPU (rotate_ref.int_scores)
before a device result is looked at.

Widths {2, 6, 30, 34, 64, 200, 1024} cross the RT_KC = 32 chunk edge of the
score tile and rank_load4's partial-float4 path (d % 4 != 0); N = 150 crosses
the 128-row tile."""
import numpy as np
import pytest
import torch

import eval_ref as X
import rotate_ref as RR
import topk_ref as T

pytestmark = pytest.mark.gpu

WIDTHS = [2, 6, 30, 34, 64, 200, 1024]
N, M, NQ, K = 150, 3, 12, 5
ROT = {0: (1, 0), 1: (0, 1), 2: (-1, 0), 3: (0, -1)}   # 1, i, -1, -i


def _rot(r, v, conj=False):
    re, im = ROT[r]
    if conj:
        im = -im
    return (v[0] * re - v[1] * im, v[0] * im + v[1] * re)


def _tables(d, seed, unit_relations=False):
    """(E, R, test, known) int64; test triple t = (2t, 2t + 1, t % M)."""
    rs = np.random.RandomState(seed)
    h = d // 2
    horiz = rs.randint(2, size=h).astype(bool)      # line im = c (else re = c)
    off = rs.randint(-3, 4, size=h)
    rot = np.zeros((M, h), dtype=np.int64)
    for j in range(h):
        choices = (0, 2) if off[j] == 0 else (0, 1, 3)
        rot[:, j] = rs.choice(choices, size=M)
    if unit_relations:
        rot[:] = 0

    def point(j, x):
        return (x, off[j]) if horiz[j] else (off[j], x)

    def on_line(j, v):
        return (v[1] if horiz[j] else v[0]) == off[j]

    E = np.zeros((N, d), dtype=np.int64)
    for e in range(N):
        for j in range(h):
            E[e, 2 * j], E[e, 2 * j + 1] = point(j, rs.randint(-3, 4))
    test = []
    for t in range(NQ):
        s, o, p = 2 * t, 2 * t + 1, t % M
        test.append((s, o, p))
        for j in range(h):
            for row, conj in ((s, False), (o, True)):
                v = (E[row, 2 * j], E[row, 2 * j + 1])
                if not on_line(j, _rot(rot[p, j], v, conj)):
                    ok = [x for x in range(-3, 4) if on_line(j, _rot(rot[p, j], point(j, x), conj))]
                    assert ok, (j, off[j], rot[p, j])
                    E[row, 2 * j], E[row, 2 * j + 1] = point(j, ok[0])
    # ties: copies of the first triple's true tail and head, and of a bystander
    E[100], E[101], E[102] = E[1], E[0], E[60]
    R = np.zeros((M, d), dtype=np.int64)
    for p in range(M):
        for j in range(h):
            R[p, 2 * j], R[p, 2 * j + 1] = ROT[rot[p, j]]
    test = np.array(test, dtype=np.int64)
    # known: the test triples, other answers of the same queries (some scoring
    # above the true one, some below), unrelated triples
    known = [tuple(x) for x in test.tolist()]
    for s, o, p in test.tolist():
        for e in rs.choice(N, size=6, replace=False).tolist():
            known.append((s, e, p))
            known.append((e, o, p))
    known = np.array(sorted(set(known)), dtype=np.int64)
    assert E.min() >= -3 and E.max() <= 3
    return E, R, test, known


def _query_scores(E, R, q):
    """int64 [2 nq][N]: row 2i the tail scores of triple i, 2i + 1 the head
    scores.  int_scores asserts that every modulus is an integer."""
    out = []
    for s, o, p in q.tolist():
        out.append(RR.int_scores(RR.int_query(E, R, s, p, True), E))
        out.append(RR.int_scores(RR.int_query(E, R, o, p, False), E))
    return np.array(out)


def _answers(q, known):
    """per query vector the known answers other than the true entity"""
    ks = set(map(tuple, known.tolist()))
    out = []
    for s, o, p in q.tolist():
        out.append([e for e in range(N) if e != o and (s, e, p) in ks])
        out.append([e for e in range(N) if e != s and (e, o, p) in ks])
    return out


def _exact_ranks(E, R, q, known, members=None):
    sc = _query_scores(E, R, q)
    ans = _answers(q, known)
    out = np.zeros((len(q), 4), dtype=np.int64)
    for v in range(2 * len(q)):
        true = q[v // 2][1] if v % 2 == 0 else q[v // 2][0]
        above = sc[v] > sc[v][true]
        if members is not None and members[v] is not None:
            mask = np.zeros(N, dtype=bool)
            mask[members[v]] = True
            above &= mask
        raw = 1 + int(above.sum())
        out[v // 2, 2 * (v % 2)] = raw
        out[v // 2, 2 * (v % 2) + 1] = raw - int(sum(above[e] for e in ans[v]))
    return out


def _model(E, R):
    import skge_amd as S
    m = S.RotatE((E.shape[0], E.shape[0], R.shape[0]), E.shape[1])
    m.params["E"].data.copy_(torch.tensor(E, dtype=torch.float32))
    m.params["R"].data.copy_(torch.tensor(R, dtype=torch.float32))
    return m


def _assert_topk(got, want, what):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32
    np.testing.assert_array_equal(got[0], want[0], err_msg="ids, " + what)
    np.testing.assert_array_equal(got[1].astype(np.float64), want[1], err_msg="scores, " + what)


@pytest.mark.parametrize("d", WIDTHS)
def test_ranks_topk_pools_and_scores_equal_reference(d):
    import skge_amd as S
    E, R, test, known = _tables(d, 100 + d)
    q = X.eval_order(test)
    sc = _query_scores(E, R, q)            # (asserts the integer moduli)
    m = _model(E, R)
    ev = S.FilteredRankingEval(test.astype(np.int32), known.astype(np.int32))
    got = ev.ranks(m)
    want = _exact_ranks(E, R, q, known)
    np.testing.assert_array_equal(got, want)
    # the tie and filter constructions hold in this case: copies of the true
    # rows do not count, and some known answer outranks a true entity
    assert (want[:, 1] < want[:, 0]).any() or (want[:, 3] < want[:, 2]).any()
    first = [i for i, x in enumerate(q.tolist()) if x == [0, 1, 0]][0]
    assert sc[2 * first][100] == sc[2 * first][1] and sc[2 * first + 1][101] == sc[2 * first + 1][0]
    # pools: even entities, a small hand-made pool, and every entity (-1)
    pools = [list(range(0, N, 2)), [1, 0, 5, 60, 100, 101, 102, 149]]
    pools = [sorted(p) for p in pools]
    tp = np.array([(i % 3) - 1 for i in range(len(q))], dtype=np.int64)
    hp = np.array([((i + 1) % 3) - 1 for i in range(len(q))], dtype=np.int64)
    members = []
    for i in range(len(q)):
        members.append(None if tp[i] < 0 else pools[tp[i]])
        members.append(None if hp[i] < 0 else pools[hp[i]])
    np.testing.assert_array_equal(ev.candidate_ranks(m, pools, tp, hp),
                                  _exact_ranks(E, R, q, known, members))
    # top-k tails and heads with their tie order
    lp = S.LinkPredictor(m, known)
    for direction, fn, col, rows in (("tail", lp.tails, 0, sc[0::2]), ("head", lp.heads, 1, sc[1::2])):
        qq = q[:, [col, 2]]
        for flt in (False, True):
            excl = T.known_answers(qq, known, direction) if flt else None
            _assert_topk(fn(qq[:, 0], qq[:, 1], k=K, filtered=flt),
                         T.topk_of_scores(rows.astype(np.float64), K, excl),
                         "%s filtered=%s" % (direction, flt))
    # raw scores (k_score_rot): every entity as the tail of each test triple
    trip = np.array([(s, e, p) for s, _, p in q.tolist() for e in range(N)], dtype=np.int32)
    got_sc = m.score(trip).cpu().numpy()
    assert got_sc.dtype == np.float32
    np.testing.assert_array_equal(got_sc.astype(np.float64), sc[0::2].reshape(-1))


@pytest.mark.parametrize("d", [6, 64])
def test_unit_relations_rank_by_modulus_distance(d):
    """Every R_p = (1, 0): the ranks order the entities by the complex-modulus
    distance |E_s - E_o|."""
    import skge_amd as S
    E, R, test, known = _tables(d, 300 + d, unit_relations=True)
    assert np.array_equal(R[:, 0::2], np.ones_like(R[:, 0::2])) and not R[:, 1::2].any()
    q = X.eval_order(test)
    dist = np.array([[-RR.int_scores(E[a], E)[e] for e in range(N)] for a in range(N)])
    m = _model(E, R)
    got = S.FilteredRankingEval(test.astype(np.int32), test.astype(np.int32)).ranks(m)
    for i, (s, o, p) in enumerate(q.tolist()):
        assert got[i, 0] == 1 + int((dist[s] < dist[s][o]).sum())
        assert got[i, 2] == 1 + int((dist[o] < dist[o][s]).sum())
