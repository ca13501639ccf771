"""NumPy restatement of the subgraph contract: grouping,
embeddings, ranks.  fp64, no torch, no GPU, and no code shared with
skge_amd.subgraphs.

group()          plain Python: ``sorted`` on (p, anchor) and a walk over the
                 sorted list, as the contract words it
embed()          SA = member mean; SV = sum (E[m] - SA)^2 / (count - 1) for
                 count > 2, else SA
scores()         the model's score with row x of X in the entity's place
ranks()          by explicit sort of the eligible subgraphs' scores
chain_scores()   the DEVICE's fp32 arithmetic restated on the host (the query
                 vector's and the score's sequential chains, each operation
                 rounded to fp32), so that ranks() on them must EQUAL the
                 device's ranks, ties included
"""
import numpy as np

SPO, POS = 0, 1
DIRECTIONS = ("tail", "head")


# ----------------------------------------------------------------------------
# grouping
# ----------------------------------------------------------------------------

def group(triples, mincard):
    """The subgraphs of (s, o, p) triples as a list of dicts
    {kind, ent, rel, size, entities}, ids in list order: every SPO subgraph in
    (p, s) order, then every POS subgraph in (p, o) order; a group is a
    subgraph iff count > mincard; members keep the triples' order."""
    trip = [tuple(int(x) for x in t) for t in np.asarray(triples).reshape(-1, 3)]
    out = []
    for kind, a_col, m_col in ((SPO, 0, 1), (POS, 1, 0)):
        srt = sorted(trip, key=lambda t: (t[2], t[a_col]))
        i = 0
        while i < len(srt):
            j = i
            while j < len(srt) and (srt[j][2], srt[j][a_col]) == (srt[i][2], srt[i][a_col]):
                j += 1
            if j - i > mincard:
                out.append({"kind": kind, "ent": srt[i][a_col], "rel": srt[i][2], "size": j - i,
                            "entities": [t[m_col] for t in srt[i:j]]})
            i = j
    return out


def csr(groups):
    """(mem_off int64 [S + 1], mem_ent int64) of group()'s list."""
    off = np.zeros(len(groups) + 1, dtype=np.int64)
    off[1:] = np.cumsum([g["size"] for g in groups])
    ent = np.array([m for g in groups for m in g["entities"]], dtype=np.int64)
    return off, ent


# ----------------------------------------------------------------------------
# embeddings
# ----------------------------------------------------------------------------

def embed(E, groups):
    """(SA, SV) float64 [S, d], two passes per group."""
    E = np.asarray(E, dtype=np.float64)
    SA = np.zeros((len(groups), E.shape[1]))
    SV = np.zeros_like(SA)
    for i, g in enumerate(groups):
        rows = E[g["entities"]]
        n = len(rows)
        SA[i] = rows.sum(axis=0) / n
        SV[i] = ((rows - SA[i]) ** 2).sum(axis=0) / (n - 1) if n > 2 else SA[i]
    return SA, SV


# ----------------------------------------------------------------------------
# scores (fp64) and ranks
# ----------------------------------------------------------------------------

def _ccorr(a, b):
    """ccorr(a, b)_k = sum_i a_i b_{(i + k) mod d}."""
    d = len(a)
    i = np.arange(d)
    return np.array([np.sum(a * b[(i + k) % d]) for k in range(d)])


def _hole_scores(r, X, fixed, direction):
    """r . ccorr(fixed, x) ('tail') or r . ccorr(x, fixed) ('head') for every
    row x of X, with the sums over k and i exchanged so that all rows go
    through one matrix product:
      r . ccorr(a, x) = sum_m x_m sum_k r_k a_{(m - k) mod d}
      r . ccorr(x, b) = sum_i x_i sum_k r_k b_{(i + k) mod d}"""
    d = len(r)
    m, k = np.arange(d)[:, None], np.arange(d)[None, :]
    M = fixed[(m - k) % d] if direction == "tail" else fixed[(m + k) % d]
    return X @ (M @ r)


def scores(model, E, R, X, s, o, p, direction):
    """float64 [S]: row x_i of X as the object of (s, p, x_i) ('tail') or the
    subject of (x_i, p, o) ('head')."""
    E, R, X = (np.asarray(a, dtype=np.float64) for a in (E, R, X))
    if model == "transe":
        if direction == "tail":
            return -np.abs(E[s] + R[p] - X).sum(axis=1)
        return -np.abs(X + R[p] - E[o]).sum(axis=1)
    if model == "hole":
        return _hole_scores(R[p], X, E[s] if direction == "tail" else E[o], direction)
    assert model == "rescal"
    W = R[p].reshape(E.shape[1], E.shape[1])
    return X @ (E[s] @ W) if direction == "tail" else X @ (W @ E[o])


def skip_id(groups, kind, ent, rel):
    for i, g in enumerate(groups):
        if (g["kind"], g["ent"], g["rel"]) == (kind, ent, rel):
            return i
    return -1


def rank_of(sc, groups, answer, skip):
    """(rank, found) from one query's scores [S], by explicit sort."""
    elig = [i for i in range(len(groups)) if i != skip]
    have = [i for i in elig if answer in groups[i]["entities"]]
    if not have:
        return len(elig) + 1, 0
    best = max(sc[i] for i in have)
    order = sorted((sc[i] for i in elig), reverse=True)
    return 1 + order.index(best), 1      # the first of equal scores: ties for the answer


def ranks(score_fn, groups, queries):
    """[nq, 4] int64 (tail, head, found_tail, found_head); score_fn(s, o, p,
    direction) -> [S].  Tail skips the SPO subgraph anchored at (s, p), head
    the POS subgraph anchored at (o, p)."""
    out = np.zeros((len(queries), 4), dtype=np.int64)
    for n, (s, o, p) in enumerate(np.asarray(queries).tolist()):
        out[n, 0], out[n, 2] = rank_of(score_fn(s, o, p, "tail"), groups, o,
                                       skip_id(groups, SPO, s, p))
        out[n, 1], out[n, 3] = rank_of(score_fn(s, o, p, "head"), groups, s,
                                       skip_id(groups, POS, o, p))
    return out


# ----------------------------------------------------------------------------
# the device's fp32 chains on the host
# ----------------------------------------------------------------------------

F32 = np.float32


def _fma32(a, b, c):
    """fp32 fma(a, b, c): the product of two fp32 values is exact in fp64;
    the one fp64 rounding of the sum before the fp32 rounding can differ from
    a true fma only when the fp64 sum lands exactly on an fp32 rounding
    boundary, which the fixed test data does not hit."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
            + np.asarray(c, dtype=np.float64)).astype(F32)


def chain_query(model, E, R, s, o, p, direction):
    """The evaluator's query vector (skge_eval.hip k_rank_query) in its own
    fp32 order: fp32 [d]."""
    E = np.asarray(E, dtype=F32)
    R = np.asarray(R, dtype=F32)
    d = E.shape[1]
    k = np.arange(d)
    if model == "transe":
        return E[s] + R[p] if direction == "tail" else E[o] - R[p]
    acc = np.zeros(d, dtype=F32)
    if model == "hole":
        ea = E[s] if direction == "tail" else E[o]
        for j in range(d):
            ix = (k - j) % d if direction == "tail" else (j + k) % d
            acc = _fma32(R[p][j], ea[ix], acc)
        return acc
    W = R[p].reshape(d, d)
    for j in range(d):
        acc = _fma32(E[s][j], W[j, :], acc) if direction == "tail" else _fma32(W[:, j], E[o][j], acc)
    return acc


def chain_scores(model, E, R, X, s, o, p, direction):
    """fp32 [S]: every row of X under the query vector, by the counting
    pass's sequential-k chain (skge_device.h rank_score)."""
    X = np.asarray(X, dtype=F32)
    q = chain_query(model, E, R, s, o, p, direction)
    acc = np.zeros(X.shape[0], dtype=F32)
    for k in range(X.shape[1]):
        if model == "transe":
            acc = acc - np.abs(q[k] - X[:, k])
        else:
            acc = _fma32(X[:, k], q[k], acc)
    return acc
