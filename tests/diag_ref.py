"""fp64 NumPy restatement of DistMult and ComplEx (TEST INFRASTRUCTURE ONLY).

Both models follow HolE's conventions (oracle.skge_oracle.hole_*): E projected
by normless1, pairwise violation f(n) + margin > f(p) with gp = -g(f(p)) and
gn = g(f(n)), contribution lists (pp, pn) for R and (sp, sn, op, on) for E,
mean over occurrences, rparam on R only (pairwise) or on both (logistic).  The
segment mean, the updaters and the projections are the oracle's, by import;
only the trilinear form differs:

  DistMult  phi = sum_k s_k r_k o_k
  ComplEx   phi = sum_j c (a f + b g) + e (a g - b f), a row of width d holding
            d/2 components interleaved: s_j = (a, b) = (x[2j], x[2j+1]),
            r_j = (c, e), o_j = (f, g)

Triples are (s, o, p) rows, as everywhere in the oracle.
"""
import numpy as np

from oracle import skge_oracle as O

MODELS = ("distmult", "complex")


def _c(x):
    """interleaved floats [..., d] -> complex [..., d/2]"""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[-1] % 2:
        raise ValueError("ComplEx needs an even width, not %d" % x.shape[-1])
    return x[..., 0::2] + 1j * x[..., 1::2]


def _f(z):
    """complex [..., d/2] -> interleaved floats [..., d]"""
    out = np.empty(z.shape[:-1] + (2 * z.shape[-1],))
    out[..., 0::2] = z.real
    out[..., 1::2] = z.imag
    return out


def phi(model, s, r, o):
    """The trilinear form over the last axis of rows s, r, o."""
    if model == "distmult":
        return np.sum(s * r * o, axis=-1)
    a, b = s[..., 0::2], s[..., 1::2]
    c, e = r[..., 0::2], r[..., 1::2]
    f, g = o[..., 0::2], o[..., 1::2]
    return np.sum(c * (a * f + b * g) + e * (a * g - b * f), axis=-1)


def d_s(model, r, o):
    """d phi / d s = (c f + e g, c g - e f)"""
    if model == "distmult":
        return r * o
    return _f(np.conj(_c(r)) * _c(o))


def d_o(model, s, r):
    """d phi / d o = (c a - e b, c b + e a)"""
    if model == "distmult":
        return s * r
    return _f(_c(s) * _c(r))


def d_r(model, s, o):
    """d phi / d r = (a f + b g, a g - b f)"""
    if model == "distmult":
        return s * o
    return _f(np.conj(_c(s)) * _c(o))


# the query vectors: the score over candidate rows x is q . x
def q_tail(model, s, r):    # x is the object
    return d_o(model, s, r)


def q_head(model, r, o):    # x is the subject
    return d_s(model, r, o)


def q_rel(model, s, o):     # x is the relation
    return d_r(model, s, o)


def scores(model, E, R, trip):
    s, p, o = O._split(trip)
    return phi(model, E[s], R[p], E[o])


def entity_scores(model, E, R, s, o, p, direction):
    """oracle.entity_scores' form: every entity as the tail or as the head."""
    if direction == "tail":
        return E.dot(q_tail(model, E[s], R[p]))
    return E.dot(q_head(model, R[p], E[o]))


def relation_scores(model, E, R, s, o):
    return R.dot(q_rel(model, E[s], E[o]))


def pairwise_gradients(model, E, R, pos, neg, margin, rparam=0.0, af=O.Sigmoid):
    """hole_pairwise_gradients with the trilinear form.  Returns (pscore_raw,
    nscore_raw, nviol, grads | None)."""
    sp, pp, op = O._split(pos)
    sn, pn, on = O._split(neg)
    praw = scores(model, E, R, pos)
    nraw = scores(model, E, R, neg)
    pf, nf = af.f(praw), af.f(nraw)
    ind = np.where(nf + margin > pf)[0]
    nviol = len(ind)
    if nviol == 0:
        return praw, nraw, 0, None
    sp, sn, op, on, pp, pn = sp[ind], sn[ind], op[ind], on[ind], pp[ind], pn[ind]
    gp = -np.asarray(af.g_given_f(pf[ind]), dtype=np.float64)[:, None]
    gn = np.asarray(af.g_given_f(nf[ind]), dtype=np.float64)[:, None]
    ridx, rsum, rn = O.segment_mean(
        np.concatenate([pp, pn]),
        np.vstack([gp * d_r(model, E[sp], E[op]), gn * d_r(model, E[sn], E[on])]))
    gr = rsum / rn[:, None] + rparam * R[ridx]
    eidx, esum, en = O.segment_mean(
        np.concatenate([sp, sn, op, on]),
        np.vstack([gp * d_s(model, R[pp], E[op]), gn * d_s(model, R[pn], E[on]),
                   gp * d_o(model, E[sp], R[pp]), gn * d_o(model, E[sn], R[pn])]))
    ge = esum / en[:, None]
    return praw, nraw, nviol, {"E": (ge, eidx), "R": (gr, ridx)}


def gradients(model, E, R, trip, ys, rparam=0.0):
    """hole_gradients (logistic loss) with the trilinear form.  Returns
    (score, loss, grads)."""
    ss, ps, os_ = O._split(trip)
    ys = np.asarray(ys, dtype=np.float64)
    score = scores(model, E, R, trip)
    ysc = ys * score
    loss = np.sum(np.logaddexp(0, -ysc))
    fs = -(ys * O.Sigmoid.f(-ysc))[:, None]
    ridx, rsum, rn = O.segment_mean(ps, fs * d_r(model, E[ss], E[os_]))
    gr = rsum / rn[:, None] + rparam * R[ridx]
    eidx, esum, en = O.segment_mean(
        np.concatenate([ss, os_]),
        np.vstack([fs * d_s(model, R[ps], E[os_]), fs * d_o(model, E[ss], R[ps])]))
    ge = esum / en[:, None] + rparam * E[eidx]
    return score, loss, {"E": (ge, eidx), "R": (gr, ridx)}


def pairwise_step(model, params, state, pos, neg, lr, margin, opt="adagrad", rparam=0.0,
                  af=O.Sigmoid):
    """oracle.pairwise_step for DistMult / ComplEx: HolE's updaters and posts."""
    ps, ns, nv, g = pairwise_gradients(model, params["E"], params["R"], pos, neg, margin,
                                       rparam=rparam, af=af)
    if g is not None:
        O.apply_grads("hole", params, state, g, lr, opt)
    return ps, ns, nv, g


def logistic_step(model, params, state, trip, ys, lr, opt="adagrad", rparam=0.0):
    sc, loss, g = gradients(model, params["E"], params["R"], trip, ys, rparam)
    O.apply_grads("hole", params, state, g, lr, opt)
    return sc, loss, g


# ---------------------------------------------------------------------------
# shared test inputs
# ---------------------------------------------------------------------------
def tables(model, N, M, d, seed, scale=None):
    """fp32-representable random tables (float64 arrays)."""
    rs = np.random.RandomState(seed)
    sc = scale if scale is not None else 1.0 / np.sqrt(d)
    E = (rs.randn(N, d) * sc).astype(np.float32).astype(np.float64)
    R = (rs.randn(M, d) * sc).astype(np.float32).astype(np.float64)
    return E, R


def forced_pairs(N, M, P, seed):
    """P explicit pairs with the duplicates the kernels merge: some s == o,
    some sp == sn (the o-corrupted form), some op == on, one relation on every
    pair, a few entities on many pairs."""
    rs = np.random.RandomState(seed)
    pos = np.stack([rs.randint(N, size=P), rs.randint(N, size=P), rs.randint(M, size=P)], axis=1)
    pos[: P // 8, 0] = 3                      # a hub subject
    pos[P // 8: P // 6, 1] = pos[P // 8: P // 6, 0]   # s == o
    pos[:, 2] = np.where(rs.rand(P) < 0.5, 1, pos[:, 2])   # relation 1 on half of them
    neg = pos.copy()
    half = rs.rand(P) < 0.5
    neg[half, 0] = rs.randint(N, size=int(half.sum()))     # s corrupted: op == on, pp == pn
    neg[~half, 1] = rs.randint(N, size=int((~half).sum())) # o corrupted: sp == sn
    neg[-3:] = pos[-3:][:, [1, 0, 2]]                       # all positions differ but p
    return pos.astype(np.int64), neg.astype(np.int64)


# ---------------------------------------------------------------------------
# the fp32 envelope of the evaluation kernels (HolE's dot-product form,
# tests/eval_ref.py rank_envelope: a candidate's fp32 score differs from the
# fp64 one by at most tau_j = 2 (d + 2) u A_j, A_j the score formula on
# absolute values)
# ---------------------------------------------------------------------------
U32 = 2.0 ** -24


def _abs_prod(model, x, y):
    """elementwise bound on |x * y| and |conj(x) * y| (the same for both)"""
    x, y = np.abs(x), np.abs(y)
    if model == "distmult":
        return x * y
    out = np.empty_like(x)
    out[..., 0::2] = x[..., 0::2] * y[..., 0::2] + x[..., 1::2] * y[..., 1::2]
    out[..., 1::2] = x[..., 0::2] * y[..., 1::2] + x[..., 1::2] * y[..., 0::2]
    return out


def slot_scores(model, E, R, s, o, p, slot):
    """(candidate table's fp64 scores, tau) for slot 'tail', 'head' or 'rel'."""
    d = E.shape[1]
    if slot == "tail":
        T, q, qa = E, q_tail(model, E[s], R[p]), _abs_prod(model, E[s], R[p])
    elif slot == "head":
        T, q, qa = E, q_head(model, R[p], E[o]), _abs_prod(model, R[p], E[o])
    else:
        T, q, qa = R, q_rel(model, E[s], E[o]), _abs_prod(model, E[s], E[o])
    return T.dot(q), 2.0 * (d + 2) * U32 * np.abs(T).dot(qa)


def _bounds(sc, tau, t, filt):
    n = len(sc)
    diff, slack = sc - sc[t], tau + tau[t]
    above = diff > slack
    maybe = (diff >= -slack) & (np.arange(n) != t)
    return (1 + above.sum(), 1 + maybe.sum(), 1 + (above & ~filt).sum(), 1 + (maybe & ~filt).sum())


def rank_envelope(model, E, R, queries, known):
    """eval_ref.rank_envelope for DistMult / ComplEx: (lo, hi), each [nq, 4]."""
    N = E.shape[0]
    kset = set(map(tuple, np.asarray(known).reshape(-1, 3).tolist()))
    q = np.asarray(queries).reshape(-1, 3).tolist()
    lo = np.zeros((len(q), 4), dtype=np.int64)
    hi = np.zeros((len(q), 4), dtype=np.int64)
    for i, (s, o, p) in enumerate(q):
        for col, slot, t in ((0, "tail", o), (2, "head", s)):
            sc, tau = slot_scores(model, E, R, s, o, p, slot)
            if slot == "tail":
                filt = np.array([(s, j, p) in kset and j != o for j in range(N)])
            else:
                filt = np.array([(j, o, p) in kset and j != s for j in range(N)])
            lo[i, col], hi[i, col], lo[i, col + 1], hi[i, col + 1] = _bounds(sc, tau, t, filt)
    return lo, hi


def relation_envelope(model, E, R, queries, known):
    """(lo, hi), each [nq, 2]: raw and filtered rank of p among all relations."""
    M = R.shape[0]
    kset = set(map(tuple, np.asarray(known).reshape(-1, 3).tolist()))
    q = np.asarray(queries).reshape(-1, 3).tolist()
    lo = np.zeros((len(q), 2), dtype=np.int64)
    hi = np.zeros((len(q), 2), dtype=np.int64)
    for i, (s, o, p) in enumerate(q):
        sc, tau = slot_scores(model, E, R, s, o, p, "rel")
        filt = np.array([(s, o, j) in kset and j != p for j in range(M)])
        lo[i, 0], hi[i, 0], lo[i, 1], hi[i, 1] = _bounds(sc, tau, p, filt)
    return lo, hi


def topk_forced(model, E, R, s, o, p, slot, k, excluded=()):
    """The candidates every correct fp32 evaluation returns among the k best
    of the slot (all of them when fewer than k remain), and the number of
    places min(k, candidates)."""
    sc, tau = slot_scores(model, E, R, s, o, p, slot)
    keep = np.ones(len(sc), dtype=bool)
    keep[list(excluded)] = False
    ids = np.nonzero(keep)[0]
    places = min(k, len(ids))
    forced = []
    for j in ids:
        rivals = (sc[ids] - sc[j] >= -(tau[ids] + tau[j])).sum() - 1
        if rivals < places:
            forced.append(int(j))
    return forced, places


def eval_case(model, N, M, d, nq, seed):
    """tables, test triples and known triples of the evaluation tests"""
    from eval_ref import random_triples
    E, R = tables(model, N, M, d, seed)
    test, known = random_triples(np.random.RandomState(seed + 1), N, M, nq)
    return E, R, test, known
