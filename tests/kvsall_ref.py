"""KvsAll (1-N) training of DistMult and ComplEx in float64: the restatement
the device is compared with (tests/test_gpu_kvsall.py), judged on the CPU by
tests/test_kvsall_ref.py (finite differences of its own loss).  Written from
the definition; it shares no code with the library.

A query is (anchor a, relation p, direction t): t = 0 asks for the tails of
(a, p, ?), t = 1 for the heads of (?, p, a).  Its query vector q makes the
model's score of candidate e the dot product z_e = q . E_e:

  DistMult        q = E_a o R_p                     (both directions)
  ComplEx tails   q = E_a R_p     heads   q = conj(R_p) E_a
                  on the d / 2 complex components (x[2j], x[2j + 1])

and for a batch of B queries over N entities, with eps the label smoothing,

  y'_be = (1 - eps) [e answers b] + eps / N
  L     = (1 / B) sum_b sum_e softplus(z_be) - y'_be z_be
  G_be  = (sigmoid(z_be) - y'_be) / B
  gE[e] = sum_b G_be q_b;   dq_b = sum_e G_be E_e, taken through q's real
  Jacobian to gE[a_b] and gR[p_b] (summed, never averaged).

softplus(z) - y z = -(y log sigmoid(z) + (1 - y) log(1 - sigmoid(z))).
The step adds rparam * param, takes SGD or AdaGrad on every E row and on the R
rows some query names, and projects every E row with normless1."""
import numpy as np

MODELS = ("distmult", "complex")


def softplus(x):
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _parts(x):
    return x[..., 0::2], x[..., 1::2]


def _join(re, im):
    out = np.empty(re.shape[:-1] + (2 * re.shape[-1],), dtype=np.float64)
    out[..., 0::2] = re
    out[..., 1::2] = im
    return out


def query_vectors(model, E, R, anchor, rel, dirn):
    """Q [B][d]."""
    a, r = E[np.asarray(anchor)], R[np.asarray(rel)]
    if model == "distmult":
        return a * r
    tail = (np.asarray(dirn) == 0)[:, None]
    ar, ai = _parts(a)
    rr, ri = _parts(r)
    # tails a r; heads conj(r) a
    re = np.where(tail, ar * rr - ai * ri, rr * ar + ri * ai)
    im = np.where(tail, ar * ri + ai * rr, rr * ai - ri * ar)
    return _join(re, im)


def chain(model, E, R, anchor, rel, dirn, dq):
    """(d L / d E_a, d L / d R_p) rows [B][d] from dq [B][d]: the transposed
    real Jacobian of query_vectors, component by component."""
    a, r = E[np.asarray(anchor)], R[np.asarray(rel)]
    if model == "distmult":
        return dq * r, dq * a
    tail = (np.asarray(dirn) == 0)[:, None]
    ar, ai = _parts(a)
    rr, ri = _parts(r)
    qr, qi = _parts(dq)
    # tails: q.re = ar rr - ai ri, q.im = ar ri + ai rr
    # heads: q.re = rr ar + ri ai, q.im = rr ai - ri ar
    ga_re = np.where(tail, qr * rr + qi * ri, qr * rr - qi * ri)
    ga_im = np.where(tail, -qr * ri + qi * rr, qr * ri + qi * rr)
    gr_re = qr * ar + qi * ai
    gr_im = np.where(tail, -qr * ai + qi * ar, qr * ai - qi * ar)
    return _join(ga_re, ga_im), _join(gr_re, gr_im)


def labels(off, ans, B, N):
    """Multi-hot [B][N] of the answers' CSR."""
    Y = np.zeros((B, N), dtype=bool)
    off = np.asarray(off, dtype=np.int64)
    for b in range(B):
        Y[b, np.asarray(ans[off[b]:off[b + 1]], dtype=np.int64)] = True
    return Y


def forward(model, E, R, anchor, rel, dirn, off, ans, eps):
    E, R = np.asarray(E, dtype=np.float64), np.asarray(R, dtype=np.float64)
    B, N = len(anchor), E.shape[0]
    Q = query_vectors(model, E, R, anchor, rel, dirn)
    z = Q @ E.T
    y = (1.0 - eps) * labels(off, ans, B, N) + eps / N
    loss = float((softplus(z) - y * z).sum() / B)
    return {"Q": Q, "z": z, "y": y, "loss": loss}


def loss(model, E, R, anchor, rel, dirn, off, ans, eps):
    return forward(model, E, R, anchor, rel, dirn, off, ans, eps)["loss"]


def gradients(model, E, R, anchor, rel, dirn, off, ans, eps):
    """fw, gE [N][d], gR [M][d], touched [M] (bool): the plain gradient of L."""
    E, R = np.asarray(E, dtype=np.float64), np.asarray(R, dtype=np.float64)
    fw = forward(model, E, R, anchor, rel, dirn, off, ans, eps)
    B = len(anchor)
    G = (sigmoid(fw["z"]) - fw["y"]) / B
    gE = G.T @ fw["Q"]
    dq = G @ E
    ga, gr = chain(model, E, R, anchor, rel, dirn, dq)
    gR = np.zeros_like(R)
    np.add.at(gE, np.asarray(anchor), ga)
    np.add.at(gR, np.asarray(rel), gr)
    touched = np.zeros(R.shape[0], dtype=bool)
    touched[np.asarray(rel)] = True
    fw["G"] = G
    return fw, gE, gR, touched


def normless1_rows(P):
    ss = (P * P).sum(axis=1, keepdims=True)
    return P / np.where(ss < 1.0, 1.0, ss)


def step_from(grads, params, state, lr, opt, rparam):
    """One batch from params {"E", "R"} (and AdaGrad state, or None) and the
    batch's `gradients` (fw, gE, gR, touched): returns fw, the new params, the
    new state, and per table (g rows incl. rparam * param, ids, the rows before
    the projection)."""
    fw, gE, gR, touched = grads
    E, R = params["E"], params["R"]
    ids = {"E": np.arange(E.shape[0]), "R": np.flatnonzero(touched)}
    g = {"E": gE + rparam * E, "R": (gR + rparam * R)[ids["R"]]}
    new, nstate, pre = {}, {}, {}
    for pid in ("E", "R"):
        P = params[pid].copy()
        i = ids[pid]
        if opt == "adagrad":
            p2 = state[pid].copy()
            p2[i] += g[pid] ** 2
            P[i] -= lr * g[pid] / np.maximum(np.sqrt(p2[i]), 1e-7)
            nstate[pid] = p2
        else:
            P[i] -= lr * g[pid]
            nstate[pid] = None
        pre[pid] = P.copy()
        new[pid] = normless1_rows(P) if pid == "E" else P
    return fw, new, nstate, {pid: (g[pid], ids[pid]) for pid in ("E", "R")}, pre


def step(model, params, state, batch, eps, lr, opt, rparam):
    """step_from on KvsAll's gradients of batch = (anchor, rel, dirn, off, ans)."""
    grads = gradients(model, params["E"], params["R"], *batch, eps)
    return step_from(grads, params, state, lr, opt, rparam)


# ---- cases shared by the CPU and the GPU tests ----

def build_case(model, N, M, B, d, seed, integer=False):
    """Tables, queries (directions mixed, relations drawn from the even ids so
    that odd relation rows are named by no query when M > 1) and answers.
    When the sizes allow, the batch holds: a repeated anchor (queries 0 and 1),
    a self-loop answer (query 0 answers with its own anchor), an empty answer
    list (query 2) and an answer list longer than 64 (query 3, N > 64).
    Float tables are fp32 values, so the device starts from the same numbers."""
    rng = np.random.RandomState(seed)
    if integer:
        E = rng.randint(-3, 4, size=(N, d)).astype(np.float64)
        R = rng.randint(-3, 4, size=(M, d)).astype(np.float64)
    else:
        E = rng.uniform(-0.5, 0.5, size=(N, d)).astype(np.float32).astype(np.float64)
        R = rng.uniform(-0.5, 0.5, size=(M, d)).astype(np.float32).astype(np.float64)
    anchor = rng.randint(0, N, size=B).astype(np.int32)
    rel = (2 * rng.randint(0, (M + 1) // 2, size=B)).astype(np.int32)
    dirn = (np.arange(B) % 2).astype(np.int32)
    rng.shuffle(dirn)
    if B > 1:
        anchor[1] = anchor[0]
    lists = []
    for b in range(B):
        n = rng.randint(1, min(N, 6) + 1)
        lists.append(np.sort(rng.choice(N, size=n, replace=False)))
    lists[0] = np.unique(np.append(lists[0], anchor[0]))
    if B > 2:
        lists[2] = np.zeros(0, dtype=np.int64)
    if B > 3 and N > 64:
        lists[3] = np.sort(rng.choice(N, size=min(N, 70), replace=False))
    off = np.zeros(B + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    ans = (np.concatenate(lists) if off[-1] else np.zeros(0)).astype(np.int32)
    return E, R, (anchor, rel, dirn, off, ans)


# the table tile is 128 rows, an MFMA block 32 queries, a query block 128, a
# staging group 4 dims and a chunk 32: every value of each axis, with each model
EDGE_SHAPES = [   # (N, B, d)
    (1, 1, 2), (127, 33, 8), (128, 130, 50), (129, 1, 200), (300, 33, 200), (300, 130, 8),
    (129, 130, 2), (127, 1, 50), (128, 33, 2), (1, 130, 50),
]
EDGE_M = 7
