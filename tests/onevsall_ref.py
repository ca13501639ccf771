"""1vsAll training of DistMult and ComplEx with N3 in float64: the restatement
the device is compared with (tests/test_gpu_onevsall.py), judged on the CPU by
tests/test_onevsall_ref.py (finite differences of its own loss).  Written from
the definition; it shares no code with the library and imports
nothing from it.

A query is (anchor a, relation p, direction t, target g): t = 0 is (a, p, ?)
with g the triple's object, t = 1 is (?, p, a) with g its subject.  Its query
vector q makes the model's score of candidate e the dot product z_e = q . E_e:

  DistMult        q = E_a o R_p                     (both directions)
  ComplEx tails   q = E_a R_p     heads   q = conj(R_p) E_a
                  on the d / 2 complex components (x[2j], x[2j + 1])

and for B queries over N entities, with eps the label smoothing,

  y'_be = (1 - eps) [e == g_b] + eps / N
  lse_b = log sum_e exp(z_be)
  L_ce  = (1 / B) sum_b ( lse_b - sum_e y'_be z_be )
  G_be  = ( exp(z_be - lse_b) - y'_be ) / B
  gE[e] = sum_b G_be q_b;   dq_b = sum_e G_be E_e, taken through q's real
  Jacobian to gE[a_b] and gR[p_b] (summed, never averaged);
  L_n3  = (n3 / B) sum_b ( |E_a|_3^3 + |R_p|_3^3 + |E_g|_3^3 ),
  |x|_3^3 = sum_k |x_k|^3 (DistMult), sum_j (re_j^2 + im_j^2)^(3/2) (ComplEx),
  with gradient 3 |x_k| x_k, 3 |c_j| (re_j, im_j): 0 at a zero component.

L = L_ce + L_n3.  A query whose anchor, relation, direction or target lies
outside its table contributes nothing; B still counts it.  The step adds
rparam * param, takes SGD or AdaGrad on every E row and on the R rows some valid
query names, and projects every E row with normless1."""
import numpy as np

# the query vectors, their Jacobian, the projection and the step are KvsAll's
from kvsall_ref import (_join, _parts, chain, normless1_rows, query_vectors,  # noqa: F401
                        split_ids, step_from)

MODELS = ("distmult", "complex")


def valid(anchor, rel, dirn, target, N, M):
    a, p, t, g = (np.asarray(x, dtype=np.int64) for x in (anchor, rel, dirn, target))
    return (a >= 0) & (a < N) & (p >= 0) & (p < M) & ((t == 0) | (t == 1)) & (g >= 0) & (g < N)


def n3_norm(model, X):
    """|x|_3^3 of every row of X."""
    if model == "distmult":
        return (np.abs(X) ** 3).sum(axis=-1)
    re, im = _parts(X)
    return ((re * re + im * im) ** 1.5).sum(axis=-1)


def n3_grad(model, X):
    """d |x|_3^3 / d x of every row: 0 (not NaN) at a zero component."""
    if model == "distmult":
        return 3.0 * np.abs(X) * X
    re, im = _parts(X)
    mod = np.sqrt(re * re + im * im)
    return _join(3.0 * mod * re, 3.0 * mod * im)


def forward(model, E, R, anchor, rel, dirn, target, eps, n3=0.0):
    """z, lse, G over the valid queries (rows of the others: z = 0, G = 0,
    lse = log N), L_ce, L_n3 and their sum."""
    E, R = np.asarray(E, dtype=np.float64), np.asarray(R, dtype=np.float64)
    B, (N, d), M = len(anchor), E.shape, R.shape[0]
    ok = valid(anchor, rel, dirn, target, N, M)
    v = np.flatnonzero(ok)
    a, p, t, g = (np.asarray(x)[v] for x in (anchor, rel, dirn, target))
    Q = np.zeros((B, d))
    Q[v] = query_vectors(model, E, R, a, p, t)
    z = Q @ E.T
    m = z.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))[:, 0]
    y = np.zeros((B, N))
    y[v] = eps / N
    y[v, g] += 1.0 - eps
    G = np.zeros((B, N))
    G[v] = (np.exp(z[v] - lse[v, None]) - y[v]) / B
    l_ce = float((lse[v] - (y[v] * z[v]).sum(axis=1)).sum() / B)
    l_n3 = float(n3 / B * (n3_norm(model, E[a]) + n3_norm(model, R[p]) +
                           n3_norm(model, E[g])).sum())
    return {"Q": Q, "z": z, "lse": lse, "y": y, "G": G, "ok": ok, "l_ce": l_ce, "l_n3": l_n3,
            "loss": l_ce + l_n3}


def loss(model, E, R, anchor, rel, dirn, target, eps, n3=0.0):
    return forward(model, E, R, anchor, rel, dirn, target, eps, n3)["loss"]


def gradients(model, E, R, anchor, rel, dirn, target, eps, n3=0.0):
    """fw, gE [N][d], gR [M][d], touched [M] (bool): the plain gradient of L."""
    E, R = np.asarray(E, dtype=np.float64), np.asarray(R, dtype=np.float64)
    fw = forward(model, E, R, anchor, rel, dirn, target, eps, n3)
    B = len(anchor)
    v = np.flatnonzero(fw["ok"])
    a, p, t, g = (np.asarray(x)[v] for x in (anchor, rel, dirn, target))
    G = fw["G"]
    gE = G.T @ fw["Q"]
    dq = (G @ E)[v]
    ga, gr = chain(model, E, R, a, p, t, dq)
    gR = np.zeros_like(R)
    np.add.at(gE, a, ga + n3 / B * n3_grad(model, E[a]))
    np.add.at(gR, p, gr + n3 / B * n3_grad(model, R[p]))
    np.add.at(gE, g, n3 / B * n3_grad(model, E[g]))
    touched = np.zeros(R.shape[0], dtype=bool)
    touched[p] = True
    return fw, gE, gR, touched


def step(model, params, state, batch, eps, n3, lr, opt, rparam):
    """kvsall_ref.step_from on 1vsAll's gradients of batch = (anchor, rel, dirn,
    target)."""
    grads = gradients(model, params["E"], params["R"], *batch, eps, n3)
    return step_from(grads, params, state, lr, opt, rparam)


# ---- cases shared by the CPU and the GPU tests ----

def build_case(model, N, M, B, d, seed, integer=False):
    """Tables and queries: directions mixed, relations drawn from the even ids
    (odd relation rows are named by no query when M > 1).  When the sizes
    allow, the batch holds a repeated anchor (queries 0 and 1), a query whose
    target is its own anchor (query 0), two identical queries (2 and 3) and
    targets at entity 0, N - 1, 127 and 128 (queries 4..7).  Where the plan
    splits a score row between workgroups, targets also sit at the seams
    (kvsall_ref.split_ids: chunk, N - 1, chunk - 1, 0 and the last workgroup's
    element tail, as many as the batch has queries for).  Float tables are
    fp32 values, so the device starts from the same numbers."""
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
    target = rng.randint(0, N, size=B).astype(np.int32)
    target[0] = anchor[0]
    if B > 1:
        anchor[1] = anchor[0]
    if B > 3:
        for x in (anchor, rel, dirn, target):
            x[3] = x[2]
    for b, g in zip(range(4, 8), (0, N - 1, 127, 128)):
        if b < B and 0 <= g < N:
            target[b] = g
    # the seams of the column split, on the queries no record above holds;
    # when those run out, query 0 takes one as its anchor and target
    seams = split_ids(N, M, B, d)
    free = [b for b in range(B) if b >= 8 or b == 1 or (b == 2 and B == 3)]
    for b, g in zip(free, seams):
        target[b] = g
    if len(free) < len(seams):
        target[0] = anchor[0] = seams[len(free)]
        if B > 1:
            anchor[1] = anchor[0]
    return E, R, (anchor, rel, dirn, target)
