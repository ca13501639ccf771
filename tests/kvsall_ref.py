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
import collections

import numpy as np

MODELS =("distmult", "complex")


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


def valid(anchor, rel, dirn, N, M):
    """A query names a row of E, a row of R and a direction 0 or 1."""
    a, p, t = (np.asarray(x, dtype=np.int64) for x in (anchor, rel, dirn))
    return (a >= 0) & (a < N) & (p >= 0) & (p < M) & ((t == 0) | (t == 1))


def labels(off, ans, B, N):
    """Multi-hot [B][N] of the answers' CSR; an id outside [0, N) is no answer."""
    Y = np.zeros((B, N), dtype=bool)
    off = np.asarray(off, dtype=np.int64)
    for b in range(B):
        ids = np.asarray(ans[off[b]:off[b + 1]], dtype=np.int64)
        Y[b, ids[(ids >= 0) & (ids < N)]] = True
    return Y


def forward(model, E, R, anchor, rel, dirn, off, ans, eps):
    """An invalid query (`valid`) scores as the zero vector: z = 0 on its whole
    row.  It still takes the BCE of its labels (log 2 per entity, whatever the
    labels) and still counts in 1 / B."""
    E, R = np.asarray(E, dtype=np.float64), np.asarray(R, dtype=np.float64)
    B, (N, d) = len(anchor), E.shape
    ok = valid(anchor, rel, dirn, N, R.shape[0])
    v = np.flatnonzero(ok)
    Q = np.zeros((B, d))
    Q[v] = query_vectors(model, E, R, np.asarray(anchor)[v], np.asarray(rel)[v],
                         np.asarray(dirn)[v])
    z = Q @ E.T
    y = (1.0 - eps) * labels(off, ans, B, N) + eps / N
    loss = float((softplus(z) - y * z).sum() / B)
    return {"Q": Q, "z": z, "y": y, "ok": ok, "loss": loss}


def loss(model, E, R, anchor, rel, dirn, off, ans, eps):
    return forward(model, E, R, anchor, rel, dirn, off, ans, eps)["loss"]


def gradients(model, E, R, anchor, rel, dirn, off, ans, eps):
    """fw, gE [N][d], gR [M][d], touched [M] (bool): the plain gradient of L.
    An invalid query's q is the constant 0, so it reaches no table row: nothing
    through gE = G^T Q, no chain rule, no mark."""
    E, R = np.asarray(E, dtype=np.float64), np.asarray(R, dtype=np.float64)
    fw = forward(model, E, R, anchor, rel, dirn, off, ans, eps)
    B = len(anchor)
    v = np.flatnonzero(fw["ok"])
    a, p, t = (np.asarray(x)[v] for x in (anchor, rel, dirn))
    G = (sigmoid(fw["z"]) - fw["y"]) / B
    gE = G.T @ fw["Q"]
    dq = (G @ E)[v]
    ga, gr = chain(model, E, R, a, p, t, dq)
    gR = np.zeros_like(R)
    np.add.at(gE, a, ga)
    np.add.at(gR, p, gr)
    touched = np.zeros(R.shape[0], dtype=bool)
    touched[p] = True
    fw["G"] = G
    fw["dq"] = dq
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


# ---- the 1-N batch core's plan (csrc/skge_kvsall.hip, kv_plan), restated ----
# tests/test_kvsall_ref.py and tests/test_onevsall_ref.py hold it against the
# library's two _workspace_bytes calls, so a change of the plan shows there and
# the regime claims of REGIME_SHAPES cannot go stale unnoticed.

Plan = collections.namedtuple("Plan", "ldg wpr nbx nby ntd kslice ns nsplit chunk total")
TILE, KC = 128, 32   # output rows / columns per tile, contraction indices per LDS chunk


def _cdiv(a, b):
    return -(-a // b)


def plan(regime, B, N, M, d):
    """regime "kvsall" or "onevsall".  nsplit and chunk are 1vsAll's (0 in
    KvsAll's plan); total is the workspace in bytes, every part rounded up to
    256."""
    assert regime in ("kvsall", "onevsall")
    ova = regime == "onevsall"
    ldg = (N + 3) & ~3
    wpr = _cdiv(N, 32)
    nbx, nby, ntd = _cdiv(B, TILE), _cdiv(N, TILE), _cdiv(d, TILE)
    # DQ: about 512 workgroups, the partials at most 16 MB
    tiles, chunks = nbx * ntd, _cdiv(N, KC)
    cap = max(1, (16 << 20) // (B * d * 4))
    want = max(1, min(chunks, _cdiv(512, tiles), cap))
    per = _cdiv(chunks, want)
    kslice = min(per * KC, 1 << 30)
    ns = _cdiv(chunks, per)
    nsplit = chunk = 0
    if ova:   # about 1024 workgroups, none with fewer than 1024 columns
        want = max(1, min(_cdiv(1024, B), _cdiv(N, 1024)))
        chunk = min((_cdiv(N, want) + 3) & ~3, (1 << 31) - 4)
        nsplit = _cdiv(N, chunk)
    parts = [B * d * 4]                                     # Q
    if not ova:
        parts.append(B * wpr * 4)                           # the answers' bitmap
    parts += [B * ldg * 4, ns * B * d * 4]                  # G, the DQ partials
    if ova:
        parts += [3 * nby * B * 4, B * 4, (N + M) * 4]      # row partials, lse, occ
    parts += [(B if ova else nbx * nby) * 4,                # loss partials
              N * d * 4, M * d * 4, M * 4]                  # gE, gR, the marks
    total = sum((x + 255) & ~255 for x in parts)
    return Plan(ldg, wpr, nbx, nby, ntd, kslice, ns, nsplit, chunk, total)


def last_slice(p, N):
    """Entities in the last DQ slice."""
    return N - (p.ns - 1) * p.kslice


# What a shape can make the core do; each takes (p, N, B, d), p the 1vsAll
# plan (KvsAll's plan has the same fields but nsplit and chunk).  The first six
# are the regimes no EDGE_SHAPES entry reaches.
PREDICATES = collections.OrderedDict([
    ("kslice > 32", lambda p, N, B, d: p.kslice > KC),
    ("ns == 1 < chunks", lambda p, N, B, d: p.ns == 1 < _cdiv(N, KC)),
    ("nsplit > 1", lambda p, N, B, d: p.nsplit > 1),
    ("chunk > 1024", lambda p, N, B, d: p.nsplit > 1 and p.chunk > 1024),
    ("nby > 256", lambda p, N, B, d: p.nby > 256),
    ("nbx nby > 256", lambda p, N, B, d: p.nbx * p.nby > 256),
    # a last slice shorter than the others, of several chunks, the last of
    # them short: the k-major staging's clamp to kbeg > 0
    ("ragged last slice", lambda p, N, B, d: p.kslice > KC and p.ns > 1 and
     last_slice(p, N) < p.kslice),
    ("clamp to kbeg > 0", lambda p, N, B, d: p.kslice > KC and p.ns > 1 and
     last_slice(p, N) % KC != 0),
    ("last slice past one chunk", lambda p, N, B, d: p.ns > 1 and KC < last_slice(p, N) and
     last_slice(p, N) % KC != 0),
    ("kslice > N", lambda p, N, B, d: p.kslice > N > KC),
    # k_ova_combine: an element tail in a workgroup with c0 > 0
    ("element tail past chunk 0", lambda p, N, B, d: p.nsplit > 1 and N % 4 != 0),
    ("nbx > 2", lambda p, N, B, d: p.nbx > 2),
    ("ntd > 2", lambda p, N, B, d: p.ntd > 2),
    ("ntd == 8", lambda p, N, B, d: p.ntd == 8),
    ("B == 4096", lambda p, N, B, d: B == 4096),
    ("B > 256", lambda p, N, B, d: B > 256),      # 1vsAll's loss partials: one per query
    ("d == 1024", lambda p, N, B, d: d == 1024),  # s_dq full
    ("odd d", lambda p, N, B, d: d % 2 == 1),
    ("d & 3 == 1", lambda p, N, B, d: d & 3 == 1),
    ("unaligned rows at ntd == 8", lambda p, N, B, d: d & 3 != 0 and p.ntd == 8),
    ("d & 3 == 3", lambda p, N, B, d: d & 3 == 3),
    ("last dimension tile 3 wide", lambda p, N, B, d: p.ntd > 1 and d % TILE == 3),
])
GAP = list(PREDICATES)[:6]


# ---- cases shared by the CPU and the GPU tests ----

def split_ids(N, M, B, d):
    """The entity ids at the seams of 1vsAll's column split, most telling
    first; none when one workgroup rewrites a query's whole row.  chunk starts
    workgroup 1, N - 1 ends the last one, chunk - 1 ends workgroup 0, and the
    last id is the first of the last workgroup's element tail (N - 1 itself
    when the tail is one element, none when N is a multiple of 4)."""
    p = plan("onevsall", B, N, M, d)
    if p.nsplit < 2:
        return []
    ids = [p.chunk, N - 1, p.chunk - 1, 0]
    if N % 4 and (N & ~3) not in ids:
        ids.append(N & ~3)
    return ids


def build_case(model, N, M, B, d, seed, integer=False):
    """Tables, queries (directions mixed, relations drawn from the even ids so
    that odd relation rows are named by no query when M > 1) and answers.
    When the sizes allow, the batch holds: a repeated anchor (queries 0 and 1),
    a self-loop answer (query 0 answers with its own anchor), an empty answer
    list (query 2) and an answer list longer than 64 (query 3, N > 64).  Where
    1vsAll splits a score row (split_ids), query 1 -- query 0 of a batch of
    one -- also answers with every one of those ids.
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
    seams = split_ids(N, M, B, d)
    if seams:
        b = 1 if B > 1 else 0
        lists[b] = np.unique(np.concatenate([lists[b], seams]))
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

# Every EDGE_SHAPES entry plans to kslice = 32 with one chunk per slice, one
# k_ova_combine workgroup per query and at most 3 x 2 forward tiles.  These
# reach the rest of the plan: (N, B, d, models, why), why = (the plan's values,
# the PREDICATES the entry is there for), each the smallest shape that does it.
# tests/test_kvsall_ref.py holds every claim against plan().  "last" is
# last_slice.
_BOTH, _DM = MODELS, ("distmult",)
REGIME_SHAPES = [
    (300, 2048, 512, _BOTH, (dict(kslice=96, ns=4, last=12, nbx=16, ntd=4),
     ("kslice > 32", "ragged last slice", "clamp to kbeg > 0", "nbx > 2", "ntd > 2", "B > 256"))),
    (1100, 4096, 2, _BOTH, (dict(kslice=96, ns=12, nbx=32, nby=9),
     ("nbx nby > 256", "kslice > 32", "B == 4096"))),
    (33, 4096, 1024, _BOTH, (dict(kslice=64, ns=1, ntd=8),
     ("ns == 1 < chunks", "kslice > N", "B == 4096", "d == 1024", "ntd == 8"))),
    (1025, 3, 2, _BOTH, (dict(nsplit=2, chunk=516),
     ("nsplit > 1", "element tail past chunk 0"))),
    (2501, 600, 2, _BOTH, (dict(nsplit=2, chunk=1252),
     ("nsplit > 1", "chunk > 1024", "element tail past chunk 0", "B > 256"))),
    (8300, 130, 130, _BOTH, (dict(kslice=96, ns=87, last=44, nsplit=8, chunk=1040, ntd=2),
     ("kslice > 32", "ragged last slice", "clamp to kbeg > 0", "last slice past one chunk",
      "nsplit > 1", "chunk > 1024"))),
    (32801, 2, 2, _BOTH, (dict(nby=257, kslice=96, ns=342, last=65, nsplit=33, chunk=996,
                               wpr=1026),
     ("nby > 256", "nbx nby > 256", "kslice > 32", "last slice past one chunk", "nsplit > 1",
      "element tail past chunk 0"))),
    (200, 5, 1, _DM, (dict(ntd=1), ("odd d", "d & 3 == 1"))),
    (200, 5, 33, _DM, (dict(ntd=1), ("odd d", "d & 3 == 1"))),
    (129, 130, 515, _DM, (dict(ntd=5, nbx=2),
     ("odd d", "d & 3 == 3", "last dimension tile 3 wide", "ntd > 2"))),
    (200, 5, 1022, _BOTH, (dict(ntd=8), ("ntd == 8", "unaligned rows at ntd == 8"))),
    (200, 5, 1024, _BOTH, (dict(ntd=8), ("ntd == 8", "d == 1024"))),
]
# for the exact zero-relation test only: B a power of two at the two large-N
# regimes whose B above is not (or that it may run at one query)
EXACT_EXTRA_SHAPES = [(32768 + 33, 1, 2, _BOTH), (8300, 128, 130, _BOTH)]
# the benchmark's shape (WN18, B = 512): in the plan tests only
BENCH_SHAPE = (40943, 512, 200)
BENCH_M = 18


def regime_id(s):
    return "N%d-B%d-d%d" % s[:3]


def plan_grid():
    """(B, N, M, d) at which plan() is held against the library: every shape
    of the suites, the benchmark's, and both sides of the plan's thresholds."""
    grid = [(B, N, EDGE_M, d) for N, B, d in EDGE_SHAPES]
    grid += [(s[1], s[0], EDGE_M, s[2]) for s in REGIME_SHAPES + EXACT_EXTRA_SHAPES]
    grid.append((BENCH_SHAPE[1], BENCH_SHAPE[0], BENCH_M, BENCH_SHAPE[2]))
    # chunks either side of ceil(512 / tiles), tiles = 1, 3 and 4
    for B, d in ((128, 128), (300, 8), (130, 130)):
        c = _cdiv(512, _cdiv(B, TILE) * _cdiv(d, TILE))
        grid += [(B, N, 1, d) for N in (KC * (c - 1), KC * c - 1, KC * c, KC * c + 1,
                                        KC * (c + 1), KC * 2 * c, KC * 2 * c + 1)]
    # B d 4 either side of 8 MB and up to 16 MB (B and d at their limits)
    for B, d in ((4096, 1024), (4095, 1024), (4096, 1022), (2047, 1024), (2048, 1024),
                 (2049, 1024), (4096, 510), (4096, 512), (4096, 514), (1366, 1024), (1365, 1024)):
        grid += [(B, N, EDGE_M, d) for N in (33, 100, 300)]
    # N either side of 1024 and 2048, B either side of 1024 (and of 512, 342)
    for N in (1023, 1024, 1025, 2047, 2048, 2049, 5000):
        grid += [(B, N, EDGE_M, 2) for B in (1, 3, 341, 342, 343, 511, 512, 513, 600, 1023, 1024,
                                             1025)]
    return grid
