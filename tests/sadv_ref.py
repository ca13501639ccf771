"""Self-adversarial negative-sampling loss in float64: the restatement the
device is compared with (tests/test_gpu_sadv.py), judged on the CPU by
tests/test_sadv_ref.py.  Written from the definition; it
shares no code with the library (RotatE's score and directions come from
tests/rotate_ref.py).

A positive (s, o, p) has K slots; slot k corrupts position modes[k % nmodes]
(0: s, 1: o, 2: p) with the id it holds, -1: the slot is absent.

  L_j   = -log sigmoid(gamma + phi_pos) - sum_k w_k log sigmoid(-(gamma + phi_k))
  w_k   = softmax over the valid slots of alpha phi_k; a constant in the gradient
  c_pos = -sigmoid(-(gamma + phi_pos))      c_k = w_k sigmoid(gamma + phi_k)

Each of the 1 + Kv triples contributes c * d phi / d row to its rows s, o and p
and is one occurrence of each; a row's gradient is the mean over its
occurrences; SGD or AdaGrad; then the projections.  The directions are the
library's convention: TransE-L1 -sign(v), TransE-L2 -v (the reference's
difference, without the factor 2), v = E_s + R_p - E_o, for s and p and the
negation for o; RotatE rotate_ref.triple_grads.

Beside each gradient row stands its ROUNDING BOUND (derived, not tuned):
  tol_phi = ATOL + RTOL |phi|                       a score's bar (parity_util)
  dc_k    = RTOL |c_k| + (1 + 2 alpha) |c_k| max_k' tol_phi_k'
            since |d c_k / d phi_k| <= (1 + alpha) c_k and
            sum_j |d c_k / d phi_j| <= alpha c_k;  c_pos: factor 1, its own phi
  eps     = GRAD_ROUNDING + ROW_ULPS rownorm + segment_mean(|direction| dc)
"""
import numpy as np

import rotate_ref as RR
from parity_util import (ATOL, FLIP_ROWS_FRAC, FLIP_ROWS_MIN, FLIPS, GRAD_ROUNDING, RECORDS, ROW_ULPS,
                         RTOL, headroom)

FORMS = ("l1", "l2", "rot")


def phi(form, E, R, trip):
    trip = np.asarray(trip, dtype=np.int64).reshape(-1, 3)
    if form == "rot":
        return RR.scores(E, R, trip)
    v = E[trip[:, 0]] + R[trip[:, 2]] - E[trip[:, 1]]
    return -np.abs(v).sum(axis=1) if form == "l1" else -(v * v).sum(axis=1)


def dirs(form, E, R, trip):
    """(d phi / d E_s, d phi / d E_o, d phi / d R_p) rows [n][d], library convention."""
    trip = np.asarray(trip, dtype=np.int64).reshape(-1, 3)
    if form == "rot":
        return RR.triple_grads(E, R, trip)
    v = E[trip[:, 0]] + R[trip[:, 2]] - E[trip[:, 1]]
    h = -np.sign(v) if form == "l1" else -v
    return h, -h, h


def nls(x):
    """-log sigmoid(x), stable."""
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def slot_triples(pos, negK, modes):
    """neg [P][K][3] (an absent slot keeps the positive's ids) and valid [P][K]."""
    pos = np.asarray(pos, dtype=np.int64).reshape(-1, 3)
    negK = np.asarray(negK, dtype=np.int64).reshape(len(pos), -1)
    K = negK.shape[1]
    neg = np.repeat(pos[:, None, :], K, axis=1)
    valid = negK >= 0
    for k in range(K):
        m = modes[k % len(modes)]
        neg[valid[:, k], k, m] = negK[valid[:, k], k]
    return pos, negK, neg, valid


def weights(nphi, valid, alpha):
    """Stable softmax of alpha * phi over the valid slots of each row; 0 elsewhere."""
    a = np.where(valid, alpha * nphi, -np.inf)
    m = np.max(a, axis=1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    e = np.where(valid, np.exp(np.where(valid, a - m, 0.0)), 0.0)
    Z = e.sum(axis=1, keepdims=True)
    return np.where(valid, e / np.where(Z > 0, Z, 1.0), 0.0)


def forward(form, E, R, pos, negK, modes, gamma, alpha):
    pos, negK, neg, valid = slot_triples(pos, negK, modes)
    P, K = negK.shape
    pphi = phi(form, E, R, pos)
    nphi = np.where(valid, phi(form, E, R, neg.reshape(-1, 3)).reshape(P, K), 0.0)
    w = weights(nphi, valid, alpha)
    cpos = -sigmoid(-(gamma + pphi))
    cneg = np.where(valid, w * sigmoid(gamma + nphi), 0.0)
    Lj = nls(gamma + pphi) + np.where(valid, w * nls(-(gamma + nphi)), 0.0).sum(axis=1)
    # the coefficients' rounding bounds
    tol_p = ATOL + RTOL * np.abs(pphi)
    tol_n = np.where(valid, ATOL + RTOL * np.abs(nphi), 0.0).max(axis=1, keepdims=True)
    dcpos = RTOL * np.abs(cpos) + np.abs(cpos) * tol_p
    dcneg = RTOL * np.abs(cneg) + (1.0 + 2.0 * alpha) * np.abs(cneg) * tol_n
    return dict(pos=pos, negK=negK, neg=neg, valid=valid, pphi=pphi, nphi=nphi, w=w, cpos=cpos,
                cneg=cneg, Lj=Lj, loss=float(Lj.sum()), dcpos=dcpos, dcneg=dcneg)


def loss_one(form, E, R, pos1, negK1, modes, gamma, w_fixed, dphi=None):
    """L_j of one positive with the weights held fixed and the scores shifted by
    dphi [1 + K] (finite differences of d L / d phi)."""
    fw = forward(form, E, R, pos1, negK1, modes, gamma, 0.0)
    d = np.zeros(1 + fw["negK"].shape[1]) if dphi is None else np.asarray(dphi, dtype=np.float64)
    pphi, nphi = fw["pphi"][0] + d[0], fw["nphi"][0] + d[1:]
    v = fw["valid"][0]
    return float(nls(gamma + pphi) + np.where(v, w_fixed * nls(-(gamma + nphi)), 0.0).sum())


def segment_mean(rows, ids):
    ids = np.asarray(ids, dtype=np.int64)
    uniq, inv = np.unique(ids, return_inverse=True)
    g = np.zeros((len(uniq), rows.shape[1]))
    np.add.at(g, inv, rows)
    cnt = np.bincount(inv, minlength=len(uniq)).astype(np.float64)
    return g / cnt[:, None], uniq, cnt


def gradients(form, E, R, pos, negK, modes, gamma, alpha):
    """fw, {pid: (mean gradient rows, sorted unique ids, eps rows, counts)}."""
    fw = forward(form, E, R, pos, negK, modes, gamma, alpha)
    v = fw["valid"].reshape(-1)
    trips = np.concatenate([fw["pos"], fw["neg"].reshape(-1, 3)[v]])
    c = np.concatenate([fw["cpos"], fw["cneg"].reshape(-1)[v]])
    dc = np.concatenate([fw["dcpos"], fw["dcneg"].reshape(-1)[v]])
    Ds, Do, Dp = dirs(form, E, R, trips)
    out = {}
    for pid, rows, ids in (("E", np.concatenate([Ds, Do]),
                            np.concatenate([trips[:, 0], trips[:, 1]])),
                           ("R", Dp, trips[:, 2])):
        cc = np.concatenate([c, c]) if pid == "E" else c
        dd = np.concatenate([dc, dc]) if pid == "E" else dc
        g, idx, cnt = segment_mean(cc[:, None] * rows, ids)
        bound, _, _ = segment_mean(dd[:, None] * np.abs(rows), ids)
        rown = np.sqrt((g ** 2).sum(axis=1))
        eps = GRAD_ROUNDING + ROW_ULPS * rown[:, None] + bound
        out[pid] = (g, idx, eps, cnt)
    return fw, out


def update(P, state, g, idx, lr, opt):
    if opt == "adagrad":
        state[idx] += g * g
        P[idx] -= lr * g / np.maximum(np.sqrt(state[idx]), 1e-7)
    else:
        P[idx] -= lr * g


def posts(form):
    return {"E": "normalize", "R": "unitmod" if form == "rot" else None}


def step(form, params, state, pos, negK, modes, gamma, alpha, lr, opt):
    """One batch in place on params / state ({'E', 'R'} float64).  Returns fw,
    the gradients and, per table, the rows before the projection."""
    fw, grads = gradients(form, params["E"], params["R"], pos, negK, modes, gamma, alpha)
    pre = {}
    for pid in ("E", "R"):
        g, idx = grads[pid][0], grads[pid][1]
        update(params[pid], state[pid], g, idx, lr, opt)
        pre[pid] = params[pid][idx].copy()
    RR.normalize_rows(params["E"], grads["E"][1])
    if form == "rot":
        RR.unitmod_rows(params["R"], grads["R"][1])
    return fw, grads, pre


# ---- checks (every one appends its headroom to parity_util.RECORDS) ----

def _record(got, want, tol, what):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == np.shape(want), (what, got.shape, np.shape(want))
    assert np.all(np.isfinite(got)), what + ": not finite"
    h, emax = headroom(got, want, tol)
    RECORDS.append((what, h, emax, int(got.size)))
    if not h >= 1.0:
        bad = np.abs(got - want) > tol
        raise AssertionError("%s: %d of %d elements past the bound, headroom %.3g, max |err| %.3g"
                             % (what, int(bad.sum()), got.size, h, emax))
    return h


def check_scores(got, want, what):
    return _record(got, want, ATOL + RTOL * np.abs(want), what)


def check_coef(got_coef, fw, what):
    """coef [P][1 + K] against (c_pos, c_k) within (dc_pos, dc_k) (+ ATOL * 0)."""
    want = np.concatenate([fw["cpos"][:, None], fw["cneg"]], axis=1)
    tol = np.concatenate([fw["dcpos"][:, None], fw["dcneg"]], axis=1)
    return _record(got_coef, want, tol + 1e-30, what)


def check_rows(got_g, got_idx, grad, what):
    g, idx, eps, _ = grad
    assert np.array_equal(np.asarray(got_idx, dtype=np.int64), idx), what + ": touched ids"
    return _record(got_g, g, eps, what)


def check_param(got, want, before, grad, pre, state_after, lr, opt, post, what, flips=0):
    """A table after the step.  Per element
        a   = min(lr eps / H, 2 lr) (AdaGrad, H = max(sqrt(state), 1e-7)) or lr eps (SGD)
        tol = ATOL + RTOL |want| + a (+ the projection's share of a)
    normalize: + |want| dss / (2 ss), dss = sum over the row of 2 |pre| a + a^2
    (parity_util.check_step's term); unitmod: a component z / |z| moves by at
    most 2 |dz| / |z|, |dz| = the 2-norm of its two elements' a.  The rows whose
    error passes the plain ATOL + RTOL |want| bar are counted, recorded in
    parity_util.FLIPS and may be at most `flips`: 0 for every case whose tables
    meet the input conditions (no sign is ever in doubt); None for a step from
    tables that an earlier step has moved off the conditions' grid (the device
    loop's batches after the first), where a TransE-L1 component near 0 or a
    RotatE modulus near 0 may be decided differently in fp32 and fp64 -- there
    the ceiling is parity_util.check_step's own, max(FLIP_ROWS_MIN,
    ceil(FLIP_ROWS_FRAC * touched rows)), the project's bar for every other
    replayed epoch."""
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    g, idx, eps, _ = grad
    tol = ATOL + RTOL * np.abs(want)
    if opt == "adagrad":
        H = np.maximum(np.sqrt(np.asarray(state_after, dtype=np.float64)[idx]), 1e-7)
        a = np.minimum(lr * eps / H, 2.0 * lr)
    else:
        a = lr * eps
    if post == "normalize":
        ss = (pre ** 2).sum(axis=1)
        dss = (2.0 * np.abs(pre) * a + a * a).sum(axis=1)
        add = a + np.abs(want[idx]) * (dss / (2.0 * np.maximum(ss, 1e-30)))[:, None]
    elif post == "unitmod":
        dz = np.sqrt(a[:, 0::2] ** 2 + a[:, 1::2] ** 2)
        mz = np.abs(RR.cplx(pre))
        add = np.repeat(2.0 * dz / np.maximum(mz, 1e-30), 2, axis=1)
    else:
        add = a
    tol[idx] += add
    h = _record(got, want, tol, what)
    untouched = np.ones(len(want), dtype=bool)
    untouched[idx] = False
    assert np.array_equal(got[untouched], np.asarray(before, dtype=np.float64)[untouched]), \
        what + ": an untouched row changed"
    nflip = int((np.abs(got - want) > ATOL + RTOL * np.abs(want)).any(axis=1).sum())
    allowed = flips if flips is not None else max(FLIP_ROWS_MIN,
                                                  int(np.ceil(FLIP_ROWS_FRAC * len(idx))))
    FLIPS.append((what, nflip, len(idx), allowed))
    assert nflip <= allowed, "%s: %d rows past the plain bar (at most %d)" % (what, nflip, allowed)
    return h


# ---- cases: chosen here on the CPU, never from a device result ----
N, M, P = 48, 4, 24
WIDTHS_TRANSE = (1, 8, 50, 64, 65, 130, 200, 257, 514, 1024)
WIDTHS_ROT = (2, 8, 50, 66, 130, 200, 258, 514, 1024)
SLOTS = ((1, (0,)), (3, (0, 1, 2)), (6, (1, 0, 0)), (64, (0, 1)))
WIDE_K_WIDTHS = (8, 200)          # K = 64 runs at these widths only
GAMMAS, ALPHAS = (0.0, 6.0), (0.0, 1.0)
PHI_MIN = -12.0
MOD_MIN = 1e-3
ROT_SCALES = (1.0, 0.5, 0.25, 0.2, 0.1, 0.05)
ODD_RANGES = (64, 32, 16, 8, 4, 2, 1)


def records(K, modes, seed, n_ent=N, n_rel=M, n_pos=P):
    """pos [P][3], negK [P][K]: random ids, about one slot in eight absent
    (K >= 3), no negative equal to its positive."""
    rs = np.random.RandomState(seed)
    pos = np.stack([rs.randint(n_ent, size=n_pos), rs.randint(n_ent, size=n_pos),
                    rs.randint(n_rel, size=n_pos)], axis=1)
    negK = np.empty((n_pos, K), dtype=np.int64)
    for k in range(K):
        m = modes[k % len(modes)]
        rng = n_rel if m == 2 else n_ent
        c = rs.randint(rng, size=n_pos)
        c = np.where(c == pos[:, m], (c + 1) % rng, c)
        negK[:, k] = c
    if K >= 3:
        negK[rs.uniform(size=negK.shape) < 0.125] = -1
    return pos.astype(np.int64), negK


def case_triples(pos, negK, modes):
    pos, negK, neg, valid = slot_triples(pos, negK, modes)
    return np.concatenate([pos, neg.reshape(-1, 3)[valid.reshape(-1)]])


def transe_tables(form, d, trips, seed, n_ent=N, n_rel=M):
    """E on odd multiples of 2^-7, R on odd multiples of 2^-8: every component
    of E_s + R_p - E_o is an odd multiple of 2^-8 (never 0: no sign in doubt)
    and phi is exact in fp32 (L1: < 2^12 multiples of 2^-8 below 16; L2: squares
    are multiples of 2^-16 and the sum stays below 16, 20 bits).  The widest odd
    range that keeps every phi of the case in [PHI_MIN, 0]."""
    for A in ODD_RANGES:
        rs = np.random.RandomState(seed)
        E = (2 * rs.randint(-A, A, size=(n_ent, d)) + 1) * 2.0 ** -7
        R = (2 * rs.randint(-A, A, size=(n_rel, d)) + 1) * 2.0 ** -8
        if phi(form, E, R, trips).min() >= PHI_MIN:
            return E, R
    raise AssertionError("no TransE tables for %s d = %d" % (form, d))


def min_modulus(E, R, trips):
    u = RR.cplx(E[trips[:, 0]]) * RR.cplx(R[trips[:, 2]]) - RR.cplx(E[trips[:, 1]])
    return np.abs(u)


def rot_tables(d, trips, seed, n_ent=N, n_rel=M):
    """rotate_ref.tables (fp32-held) at the largest scale that keeps every phi of
    the case in [PHI_MIN, 0]; then every component of a subject row that leaves a
    modulus of the case below 1.5 MOD_MIN is drawn again (a Gaussian of the
    row's component size; for a triple with s == o the relation's phase too),
    until none is left.  The caller asserts the floor."""
    for scale in ROT_SCALES:
        E, R = RR.tables(n_ent, n_rel, d, seed, scale)
        if RR.scores(E, R, trips).min() >= PHI_MIN:
            break
    else:
        raise AssertionError("no RotatE scale for d = %d" % d)
    rs = np.random.RandomState(seed + 7)
    sigma = scale / np.sqrt(d)
    for _ in range(200):
        m = min_modulus(E, R, trips)
        t, j = np.nonzero(m < 1.5 * MOD_MIN)
        if len(t) == 0:
            return E, R
        for ti, ji in zip(t, j):
            e, o, p = trips[ti]
            E[e, 2 * ji:2 * ji + 2] = rs.normal(0.0, sigma, 2).astype(np.float32)
            if e == o:   # |s_j| |r_j - 1|: the phase is what is small
                th = rs.uniform(0.5, np.pi)
                R[p, 2 * ji:2 * ji + 2] = np.array([np.cos(th), np.sin(th)], dtype=np.float32)
    raise AssertionError("RotatE moduli stay below the floor, d = %d" % d)


def step_cases():
    """(form, d, K, modes) of the step-parity test."""
    out = []
    for form in FORMS:
        for d in (WIDTHS_ROT if form == "rot" else WIDTHS_TRANSE):
            for K, modes in SLOTS:
                if K == 64 and d not in WIDE_K_WIDTHS:
                    continue
                out.append((form, d, K, modes))
    return out


def case_seed(form, d, K):
    return 1000 * FORMS.index(form) + 7 * d + K


def build_case(form, d, K, modes):
    """(E, R, pos, negK, gamma, alpha) of one step case; gamma and alpha cycle
    through GAMMAS x ALPHAS with the case's seed."""
    seed = case_seed(form, d, K)
    pos, negK = records(K, modes, seed)
    trips = case_triples(pos, negK, modes)
    if form == "rot":
        E, R = rot_tables(d, trips, seed)
    else:
        E, R = transe_tables(form, d, trips, seed)
    gamma = GAMMAS[seed % 2]
    alpha = ALPHAS[(seed // 2) % 2]
    return E, R, pos, negK, gamma, alpha


def check_conditions(form, E, R, pos, negK, modes):
    """The input conditions of the GPU cases (asserted, on the CPU)."""
    trips = case_triples(pos, negK, modes)
    ph = phi(form, E, R, trips)
    assert ph.min() >= PHI_MIN and ph.max() <= 0.0, (form, ph.min(), ph.max())
    assert np.array_equal(E.astype(np.float32).astype(np.float64), E)
    assert np.array_equal(R.astype(np.float32).astype(np.float64), R)
    if form == "rot":
        assert min_modulus(E, R, trips).min() >= MOD_MIN, min_modulus(E, R, trips).min()
    else:
        e, r = E * 2.0 ** 7, R * 2.0 ** 8
        assert np.array_equal(e, np.rint(e)) and np.all(np.abs(e) % 2 == 1)
        assert np.array_equal(r, np.rint(r)) and np.all(np.abs(r) % 2 == 1)
        v = (E[trips[:, 0]] + R[trips[:, 2]] - E[trips[:, 1]]) * 2.0 ** 8
        assert np.all(np.abs(v) % 2 == 1)
        assert np.array_equal(ph.astype(np.float32).astype(np.float64), ph)


def adagrad_state(shape, seed):
    """Nonzero AdaGrad state in [0.5, 1.5], held in fp32."""
    rs = np.random.RandomState(seed + 99)
    return rs.uniform(0.5, 1.5, shape).astype(np.float32).astype(np.float64)


# ---- edge cases: hand-built records (n_ent = N); a record carries its n_rel ----
EDGE_WIDTHS = (8, 200)


def edge_records():
    """name -> (pos, negK, modes, n_rel)."""
    one_pos, one_neg = records(3, (0, 1, 2), 77, n_rel=1, n_pos=7)
    one_neg[:, 2] = np.where(one_neg[:, 2] >= 0, 0, -1)   # the only relation there is
    out = {
        "absent slot": ([[1, 2, 0], [3, 4, 1]], [[5, -1, 6], [-1, 7, 8]], (0, 1, 0), M),
        "all absent": ([[1, 2, 0], [3, 4, 1]], [[-1, -1], [-1, -1]], (0, 1), M),
        "c==o mode 0, c==s mode 1": ([[1, 2, 0], [3, 4, 1]], [[2, 1], [4, 3]], (0, 1), M),
        "one id in two slots": ([[1, 2, 0]], [[9, 9, 9, 10]], (0, 0, 1, 1), M),
        "o==s": ([[5, 5, 2], [6, 6, 1]], [[7, 8], [5, 6]], (0, 1), M),
        "mode 2 neighbour row": ([[1, 2, 1], [3, 4, 2]], [[2, 0], [3, 1]], (2, 2), M),
        "P=1": ([[10, 11, 3]], [[12, 13, 0]], (0, 1, 2), M),
        "P=5": ([[i, i + 1, i % 4] for i in range(5)],
                [[i + 7, i + 9, (i + 1) % 4] for i in range(5)], (0, 1, 2), M),
        "one relation row": (one_pos, one_neg, (0, 1, 2), 1),
    }
    return {k: (np.array(v[0]), np.array(v[1]), v[2], v[3]) for k, v in out.items()}


def edge_case(form, d, name):
    """(E, R, pos, negK, modes, n_rel) of one edge case."""
    pos, negK, modes, n_rel = edge_records()[name]
    trips = case_triples(pos, negK, modes)
    seed = 50 + d
    E, R = (rot_tables(d, trips, seed, n_rel=n_rel) if form == "rot"
            else transe_tables(form, d, trips, seed, n_rel=n_rel))
    return E, R, pos, negK, modes, n_rel


# ---- the device loop: its records are drawn on the device, so the initial
# tables meet the input conditions on EVERY triple of N x N x M ----
LOOP_WIDTHS = (8, 200)


def all_triples(n_ent=N, n_rel=M):
    s, o, p = np.meshgrid(np.arange(n_ent), np.arange(n_ent), np.arange(n_rel), indexing="ij")
    return np.stack([s.ravel(), o.ravel(), p.ravel()], axis=1)


def loop_tables(form, d):
    trips = all_triples()
    seed = 300 + d
    return rot_tables(d, trips, seed) if form == "rot" else transe_tables(form, d, trips, seed)


def check_conditions_on(form, E, R, trips):
    """check_conditions over explicit triples (s, o, p)."""
    n = len(trips)
    check_conditions(form, E, R, trips, np.full((n, 1), -1), (0,))
