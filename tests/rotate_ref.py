"""RotatE in float64: the restatement the device is compared with
(tests/test_gpu_rotate.py, tests/test_gpu_rotate_exact.py).

Rows hold d/2 complex components interleaved, (re, im) = (x[2j], x[2j + 1]).

  phi(s, p, o) = -sum_j |E_s[j] * R_p[j] - E_o[j]|

With u = s * r - o, m = |u|, w = u / m (w = 0 where m == 0, like sign(0)):
  d phi / d s = -conj(r) * w     d phi / d o = +w     d phi / d r = -conj(s) * w
The loss is TransE's raw pairwise margin: a pair violates when
nscore + margin > pscore (strict); a violating pair contributes the gradient
of -phi_pos and of +phi_neg; entity list (sp, op, sn, on), relation list
(pp, pn); mean over occurrences; SGD or AdaGrad; then the projections
(E: unit rows, R: unit-modulus components)."""
import numpy as np

U = 2.0 ** -24


def cplx(x):
    """[..., d] interleaved floats -> [..., d/2] complex128."""
    x = np.asarray(x, dtype=np.float64)
    return x[..., 0::2] + 1j * x[..., 1::2]


def inter(z):
    """[..., d/2] complex -> [..., d] interleaved float64."""
    out = np.empty(z.shape[:-1] + (2 * z.shape[-1],), dtype=np.float64)
    out[..., 0::2] = z.real
    out[..., 1::2] = z.imag
    return out


def scores(E, R, trip):
    """phi of triples (s, o, p) [n][3]."""
    trip = np.asarray(trip).reshape(-1, 3)
    u = cplx(E[trip[:, 0]]) * cplx(R[trip[:, 2]]) - cplx(E[trip[:, 1]])
    return -np.abs(u).sum(axis=1)


def unit(u):
    m = np.abs(u)
    return np.where(m > 0, u / np.where(m > 0, m, 1.0), 0.0)


def triple_grads(E, R, trip):
    """(d phi / d s, d phi / d o, d phi / d r) rows [n][d] of triples (s, o, p)."""
    trip = np.asarray(trip).reshape(-1, 3)
    s, o, r = cplx(E[trip[:, 0]]), cplx(E[trip[:, 1]]), cplx(R[trip[:, 2]])
    w = unit(s * r - o)
    return inter(-np.conj(r) * w), inter(w), inter(-np.conj(s) * w)


def segment_mean(rows, ids, width):
    """grad_sum_matrix + the mean: sorted unique ids and the mean of their rows."""
    ids = np.asarray(ids, dtype=np.int64)
    uniq, inv = np.unique(ids, return_inverse=True)
    g = np.zeros((len(uniq), width))
    np.add.at(g, inv, rows)
    cnt = np.bincount(inv, minlength=len(uniq)).astype(np.float64)
    return g / cnt[:, None], uniq


def pairwise_gradients(E, R, pos, neg, margin):
    """pscore, nscore, nviol, {pid: (mean gradient rows, sorted unique ids)} or None."""
    pos, neg = np.asarray(pos).reshape(-1, 3), np.asarray(neg).reshape(-1, 3)
    ps, ns = scores(E, R, pos), scores(E, R, neg)
    viol = ns + margin > ps
    nv = int(viol.sum())
    if nv == 0:
        return ps, ns, 0, None
    p, n = pos[viol], neg[viol]
    gs_p, go_p, gr_p = triple_grads(E, R, p)
    gs_n, go_n, gr_n = triple_grads(E, R, n)
    d = E.shape[1]
    # entity list (sp, op, sn, on), relation list (pp, pn)
    ge = np.concatenate([-gs_p, -go_p, gs_n, go_n])
    ie = np.concatenate([p[:, 0], p[:, 1], n[:, 0], n[:, 1]])
    gr = np.concatenate([-gr_p, gr_n])
    ir = np.concatenate([p[:, 2], n[:, 2]])
    return ps, ns, nv, {"E": segment_mean(ge, ie, d), "R": segment_mean(gr, ir, d)}


def normalize_rows(M, idx):
    M[idx] = M[idx] / np.sqrt((M[idx] ** 2).sum(axis=1))[:, None]


def unitmod_rows(M, idx=None):
    """Every component of rows idx divided by its modulus; (0, 0) -> (1, 0)."""
    rows = M if idx is None else M[idx]
    z = cplx(rows)
    m = np.abs(z)
    z = np.where(m > 0, z / np.where(m > 0, m, 1.0), 1.0 + 0.0j)
    if idx is None:
        return inter(z)
    M[idx] = inter(z)
    return M


def update(P, state, g, idx, lr, opt):
    if opt == "adagrad":
        state[idx] += g * g
        P[idx] -= lr * g / np.maximum(np.sqrt(state[idx]), 1e-7)
    else:
        P[idx] -= lr * g


def pairwise_step(params, state, pos, neg, lr, margin, opt):
    """One batch in place on params / state ({'E', 'R'} float64).  Returns
    pscore, nscore, nviol, the gradients."""
    ps, ns, nv, grads = pairwise_gradients(params["E"], params["R"], pos, neg, margin)
    if nv:
        for pid in ("E", "R"):
            g, idx = grads[pid]
            update(params[pid], state[pid], g, idx, lr, opt)
        normalize_rows(params["E"], grads["E"][1])
        unitmod_rows(params["R"], grads["R"][1])
    return ps, ns, nv, grads


def init(N, M, d, seed):
    """RotatE(sz, d)'s tables from numpy's global RNG seeded with `seed`:
    init_nunif E with unit rows, then the phases of R."""
    np.random.seed(seed)
    bnd = np.sqrt(6) / np.sqrt(N + d)
    E = np.random.uniform(low=-bnd, high=bnd, size=(N, d))
    E = E / np.sqrt((E ** 2).sum(axis=1))[:, None]
    theta = np.random.uniform(-np.pi, np.pi, (M, d // 2))
    R = np.empty((M, d))
    R[:, 0::2] = np.cos(theta)
    R[:, 1::2] = np.sin(theta)
    return E, R


def tables(N, M, d, seed, scale):
    """Test tables held in fp32: E rows of norm `scale`, R on the unit circle."""
    rs = np.random.RandomState(seed)
    E = rs.uniform(-1, 1, (N, d))
    E = scale * E / np.sqrt((E ** 2).sum(axis=1))[:, None]
    th = rs.uniform(-np.pi, np.pi, (M, d // 2))
    R = np.empty((M, d))
    R[:, 0::2], R[:, 1::2] = np.cos(th), np.sin(th)
    return E.astype(np.float32).astype(np.float64), R.astype(np.float32).astype(np.float64)


def pairs(N, M, P, seed):
    """P pairs (s, o, p): corrupt-s, corrupt-o and corrupt-p negatives, with
    coinciding ids (sp == sn, op == on, s == o, pp != pn)."""
    rs = np.random.RandomState(seed)
    pos = np.stack([rs.randint(N, size=P), rs.randint(N, size=P), rs.randint(M, size=P)], axis=1)
    neg = pos.copy()
    for i in range(P):
        k = i % 4
        if k == 0:
            neg[i, 0] = rs.randint(N)
        elif k == 1:
            neg[i, 1] = rs.randint(N)
        elif k == 2:
            neg[i, 2] = rs.randint(M)
        else:
            neg[i] = (rs.randint(N), rs.randint(N), rs.randint(M))
    pos[0, 1] = pos[0, 0]          # s == o
    return pos.astype(np.int64), neg.astype(np.int64)


def km_for(d):
    for lim, km in ((64, 1), (128, 2), (192, 3), (256, 4), (512, 8), (1024, 16)):
        if d <= lim:
            return km
    raise ValueError(d)


def score_error_bound(E, R, trip):
    """Worst-case fp32 error of the device score of each triple.  Per component,
    each half of u = s * r - o is an fma, a multiply and a subtraction of terms
    no larger than |s_j| |r_j| and |o_j|: |du| <= 3 U (|s_j| |r_j| + |o_j|) per
    half, sqrt(2) of it on the modulus; the modulus itself (fma, multiply,
    sqrt) adds 2 U m_j; the sum is KM adds per lane and 6 + 2 levels of the wave
    tree, (KM + 8) U on every term.  Together
        (KM + 10) U sum_j m_j + 3 sqrt(2) U sum_j (|s_j| |r_j| + |o_j|)."""
    trip = np.asarray(trip).reshape(-1, 3)
    s, o, r = cplx(E[trip[:, 0]]), cplx(E[trip[:, 1]]), cplx(R[trip[:, 2]])
    m = np.abs(s * r - o).sum(axis=1)
    a = (np.abs(s) * np.abs(r) + np.abs(o)).sum(axis=1)
    return (km_for(E.shape[1]) + 10) * U * m + 3 * np.sqrt(2) * U * a


# ---- integer-exact helpers (tests/test_gpu_rotate_exact.py) ----

def int_query(E, R, a, p, tail):
    """The query vector of (a, p) over Gaussian-integer tables (int64,
    interleaved): tail a * r, head conj(r) * a."""
    za = E[a, 0::2] + 1j * E[a, 1::2]
    zr = R[p, 0::2] + 1j * R[p, 1::2]
    q = za * zr if tail else np.conj(zr) * za
    out = np.empty(E.shape[1], dtype=np.int64)
    out[0::2] = np.rint(q.real).astype(np.int64)
    out[1::2] = np.rint(q.imag).astype(np.int64)
    return out


def int_moduli(q, E):
    """|q_j - E[e]_j|^2 for every row e, int64 [N][d/2]."""
    t = q[None, :] - E
    return t[:, 0::2] ** 2 + t[:, 1::2] ** 2


def int_scores(q, E):
    """-sum_j |q_j - E[e]_j| for every row e as int64; every modulus must be an
    integer (asserted)."""
    m2 = int_moduli(q, E)
    m = np.rint(np.sqrt(m2.astype(np.float64))).astype(np.int64)
    assert np.array_equal(m * m, m2), "a modulus is not an integer"
    return -m.sum(axis=1)


# ---- the cases of tests/test_gpu_rotate.py: widths, and per width the table
# scale, margin and seed, all chosen here on the CPU (never from a device
# result) and judged by tests/test_rotate_ref.py ----
N, M, P = 64, 4, 64
WIDTHS = (2, 8, 50, 66, 130, 200, 258, 514)   # KM 1, 1, 1, 2, 3, 4, 8, 16
SCALES = (1.0, 0.5, 0.25, 0.2, 0.1, 0.05)
MARGINS = (0.5, 0.2, 0.1, 0.05, 0.02, 0.01, 0.005, 0.002)
ERR_BAR = 5e-6     # half of the 1e-5 parity bar
GAP = 1e-5


def case(d):
    """(E, R, pos, neg, scale, margin, seed) of width d: the largest scale whose
    worst score error bound is <= ERR_BAR, then the first seed and margin with
    20-80% of the pairs violating and no decision within GAP of the margin."""
    for seed in range(d, d + 50):
        pos, neg = pairs(N, M, P, seed)
        for scale in SCALES:
            E, R = tables(N, M, d, 1000 + seed, scale)
            trips = np.concatenate([pos, neg])
            if score_error_bound(E, R, trips).max() <= ERR_BAR:
                break
        else:
            continue
        ps, ns = scores(E, R, pos), scores(E, R, neg)
        for margin in MARGINS:
            gap = ns + margin - ps
            frac = float((gap > 0).mean())
            if 0.2 <= frac <= 0.8 and np.abs(gap).min() > GAP:
                return E, R, pos, neg, scale, margin, seed
    raise AssertionError("no case for d = %d" % d)
