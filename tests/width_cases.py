"""The shapes at which the per-batch step kernels are compared with the oracle
so that every row-width layout is reached (tests/test_gpu_widths.py), as data,
with a plain-Python restatement of the library's selection rules.

A row of width d lives in KM = km_for(d) registers per lane; every per-batch
kernel is instantiated per KM and picked by a host switch, and HolE and RESCAL
pick among several kernels by d, the relation count and the batch size.  Each
case names the path (skge_step_path's SKGE_PATH_*) and the KM it is meant to
reach: tests/test_width_cases.py (CPU) holds the restated rules to that claim
and the GPU tests hold the library's own skge_step_path to it, so a threshold
that moves cannot silently move a case onto a path another case covers.

Batches: test_gpu_models._batch on RandomState(5) (pairs) / RandomState(9)
(logistic), models seeded with 3 -- what test_gpu_models._run draws.  Margins
are chosen per model and width so that the first batch has both violating and
non-violating pairs (asserted on the CPU); P is the largest of a few hundred
for which one oracle step stays well under 2 s on the CPU (RESCAL's oracle
gathers a d x d matrix per triple: 8 P d^2 bytes per gather).
"""
from collections import namedtuple

import numpy as np

# ---------------------------------------------------------------------------
# the library's selection rules, restated (csrc/skge_host.h, skge_grad.hip,
# skge_hole_fft.h, skge_rescal.hip, skge_update.hip)
# ---------------------------------------------------------------------------
GENERIC, HOLE_FAST, HOLE_FFT, RESCAL_MFMA_SMALL, RESCAL_MFMA_SORT, RESCAL_VALU = range(6)
PATH_NAMES = ["generic", "hole-fast", "hole-fft", "rescal-mfma-small-bucket",
              "rescal-mfma-sort", "rescal-valu"]

RS_MAX_D, RS_MAX_M = 1024, 8192      # the MFMA path
SB_MAXM, SB_MAXN = 256, 1024         # k_rs_bucket_small
RS_COUNT_OWN_ROWS_M = 64             # above it rescal_front clears the chunk counts itself
WS_TILE, WS_GROUP, WG_SPLIT = 64, 128, 8


def km_for(d):
    for top, km in ((64, 1), (128, 2), (192, 3), (256, 4), (512, 8), (1024, 16)):
        if d <= top:
            return km
    return 0


def hole_fast(d):
    return d % 4 == 0 and 4 <= d <= 256


def hole_fft_ok(d):
    if d % 4 != 0 or d < 4 or d // 4 + 1 > 64:
        return False
    m = d // 2
    for r in (2, 3, 4, 5):
        while m % r == 0:
            m //= r
    return m == 1


def rescal_mfma_ok(d, n_rel):
    return 1 <= d <= RS_MAX_D and 1 <= n_rel <= RS_MAX_M


def rs_small_bucket(n_rel, n):
    return n_rel <= SB_MAXM and n <= SB_MAXN


def rs_memset_branch(n_rel, n):
    """rescal_front clears the per-chunk counts before k_rs_count."""
    return not rs_small_bucket(n_rel, n) and n_rel > RS_COUNT_OWN_ROWS_M


def rs_scan_lds_bytes(n_rel):
    return (2 * n_rel + 1) * 4


def rs_wsplit(n, n_rel, d):
    """split-K count of the dW tiles (1: the single fused dW kernel)."""
    nt = (d + WS_TILE - 1) // WS_TILE
    groups = (n // n_rel + WS_GROUP - 1) // WS_GROUP
    sp = 1 if groups < 4 else min(WG_SPLIT, groups)
    while sp > 1 and n_rel * nt * nt * sp * WS_TILE * WS_TILE * 4 > (64 << 20):
        sp -= 1
    return max(sp, 1)


def generic_lds_bytes(km):
    """dynamic LDS of k_pair_grad / k_triple_grad for HolE and RESCAL: four
    waves of six rows of 64 KM floats."""
    return 4 * 6 * 64 * km * 4


def step_path(model, mode, d, n_rel, n_items):
    """(path, KM) of one skge_pair_step (n_items = P) / skge_triple_step (T)."""
    km = km_for(d)
    if model == "hole":
        if not (km <= 4 and hole_fast(d)):
            return GENERIC, km
        return (HOLE_FFT if hole_fft_ok(d) else HOLE_FAST), km
    if model == "rescal":
        n = n_items if mode == "logistic" else 2 * n_items
        if not rescal_mfma_ok(d, n_rel):
            return RESCAL_VALU, km
        return (RESCAL_MFMA_SMALL if rs_small_bucket(n_rel, n) else RESCAL_MFMA_SORT), km
    return GENERIC, km


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
# model: transe_l1 / transe_l2 / hole / rescal; mode: pairwise / logistic;
# api: "step" (the fused _pairwise_step / _logistic_step) or "protocol"
# (_pairwise_gradients / _gradients, then the updaters); P: pairs, or positives
# of a logistic batch (T = 2 P triples: each positive and one corruption)
Case = namedtuple("Case", "id model mode api d n_ent n_rel P nb margin opt path km what")

MARGIN = {"transe_l1": 2.0, "transe_l2": 0.1, "hole": 0.002, "rescal": 0.002}
N_ENT = 300


def _case(model, mode, api, d, n_rel, P, path, km, what, nb=2, opt="adagrad", margin=None,
          tag=""):
    cid = "%s-%s-%s-d%d%s" % (model, mode, api, d, tag)
    return Case(cid, model, mode, api, d, N_ENT, n_rel, P, nb,
                MARGIN[model] if margin is None else margin, opt, path, km, what)


def _build():
    out = []
    # TransE L1 / L2, fused step: k_pair_grad<TRANSE, KM>, k_apply<KM>
    for model in ("transe_l1", "transe_l2"):
        for d, km, what in ((100, 2, "KM 2"), (129, 3, "KM 3, odd, one element in the third register"),
                            (257, 8, "KM 8, one element in the fifth register"),
                            (1024, 16, "KM 16, full")):
            out.append(_case(model, "pairwise", "step", d, 5, 300, GENERIC, km, what))
    # HolE, pairwise fused step and logistic step
    hole = ((68, HOLE_FAST, 2, "fast, KM 2 (d/2 = 2 * 17: no FFT plan)"),
            (100, HOLE_FFT, 2, "FFT, KM 2"),
            (128, HOLE_FFT, 2, "FFT, KM 2, full lanes"),
            (132, HOLE_FAST, 3, "fast, KM 3 (d/2 = 2 * 3 * 11)"),
            (160, HOLE_FFT, 3, "FFT, KM 3"),
            (192, HOLE_FFT, 3, "FFT, KM 3, the edge of KM 3"),
            (250, GENERIC, 4, "generic, KM 4, d % 4 = 2"),
            (256, HOLE_FAST, 4, "fast, KM 4, FFT refused (d/4 + 1 > 64)"),
            (257, GENERIC, 8, "generic, KM 8, one element in the fifth register"),
            (260, GENERIC, 8, "generic, KM 8"),
            (512, GENERIC, 8, "generic, KM 8, full"),
            (516, GENERIC, 16, "generic, KM 16"),
            (1024, GENERIC, 16, "generic, KM 16, 96 KB of LDS asked"))
    for mode in ("pairwise", "logistic"):
        for d, path, km, what in hole:
            out.append(_case("hole", mode, "step", d, 7, 200, path, km, what))
    # RESCAL on the MFMA path, pairwise and logistic
    rescal = ((100, 7, 300, 2, "2 column blocks, KM 2", ""),
              (130, 7, 300, 3, "non-VEC GEMM, 3 column blocks, KM 3", ""),
              (257, 3, 150, 8, "non-VEC, last block 1 column, KM 8", ""),
              (260, 2, 100, 8, "last block 4 columns; one dW split", "-split1"),
              (260, 2, 400, 8, "last block 4 columns; split-K dW", "-splitk"),
              (512, 3, 64, 8, "8 full column blocks", ""),
              (1024, 2, 16, 16, "16 column blocks, KM 16", ""))
    for mode in ("pairwise", "logistic"):
        for d, n_rel, P, km, what, tag in rescal:
            out.append(_case("rescal", mode, "step", d, n_rel, P, RESCAL_MFMA_SMALL, km, what,
                             tag=tag))
    # RESCAL bucketing branches, d = 8
    for mode in ("pairwise", "logistic"):
        for n_rel, P, what in ((100, 600, "sort path, chunk counts cleared by the launcher"),
                               (300, 200, "sort path because M > 256"),
                               (8192, 300, "the last M of the MFMA path: 65,540-byte scan")):
            out.append(_case("rescal", mode, "step", 8, n_rel, P, RESCAL_MFMA_SORT, 1, what,
                             tag="-M%d" % n_rel))
    # RESCAL per-pair fallback: one relation past the MFMA path; d = 36: W rows
    # of 1296 > 1024 floats go through the wide apply
    for mode in ("pairwise", "logistic"):
        for d in (8, 36):
            for opt in ("adagrad", "sgd"):
                out.append(_case("rescal", mode, "step", d, RS_MAX_M + 1, 100, RESCAL_VALU, 1,
                                 "VALU fallback, W width %d" % (d * d), opt=opt, tag="-" + opt))
    # the protocol path, one shape per KM and model: k_gather_mean<KM>,
    # k_update_rows<KM> (RESCAL's gradients there always come from the per-pair
    # kernels, whatever skge_step_path says of the fused step)
    for d, km in ((100, 2), (129, 3), (257, 8), (1024, 16)):
        for model in ("transe_l1", "transe_l2"):
            out.append(_case(model, "pairwise", "protocol", d, 5, 100, GENERIC, km, "protocol"))
    for d, km in ((100, 2), (132, 3), (257, 8), (516, 16)):
        for mode in ("pairwise", "logistic"):
            path, _ = step_path("hole", mode, d, 7, 60)
            out.append(_case("hole", mode, "protocol", d, 7, 60, path, km, "protocol"))
    for d, km in ((100, 2), (130, 3), (257, 8), (516, 16)):
        for mode in ("pairwise", "logistic"):
            out.append(_case("rescal", mode, "protocol", d, 3, 40, RESCAL_VALU, km, "protocol"))
    return out


CASES = _build()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

MULTI_D = ((100, 2), (129, 3), (257, 8), (1024, 16))   # k_transe_pos_multi<KM>, K = 3


def families(c):
    """The (kernel family, KM) instantiations case c runs."""
    f = set()
    kind = "pair" if c.mode == "pairwise" else "triple"
    if c.api == "protocol":
        f.add(("k_gather_mean", c.km))
        f.add(("k_update_rows", c.km))
        if c.model == "rescal":          # skge_pair_grad / skge_triple_grad + k_rescal_wgrad
            f.add(("%s_grad<RESCAL>" % kind, c.km))
            return f
    else:
        f.add(("k_apply", c.km))
    if c.model.startswith("transe"):
        f.add(("pair_grad<%s>" % c.model.upper(), c.km))
    elif c.model == "hole":
        form = {GENERIC: "%s_grad<HOLE>", HOLE_FAST: "hole_%s_fast", HOLE_FFT: "hole_%s_fft"}[c.path]
        f.add((form % kind, c.km))
    elif c.path == RESCAL_VALU:
        f.add(("%s_grad<RESCAL>" % kind, c.km))
        f.add(("k_apply_wide" if c.d * c.d > 1024 else "k_apply(W)", 0 if c.d * c.d > 1024 else
               km_for(c.d * c.d)))
    else:
        f.add(("rescal_mfma_%s" % kind, c.km))      # k_rescal_scatter<KM> and the logistic twin
        f.add(("rescal_ncb", (c.d + 63) // 64))
    return f


WIDE = (2, 3, 8, 16)
REQUIRED = set()
for _k in WIDE:
    REQUIRED |= {("pair_grad<TRANSE_L1>", _k), ("pair_grad<TRANSE_L2>", _k), ("k_apply", _k),
                 ("k_gather_mean", _k), ("k_update_rows", _k), ("rescal_mfma_pair", _k),
                 ("rescal_mfma_triple", _k), ("pair_grad<RESCAL>", _k), ("triple_grad<RESCAL>", _k)}
for _k in (2, 3, 4):
    REQUIRED |= {("hole_pair_fast", _k), ("hole_triple_fast", _k)}
for _k in (2, 3):
    REQUIRED |= {("hole_pair_fft", _k), ("hole_triple_fft", _k)}
for _k in (4, 8, 16):
    REQUIRED |= {("pair_grad<HOLE>", _k), ("triple_grad<HOLE>", _k)}
REQUIRED |= {("rescal_ncb", n) for n in (2, 3, 5, 8, 16)}
REQUIRED |= {("pair_grad<RESCAL>", 1), ("triple_grad<RESCAL>", 1), ("k_apply_wide", 0),
             ("k_apply(W)", 1)}


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def init_params(c, seed=3):
    """The model's initial tables as skge_amd draws them (numpy's global RNG
    seeded as test_gpu_models._model does; E, then R or each W slice; TransE's
    rows normalised, HolE's columns divided by max(column sum of squares, 1)),
    rounded to fp32 like the device's, as float64."""
    from oracle import skge_oracle as O
    np.random.seed(seed)
    E = O.init_nunif((c.n_ent, c.d))
    if c.model.startswith("transe"):
        E = O.normalize(E)
        rel = {"R": O.init_nunif((c.n_rel, c.d))}
    elif c.model == "hole":
        E = O.normless1(E)
        rel = {"R": O.init_nunif((c.n_rel, c.d))}
    else:
        rel = {"W": np.array([O.init_nunif((c.d, c.d)) for _ in range(c.n_rel)])}
    out = {"E": E}
    out.update(rel)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in out.items()}


def oracle_name(c):
    return "transe" if c.model.startswith("transe") else c.model


def oracle_kw(c):
    return {"l1": c.model == "transe_l1"} if c.model.startswith("transe") else {"rparam": 0.0}
