"""CPU checks of the DistMult / ComplEx width table (tests/diag_width_cases.py):
the library's own skge_step_path gives every case the KM the table names, every
KM appears for both models and both losses, and the inputs of each case are
judged here so that tests/test_gpu_diag_widths.py cannot hide behind them --
the worst-case fp32 error of a score stays under half the parity bar, both
outcomes of the margin decision occur, and none of them is within rounding."""
import numpy as np
import pytest

import diag_ref as DR
import diag_width_cases as W


def test_table_lists_the_issue_widths():
    by = {m: [c.d for c in W.CASES if c.model == m] for m in DR.MODELS}
    assert by["distmult"] == [65, 100, 128, 129, 192, 255, 256, 257, 512, 513, 1024]
    assert by["complex"] == [66, 100, 128, 130, 192, 194, 254, 256, 258, 512, 514, 1024]
    assert (W.N, W.M, W.P) == (300, 7, 200)
    # the row ends one complex component into a register
    assert all(d % 64 == 2 for d in (66, 130, 194, 258, 514))
    for m in DR.MODELS:
        assert {c.km for c in W.CASES if c.model == m} == {2, 3, 4, 8, 16}
        loops = [c.d for c in W.CASES if c.model == m and c.loop]
        # k_diag_pos<*, 2>, and both sides of the k_diag_pos edge
        assert {W.BY_ID["%s-d%d" % (m, d)].km for d in loops} >= {2, 4, 8}
        assert W.DIAG_POS_MAX_D in loops and min(d for d in by[m] if d > W.DIAG_POS_MAX_D) in loops


@pytest.mark.parametrize("logistic", [0, 1])
@pytest.mark.parametrize("cid", W.IDS)
def test_library_gives_the_tables_km(cid, logistic):
    from skge_amd import _lib as L
    c = W.BY_ID[cid]
    assert W.MODEL_CODE == {"distmult": L.SKGE_DISTMULT, "complex": L.SKGE_COMPLEX}
    items = 2 * W.P if logistic else W.P
    got = L.load().skge_step_path(W.MODEL_CODE[c.model], logistic, c.d, W.M, items)
    assert got == L.SKGE_PATH_GENERIC | c.km << 8, (got, L.load().skge_last_error())


@pytest.mark.parametrize("cid", W.IDS)
def test_score_error_stays_under_half_the_bar(cid):
    """(KM + 10) 2^-24 max_i A_i <= 5e-6 at the case's scale -- and the scale
    is the largest of SCALES for which it holds, so it is derived, not tuned."""
    c = W.BY_ID[cid]
    E, R = W.tables(c)
    bound = W.score_error_bound(c, E, R)
    print("%s: scale %g, bound %.3g" % (cid, c.scale, bound))
    assert bound <= W.ERR_BAR
    larger = [s for s in W.SCALES if s > c.scale]
    if larger:
        c2 = c._replace(scale=min(larger))
        assert W.score_error_bound(c2, *W.tables(c2)) > W.ERR_BAR


@pytest.mark.parametrize("cid", W.IDS)
def test_both_outcomes_occur_and_none_is_within_rounding(cid):
    c = W.BY_ID[cid]
    assert c.margin in W.MARGINS
    E, R = W.tables(c)
    gap = W.margin_gaps(c, E, R)
    share = float((gap > 0).mean())
    print("%s: margin %g, %.1f%% violate, min |gap| %.3g" % (cid, c.margin, 100 * share,
                                                            np.abs(gap).min()))
    assert 0.2 <= share <= 0.8
    assert np.abs(gap).min() > W.GAP
    # the reference's own count is this one
    pos, neg = W.pairs(c)
    assert DR.pairwise_gradients(c.model, E, R, pos, neg, c.margin)[2] == int((gap > 0).sum())


def test_pairs_hold_the_duplicates_the_kernels_merge():
    pos, neg = W.pairs(W.CASES[0])
    assert pos.shape == neg.shape == (W.P, 3)
    assert (pos[:, 0] == pos[:, 1]).any() and (pos[:, 2] == neg[:, 2]).all()
    assert ((pos[:, 0] == neg[:, 0]) & (pos[:, 1] != neg[:, 1])).any()
    assert ((pos[:, 1] == neg[:, 1]) & (pos[:, 0] != neg[:, 0])).any()
    trip, ys = W.labelled(W.CASES[0])
    assert trip.shape == (2 * W.P, 3) and ys.sum() == 0
    st = W.score_triples(W.CASES[0])
    assert st.shape == (W.NSCORE, 3) and st[:, :2].max() < W.N and st[:, 2].max() < W.M


def test_loop_and_dense_kgs():
    kg = W.loop_kg(192)
    assert len({tuple(t) for t in kg.tolist()}) == 192
    assert kg[:, :2].max() < W.N and kg[:, 2].max() < W.M
    dense = W.dense_kg()
    have = {tuple(t) for t in dense.tolist()}
    assert dense[:, :2].max() < W.DENSE_N and dense[:, 2].max() < W.DENSE_M
    no_s, no_o = W.undrawn(dense, None)
    assert no_s.sum() == W.DENSE_N and no_o.sum() == W.DENSE_N
    for (s, o, p), ns, no in zip(dense.tolist(), no_s, no_o):
        # undrawn exactly where every corruption of that side is a training triple
        assert ns == all((c, o, p) in have for c in range(W.DENSE_N))
        assert no == all((s, c, p) in have for c in range(W.DENSE_N))
