"""CPU checks of tests/rescal_rows_ref.py, the host restatement of RESCAL's
row grouping (k_rs_rows_ep) and of the per-slot contributions k_rescal_fold
sums: the regimes and slot order on hand-written records, and the per-slot
restatement's segment mean against oracle.pairwise_step's E gradient."""
import numpy as np
import pytest

import rescal_rows_ref as RR
from oracle import skge_oracle as O

N, M, D = 12, 3, 7

# (s, o, p, s' or -1), o' or -1
RECORDS = [
    ((0, 1, 0, 2), 3),        # plain: four distinct rows
    ((4, 4, 1, 5), 6),        # self-loop: row 4 in roles 0 and 1 of one record
    ((1, 7, 2, 7), 0),        # s' == o: row 7 in roles 1 and 2
    ((8, 0, 0, -1), 9),       # s' not found
    ((9, 8, 1, 2), -1),       # o' not found
    ((10, 3, 2, -1), -1),     # neither found: no pair
    ((0, 2, 1, 1), 0),        # o' == s: row 0 in roles 0 and 3
]
# rows 11 and 5: a 40-slot hub (20 records x roles 0 and 3; 3 of them without
# s') and the 8 / 9 item boundary
HUB = [((11, (j % 5), j % M, (j + 1) % 4 if j % 7 else -1), 11) for j in range(20)]


def _records(extra=()):
    recs = RECORDS + HUB + list(extra)
    rec = np.array([r for r, _ in recs], dtype=np.int32)
    n1 = np.array([b for _, b in recs], dtype=np.int32)
    return rec, n1


def _tables(seed=3):
    rs = np.random.RandomState(seed)
    return rs.uniform(-0.6, 0.6, (N, D)), rs.uniform(-0.6, 0.6, (M, D, D))


def _pairs(rec, n1, start, count):
    pos, neg = [], []
    for j in range(start, start + count):
        s, o, p, a = (int(x) for x in rec[j])
        b = int(n1[j])
        if a >= 0:
            pos.append((s, o, p))
            neg.append((a, o, p))
        if b >= 0:
            pos.append((s, o, p))
            neg.append((s, b, p))
    return np.array(pos, dtype=np.int64), np.array(neg, dtype=np.int64)


def test_regimes_thresholds():
    assert [RR.regime_of(i) for i in (1, 2, 8, 9, 20)] == ["single", "merge", "merge", "hub", "hub"]


def test_slots_items_and_regimes_of_hand_written_records():
    rec, n1 = _records()
    rows = {r.row: r for r in RR.group_rows(rec, n1, 0, len(rec))}
    # every slot is listed exactly once, under its own row, in ascending (j, role)
    seen = []
    for r in rows.values():
        assert r.slots == sorted(r.slots)
        assert r.items == (len(r.slots) + 1) // 2
        for j, role in r.slots:
            want = (int(rec[j][0]), int(rec[j][1]), int(rec[j][3]), int(n1[j]))[role]
            assert want == r.row
        seen += r.slots
    nslots = int(2 * len(rec) + (rec[:, 3] >= 0).sum() + (n1 >= 0).sum())
    assert len(seen) == len(set(seen)) == nslots
    assert rows[4].slots[:2] == [(1, 0), (1, 1)]                 # the self-loop
    assert (2, 1) in rows[7].slots and (2, 2) in rows[7].slots   # s' == o
    assert (6, 0) in rows[0].slots and (6, 3) in rows[0].slots   # o' == s
    assert all(role < 2 for j, role in rows[10].slots if j == 5)  # no slot for a missing id
    assert rows[10].slots == [(5, 0)] and rows[10].regime == "single"
    assert len(rows[11].slots) == 40 and rows[11].items == 20 and rows[11].regime == "hub"
    assert rows[6].slots == [(1, 3)] and rows[6].regime == "single"
    assert RR.self_loops(rec, 0, len(rec)) == 1


@pytest.mark.parametrize("nslots,items,regime", [(1, 1, "single"), (2, 1, "single"),
                                                 (3, 2, "merge"), (15, 8, "merge"),
                                                 (16, 8, "merge"), (17, 9, "hub")])
def test_item_boundaries(nslots, items, regime):
    """Row 5 alone in a batch with exactly nslots slots (as o' of nslots records)."""
    rec = np.array([(0, 1, 0, -1)] * nslots, dtype=np.int32)
    n1 = np.full(nslots, 5, dtype=np.int32)
    r = {x.row: x for x in RR.group_rows(rec, n1, 0, nslots)}[5]
    assert (len(r.slots), r.items, r.regime) == (nslots, items, regime)
    assert r.slots == [(j, 3) for j in range(nslots)]


def test_batch_window_is_respected():
    rec, n1 = _records()
    rows = RR.group_rows(rec, n1, 7, 20)          # the HUB records only, j from 0
    r11 = [r for r in rows if r.row == 11][0]
    assert r11.slots[0] == (0, 0) and len(r11.slots) == 40
    assert RR.regime_counts(rows)["hub"] >= 1


@pytest.mark.parametrize("af", [O.Linear, O.Sigmoid, O.Tanh])
@pytest.mark.parametrize("margin", [0.2, 2.0, -50.0])
def test_slot_mean_is_the_oracle_gradient(af, margin):
    """The per-slot restatement's segment mean and count against
    pairwise_step's (grad, idx) for E and its nviol, to 1e-12 -- over the
    self-loop, s' == o, o' == s, the missing negatives and the 40-slot row."""
    rec, n1 = _records()
    E, W = _tables()
    n = len(rec)
    x, c, present, nviol = RR.slot_contributions(rec, n1, 0, n, E, W, margin, af)
    assert np.array_equal(present[:, 2], rec[:, 3] >= 0) and np.array_equal(present[:, 3], n1 >= 0)
    assert not x[~present].any() and not c[~present].any()
    pos, neg = _pairs(rec, n1, 0, n)
    params = {"E": E.copy(), "W": W.copy()}
    state = {k: np.zeros_like(v) for k, v in params.items()}
    _, _, want_v, grads = O.pairwise_step("rescal", params, state, pos, neg, 1.0, margin, "sgd",
                                          af=af)
    assert nviol == want_v
    if margin < 0:
        assert want_v == 0 and grads is None and not c.any()
        return
    assert want_v > 0
    rows = RR.group_rows(rec, n1, 0, n)
    idx, g, cnt = RR.row_gradient(rows, x, c)
    want_g, want_idx = grads["E"]
    assert np.array_equal(idx, np.asarray(want_idx))
    assert np.max(np.abs(g - want_g)) <= 1e-12
    # the counts are the violating occurrences grad_sum_matrix divides by
    occ = np.bincount(np.concatenate([pos[:, 0], neg[:, 0], pos[:, 1], neg[:, 1]])[
        np.tile(_violating(E, W, pos, neg, margin, af), 4)], minlength=N)
    assert np.array_equal(cnt, occ[idx])


def _violating(E, W, pos, neg, margin, af):
    pf = af.f(O.rescal_scores(E, W, pos))
    nf = af.f(O.rescal_scores(E, W, neg))
    return nf + margin > pf


def test_entity_apply_form_conditions():
    """The capture's conditions at the shapes the GPU tests use."""
    assert RR.front_splits(3 * 256, 5) == 1 and RR.front_splits(3 * 2, 5) == 1
    assert RR.front_splits(3 * 666, 5) == 4          # 399 items per relation: 4 groups
    assert RR.entity_apply_form(768, 3, 5) == "rows"
    assert RR.entity_apply_form(800, 3, 5) == "rows"           # 266 x 3 + a tail of 2
    assert RR.entity_apply_form(768, 1, 5) == "scatter"        # one batch of 768: dW split
    assert RR.entity_apply_form(2000, 3, 5) == "scatter"
    assert RR.entity_apply_form(768, 3, 5, "scatter") == "scatter"
    assert RR.entity_apply_form(768, 3, 5, "wapply") == "scatter"
    assert RR.entity_apply_form(768, 3, 65) == "scatter"
    assert RR.entity_apply_form(3 * 2049, 3, 64) == "scatter"  # 4 bs > 8192
