"""Host restatement of RESCAL's row-grouped entity apply (csrc/skge_rescal.hip:
k_rs_rows_ep groups a batch's entity slots by row, k_rescal_fold sums and
applies them), pure numpy, no GPU.

A batch is records [start, start + count) of the epoch: rec[j] = (s, o, p, s'
or -1), rec_n1[j] = o' or -1.  Record j (numbered within the batch) holds up
to four entity slots (j, role): role 0 = s, 1 = o, 2 = s' (the subject of the
pair (s, o, p) / (s', o, p)), 3 = o' (the object of (s, o, p) / (s, o', p));
roles 2 and 3 exist only when the drawn id is >= 0.  A distinct row's slots
are kept in slot order (ascending (j, role)), two per work item, and the item
count decides the path k_rescal_fold takes for the row (its regime).

The fp64 per-slot contributions restate skge/rescal.py:78-139 in the
oracle's conventions ((s, o, p) triples, oracle.skge_oracle's activations)
slot by slot instead of through grad_sum_matrix: what each slot adds to its
row's sum and to its row's count of violating occurrences.  Their segment
mean is oracle.pairwise_step("rescal", ...)'s (grad, idx) for E
(tests/test_rescal_rows_ref.py holds that to 1e-12).
"""
import collections

import numpy as np

from oracle import skge_oracle as O

# k_rs_rows_ep (skge_rescal.hip:706, 716-718): a row of n slots becomes
# nch = (n + 1) >> 1 consecutive work items of two slots each
SLOTS_PER_ITEM = 2
# k_rescal_fold (skge_rescal.hip:1259 RS_FOLD_MERGE, 1389 `nch == 1`, 1415
# `hub = nch > RS_FOLD_MERGE`): one item: summed in registers; up to this many:
# partial sums merged by the last arriver; more: through the entity accumulator
FOLD_MERGE_ITEMS = 8
# k_rs_rows_ep's LDS hash (skge_rescal.hip:624 RS_ROWS_MAX, 2331 rs_rows_ok):
# 4 bs slots per batch at most
ROWS_MAX_SLOTS = 8192
# rs_wsplit / rs_front_splits (skge_rescal.hip:212-254): dW groups of
# WS_GROUP = 2 * 64 items; from 4 groups per relation on the dW is split
# (at most 8 ways), and a split dW keeps the W step out of the front
DW_GROUP_ITEMS = 128
DW_SPLIT_FROM_GROUPS = 4
# rescal_epoch_ok (skge_rescal.hip:2311): the epoch's buckets need M <= 64
EPOCH_BUCKETS_MAX_M = 64

REGIMES = ("single", "merge", "hub")

Row = collections.namedtuple("Row", "row slots items regime")


def regime_of(items):
    if items <= 1:
        return "single"
    return "merge" if items <= FOLD_MERGE_ITEMS else "hub"


def group_rows(rec, rec_n1, start, count):
    """The batch's distinct entity rows (ascending row id), each a
    Row(row, slots, items, regime): slots = [(j, role), ...] in slot order,
    items = ceil(len(slots) / 2)."""
    by_row = collections.defaultdict(list)
    for j in range(count):
        s, o, _, a = (int(x) for x in rec[start + j])
        b = int(rec_n1[start + j])
        for role, row in enumerate((s, o, a, b)):
            if row >= 0:
                by_row[row].append((j, role))      # ascending (j, role): slot order
    out = []
    for row in sorted(by_row):
        slots = by_row[row]
        items = (len(slots) + SLOTS_PER_ITEM - 1) // SLOTS_PER_ITEM
        out.append(Row(row, slots, items, regime_of(items)))
    return out


def regime_counts(rows):
    c = collections.Counter(r.regime for r in rows)
    return {k: c.get(k, 0) for k in REGIMES}


def self_loops(rec, start, count):
    r = np.asarray(rec)[start:start + count]
    return int((r[:, 0] == r[:, 1]).sum())


def _we(E, W, p, o):
    """W[p_n] E[o_n] per record, relation by relation."""
    out = np.zeros((len(p), E.shape[1]))
    for q in np.unique(p):
        m = p == q
        out[m] = E[o[m]].dot(W[q].T)
    return out


def _ew(E, W, s, p):
    """E[s_n] W[p_n] per record."""
    out = np.zeros((len(p), E.shape[1]))
    for q in np.unique(p):
        m = p == q
        out[m] = E[s[m]].dot(W[q])
    return out


def slot_contributions(rec, rec_n1, start, count, E, W, margin, af=O.Linear):
    """fp64 contribution and count of every slot of the batch.

    Returns (x [count, 4, d], c [count, 4], present [count, 4], nviol).  A
    record's two pairs are (s, o, p) against (s', o, p) (pair 0, when s' >= 0)
    and against (s, o', p) (pair 1, when o' >= 0); v0 / v1 say whether they
    violate the margin (rescal.py:104).  A violating pair adds four
    occurrences (rescal.py:133-137): its positive's s and o, its negative's
    subject and object -- so with gp = -g(f+), g0 / g1 = g(f-) (rescal.py:
    110-111):
      s  (role 0): v0 gp W_p E_o + v1 (gp W_p E_o + g1 W_p E_o'), count v0 + 2 v1
      o  (role 1): v0 (gp E_s W_p + g0 E_s' W_p) + v1 gp E_s W_p, count 2 v0 + v1
      s' (role 2): v0 g0 W_p E_o,                                 count v0
      o' (role 3): v1 g1 E_s W_p,                                 count v1
    (pair 1's negative keeps the subject s, pair 0's the object o)."""
    E = np.asarray(E, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    r = np.asarray(rec, dtype=np.int64)[start:start + count]
    s, o, p, a = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    b = np.asarray(rec_n1, dtype=np.int64)[start:start + count]
    k0, k1 = a >= 0, b >= 0
    a_, b_ = np.where(k0, a, 0), np.where(k1, b, 0)
    we_pos = _we(E, W, p, o)          # W_p E_o: of (s, o, p) and of (s', o, p)
    we_n1 = _we(E, W, p, b_)          # W_p E_o' of (s, o', p)
    ew_pos = _ew(E, W, s, p)          # E_s W_p: of (s, o, p) and of (s, o', p)
    ew_n0 = _ew(E, W, a_, p)          # E_s' W_p of (s', o, p)
    pf = af.f(np.sum(E[s] * we_pos, axis=1))
    f0 = af.f(np.sum(E[a_] * we_pos, axis=1))
    f1 = af.f(np.sum(E[s] * we_n1, axis=1))
    v0 = (k0 & (f0 + margin > pf)).astype(np.float64)[:, None]
    v1 = (k1 & (f1 + margin > pf)).astype(np.float64)[:, None]
    gp = -np.asarray(af.g_given_f(pf), dtype=np.float64)[:, None]
    g0 = np.asarray(af.g_given_f(f0), dtype=np.float64)[:, None]
    g1 = np.asarray(af.g_given_f(f1), dtype=np.float64)[:, None]
    x = np.zeros((count, 4, E.shape[1]))
    x[:, 0] = v0 * gp * we_pos + v1 * (gp * we_pos + g1 * we_n1)
    x[:, 1] = v0 * (gp * ew_pos + g0 * ew_n0) + v1 * gp * ew_pos
    x[:, 2] = v0 * g0 * we_pos
    x[:, 3] = v1 * g1 * ew_pos
    iv0, iv1 = v0[:, 0].astype(np.int64), v1[:, 0].astype(np.int64)
    c = np.stack([iv0 + 2 * iv1, 2 * iv0 + iv1, iv0, iv1], axis=1)
    present = np.stack([np.ones(count, dtype=bool), np.ones(count, dtype=bool), k0, k1], axis=1)
    return x, c, present, int(iv0.sum() + iv1.sum())


def row_sums(rows, x, c):
    """Per Row: (sum of its slots' contributions in slot order, its count of
    violating occurrences)."""
    out = {}
    for r in rows:
        js = np.array([j for j, _ in r.slots])
        ro = np.array([role for _, role in r.slots])
        xs = x[js, ro]
        out[r.row] = (xs.sum(axis=0), int(c[js, ro].sum()))
    return out


def row_gradient(rows, x, c):
    """The slots' segment mean over the rows with a violating occurrence:
    (idx ascending, grad [len(idx), d], counts), as pairwise_step's E
    gradient (rparam = 0)."""
    sums = row_sums(rows, x, c)
    idx = [r.row for r in rows if sums[r.row][1] > 0]
    g = np.array([sums[i][0] / sums[i][1] for i in idx]).reshape(len(idx), x.shape[2])
    return np.array(idx, dtype=np.int64), g, np.array([sums[i][1] for i in idx], dtype=np.int64)


def front_splits(n, M):
    """rs_front_splits (skge_rescal.hip:242-254) of a batch of n = 3 * count
    bucketed triples in the default form: 1 unless a relation holds at least
    DW_SPLIT_FROM_GROUPS groups (the 64 MB cap of the partial tiles is far off
    at the tests' sizes and is not restated)."""
    groups = (n // M + DW_GROUP_ITEMS - 1) // DW_GROUP_ITEMS
    return 1 if groups < DW_SPLIT_FROM_GROUPS else min(8, groups)


def entity_apply_form(T, nb, M, form=""):
    """The entity-apply form the pair loop captures for RESCAL with the Linear
    activation (skge_rescal_pos_grad_mfma_ep, skge_rescal.hip:2416-2418 and
    2451): "rows" when the W step is in the front -- one dW split for the full
    and for the last batch -- the relation count fits the epoch's buckets, the
    batch's slots fit the grouping and the form has no scatter / wapply token;
    else "scatter"."""
    bs = T // nb
    nbat = (T + bs - 1) // bs
    last = T - (nbat - 1) * bs
    tokens = [t for t in form.split(",") if t]
    ok = (M <= EPOCH_BUCKETS_MAX_M and 4 * bs <= ROWS_MAX_SLOTS and
          front_splits(3 * bs, M) == 1 and front_splits(3 * last, M) == 1 and
          not any(t in ("scatter", "wapply", "unfused", "nodedup", "dw3") for t in tokens))
    return "rows" if ok else "scatter"
