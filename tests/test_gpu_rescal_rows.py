"""RESCAL's row-grouped entity apply (k_rescal_fold, csrc/skge_rescal.hip)
against the fp64 oracle in every row regime.

k_rescal_fold takes one of three paths per distinct entity row of a batch, by
the row's work items (two slots each, k_rs_rows_ep): one item -- summed in
registers; 2 .. 8 items -- partial sums merged by the last arriver; more (a
hub row) -- through the entity accumulator (fp32 atomics, or exact FX64 in
the deterministic mode), zeroed again by the last arriver.  At WN18's uniform
geometry (test_gpu_runner_oracle.py) rows have 1-4 slots, so only the first
path met the oracle there.

Here the KG is Zipf-skewed and small (bench.make_zipf_kg(400, 5, 768, seed=7),
3 batches of B = 256; its first-256 sibling for the one-batch cases): every
batch has single, merge and hub rows, self-loops, rows at the 8 / 9 item
boundary -- asserted from the epoch's records through the host restatement of
the grouping (tests/rescal_rows_ref.py), with the captured form
(PairLoopRunner.entity_apply).  Every comparison is with
oracle.pairwise_step replaying the device's pairs (runner_oracle_util), the
E table reported per regime (single / merge / hub: the headroom record's
name says which path a failure is in).  Violation totals are exactly equal.

Widths: every KM instantiation (km_for: d <= 64 -> 1, <= 128 -> 2, <= 192 -> 3,
<= 256 -> 4, <= 512 -> 8), d % 4 != 0 (the non-vector front) and 1 .. 5 column
blocks (ncb = ceil(d / 64)).  All of them meet the fold's conditions at
B = 256, M = 5 (rescal_rows_ref.entity_apply_form: 153 items per relation are
2 dW groups, one split), so every case of the table asserts "rows".

Measured headrooms: profiles/rescal_rows/README.md.
"""
import numpy as np
import pytest
import torch

import parity_util
import rescal_rows_ref as RR
from oracle import skge_oracle as O
from runner_oracle_util import epoch_vs_oracle, pairs, snapshot

pytestmark = pytest.mark.gpu

N, M, B, NB = 400, 5, 256, 3
MARGIN = 0.2
# the runner's seed: on the CPU replay of the device draws (tests/sampler_ref.py,
# multineg_ref.epoch_permutation) seed 48 gives rows of exactly 8 or 9 items in
# every epoch of the 3-batch KG and of the one-batch KG (asserted below from
# the device's own records)
SEED = 48

#          d    KM  d % 4  ncb  form
WIDTHS = [(20, 1, 0, 1, "rows"),
          (30, 1, 2, 1, "rows"),
          (100, 2, 0, 2, "rows"),
          (130, 3, 2, 3, "rows"),
          (200, 4, 0, 4, "rows"),
          (260, 8, 0, 5, "rows")]
D_ALL = [w[0] for w in WIDTHS]
FORM = {w[0]: w[4] for w in WIDTHS}
MIN_ROWS = {"single": 20, "merge": 10, "hub": 3}


def test_width_table_is_what_the_library_instantiates():
    from skge_amd import _lib as L
    for d, km, rem, ncb, form in WIDTHS:
        assert L.lib().skge_step_path(L.SKGE_RESCAL, 0, d, M, 3 * B) >> 8 == km
        assert (d % 4, (d + 63) // 64) == (rem, ncb)
        assert form == RR.entity_apply_form(NB * B, NB, M) == RR.entity_apply_form(B, 1, M)
    assert sorted({w[1] for w in WIDTHS}) == [1, 2, 3, 4, 8]


_KGS = {}


def _zipf(T):
    from bench import make_zipf_kg
    if T not in _KGS:
        _KGS[T] = make_zipf_kg(N, M, T, seed=7)
    return _KGS[T]


def _model(d, opt, lr, xs, n_ent=N, n_rel=M, margin=MARGIN):
    import skge_amd as S
    from skge_amd.device import DeviceKG
    np.random.seed(42)
    m = S.RESCAL((n_ent, n_ent, n_rel), d)
    m.add_hyperparam("margin", margin)
    upd = _updaters(m, opt, lr)
    return m, upd, DeviceKG(xs, m.device)


def _updaters(m, opt, lr):
    import skge_amd as S
    U = S.AdaGrad if opt == "adagrad" else S.SGD
    return {pid: U(p, lr) for pid, p in m.params.items()}


def _runner(m, upd, kg, nb, form="rows", ntries=100):
    from skge_amd.device import PairLoopRunner
    r = PairLoopRunner(m, upd, kg, nb, seed=SEED, ntries=ntries)
    assert r.entity_apply == form, (r.entity_apply, form)
    return r


class Regimes:
    """The replayed batches' rows by regime (a batch_hook of epoch_vs_oracle),
    the asserts on them, and what the per-regime checks need."""

    def __init__(self, what, minima=MIN_ROWS, full=B, margin=MARGIN):
        self.what, self.minima, self.full, self.margin = what, minima, full, margin
        self.batches = []          # per batch: (rows, counts, idx of the oracle's E gradient)
        self.loops = self.boundary = 0
        self.kinds = set()         # of the records: which negatives were found

    def __call__(self, rec, n1, start, count, before, grads):
        rows = RR.group_rows(rec, n1, start, count)
        counts = RR.regime_counts(rows)
        if count == self.full:
            for k, least in self.minima.items():
                assert counts[k] >= least, (self.what, len(self.batches), counts)
        self.loops += RR.self_loops(rec, start, count)
        self.boundary += sum(1 for r in rows if r.items in (RR.FOLD_MERGE_ITEMS,
                                                            RR.FOLD_MERGE_ITEMS + 1))
        a, b = rec[start:start + count, 3] >= 0, n1[start:start + count] >= 0
        self.kinds |= set(zip(a.tolist(), b.tolist()))
        idx = np.asarray(grads["E"][1], dtype=np.int64) if grads else np.empty(0, dtype=np.int64)
        # the restatement agrees with the oracle on this very batch
        x, c, _, _ = RR.slot_contributions(rec, n1, start, count, before["E"], before["W"],
                                           self.margin)
        ridx, rg, _ = RR.row_gradient(rows, x, c)
        assert np.array_equal(ridx, idx), self.what
        if grads:
            assert np.max(np.abs(rg - grads["E"][0])) <= 1e-12, self.what
        self.batches.append((rows, counts, idx))

    def groups(self):
        """Each entity row under the heaviest regime it has in any batch."""
        rank = {}
        for rows, _, _ in self.batches:
            for r in rows:
                rank[r.row] = max(rank.get(r.row, 0), RR.REGIMES.index(r.regime))
        return {k: np.array(sorted(r for r, v in rank.items() if v == i), dtype=np.int64)
                for i, k in enumerate(RR.REGIMES)}

    def check_epoch(self):
        assert self.loops >= 1, (self.what, "no self-loop")
        assert self.boundary >= 1, (self.what, "no row of exactly 8 or 9 items")
        print("RESCAL-ROWS %s: rows per batch (single, merge, hub) %s, self-loops %d, "
              "8/9-item rows %d" % (self.what, [tuple(c[k] for k in RR.REGIMES)
                                                for _, c, _ in self.batches],
                                    self.loops, self.boundary))


def _replay(m, upd, r, kg, epoch, nb, opt, what, lr=0.1, reg=None, n_ent=N, **kw):
    reg = reg or Regimes(what)
    with torch.cuda.stream(r.stream):
        v = epoch_vs_oracle("rescal", m, upd, r, kg, SEED, epoch, nb, opt, what, n_ent=n_ent,
                            lr=lr, batch_hook=reg, groups={"E": reg.groups}, af=O.Linear, **kw)
    return v, reg


# ---- (a) gradient probe ----

@pytest.mark.parametrize("d", D_ALL)
def test_fold_gradients_vs_oracle(d):
    """SGD(lr = 1), one batch of B = 256 from tables warmed by one epoch:
    P - P' is the device's segment mean to half an ulp of |P'|
    (test_gpu_runner_oracle.test_runner_gradients_vs_oracle), held to the
    oracle's E gradient at the plain bar 1e-5 + 1e-5 |g|, separately for the
    single, merge and hub rows; rows outside idx bit-unchanged; W at the same
    bar."""
    from skge_amd.device import epoch_records
    xs = _zipf(B)
    m0, upd0, kg = _model(d, "sgd", 0.1, xs)
    r0 = _runner(m0, upd0, kg, 1, FORM[d])
    r0.run(1)
    r0.synchronize()
    del r0
    m, upd, _ = _model(d, "sgd", 1.0, xs)
    for pid, p in m.params.items():
        p.post = None
        p.data.copy_(m0.params[pid].data)
    r = _runner(m, upd, kg, 1, FORM[d])
    before, _ = snapshot(m, upd)
    rec, n1 = (x.cpu().numpy() for x in epoch_records(kg, N, SEED, 0))
    with torch.cuda.stream(r.stream):
        r.run(1)
        r.synchronize()
    torch.cuda.synchronize()
    got_v = int(r.nviol_total.item())
    pos, neg = pairs(rec, n1, 0, B)
    params = {k: v.copy() for k, v in before.items()}
    state = {k: np.zeros_like(v) for k, v in before.items()}
    _, _, want_v, grads = O.pairwise_step("rescal", params, state, pos, neg, 1.0, MARGIN, "sgd",
                                          af=O.Linear)
    assert got_v == want_v > 0
    what = "rescal rows d%d probe" % d
    reg = Regimes(what)
    reg(rec, n1, 0, B, before, grads)
    reg.check_epoch()
    after, _ = snapshot(m, upd)
    for pid in ("E", "W"):
        g_dev = before[pid] - after[pid]
        rows, idx = grads[pid]
        rows, idx = np.asarray(rows, dtype=np.float64), np.asarray(idx, dtype=np.int64)
        mask = np.ones(g_dev.shape[0], dtype=bool)
        mask[idx] = False
        assert np.array_equal(after[pid][mask], before[pid][mask]), "%s %s: untouched rows moved" \
            % (what, pid)
        if pid == "W":
            parity_util.check(g_dev[idx], rows, "%s gradient W" % what)
            continue
        seen = 0
        for name, members in reg.groups().items():
            sel = np.isin(idx, members)
            assert sel.any(), (what, name, "no row of this regime has a violating occurrence")
            seen += int(sel.sum())
            parity_util.check(g_dev[idx[sel]], rows[sel], "%s gradient E [%s rows]" % (what, name))
        assert seen == len(idx)


# ---- (b) SGD, 3 batches, two consecutive runs ----

@pytest.mark.parametrize("d", D_ALL)
def test_fold_sgd_epochs_vs_oracle(d):
    """SGD: a warm-up epoch, then one epoch of 3 batches against the oracle
    (merge rows' partial sums and hub rows' accumulator handed from batch to
    batch: the accumulator and counts must be zero again), then a second
    run(1) of the same runner replayed the same way (rowctr, the violation
    word and the accumulator across runs)."""
    m, upd, kg = _model(d, "sgd", 0.1, _zipf(NB * B))
    r = _runner(m, upd, kg, NB, FORM[d])
    with torch.cuda.stream(r.stream):
        r.run(1)
        r.synchronize()
    for epoch in (1, 2):
        what = "rescal rows d%d sgd 3 batches e%d" % (d, epoch)
        v, reg = _replay(m, upd, r, kg, epoch, NB, "sgd", what, sizes=[B] * NB)
        assert v > 0
        reg.check_epoch()


# ---- (c) AdaGrad, one batch per epoch, fp32 and deterministic sums ----

@pytest.mark.parametrize("det", [False, True], ids=["fp32", "fx64"])
@pytest.mark.parametrize("d", [30, 200])
def test_fold_adagrad_batches_vs_oracle_from_device_state(d, det):
    """AdaGrad, one batch of B = 256 per epoch, 3 epochs, each replayed from
    the device state before it (check_step), with fp32 hub sums and in the
    deterministic mode (hub rows through FX64); E's updateCounts against the
    batches whose oracle idx holds the row.  The fp32 hub rows pass check_step
    as it stands: no summation-order term for their 50-150-term sums is
    added (measured: profiles/rescal_rows/README.md)."""
    import skge_amd as S
    prev = S.deterministic()
    S.set_deterministic(det)
    try:
        m, upd, kg = _model(d, "adagrad", 0.1, _zipf(B))
        r = _runner(m, upd, kg, 1, FORM[d])
        want_counts = np.zeros(N, dtype=np.int64)
        viol = []
        for epoch in range(3):
            what = "rescal rows d%d adagrad %s e%d" % (d, "fx64" if det else "fp32", epoch)
            v, reg = _replay(m, upd, r, kg, epoch, 1, "adagrad", what, sizes=[B])
            reg.check_epoch()
            viol.append(v)
            want_counts[reg.batches[0][2]] += 1
        assert viol[0] > 0
        assert np.array_equal(m.params["E"].updateCounts, want_counts)
    finally:
        S.set_deterministic(prev)


# ---- (d) missing negatives ----

def _dense_kg():
    """N = 24, M = 2: every (s, o, p) but 117 of the 1152 (10 %), T = 1035 = 5
    batches of 207.  With ntries = 2 most draws hit a known triple."""
    n, nrel = 24, 2
    rs = np.random.RandomState(5)
    keep = np.sort(rs.permutation(n * n * nrel)[:1035])
    return np.stack([keep // (n * nrel), (keep // nrel) % n, keep % nrel], axis=1).astype(np.int32)


@pytest.mark.parametrize("d", [30, 200])
def test_fold_missing_negatives_vs_oracle(d):
    """Records whose s', o' or both were not found (the k0 / k1 bits of the
    slot word: no slot for the id, a zero coefficient for the pair), SGD, 5
    batches of 207 after a warm-up epoch.  24 entities: nearly every row is a
    hub."""
    n, nrel, nb = 24, 2, 5
    xs = _dense_kg()
    assert RR.entity_apply_form(len(xs), nb, nrel) == "rows"
    m, upd, kg = _model(d, "sgd", 0.1, xs, n_ent=n, n_rel=nrel)
    r = _runner(m, upd, kg, nb, "rows", ntries=2)
    with torch.cuda.stream(r.stream):
        r.run(1)
        r.synchronize()
    what = "rescal rows d%d missing negatives sgd" % d
    reg = Regimes(what, minima={"hub": 3}, full=207)
    v, reg = _replay(m, upd, r, kg, 1, nb, "sgd", what, reg=reg, n_ent=n, sizes=[207] * nb,
                     all_found=False, ntries=2)
    assert v > 0
    # (s' found, o' found): only s' missing, only o' missing, both missing -- and both found
    assert reg.kinds == {(False, True), (True, False), (False, False), (True, True)}, reg.kinds
    print("RESCAL-ROWS %s: rows per batch (single, merge, hub) %s"
          % (what, [tuple(c[k] for k in RR.REGIMES) for _, c, _ in reg.batches]))


# ---- (e) ragged tail ----

def test_fold_ragged_tail_vs_oracle():
    """T = 800 in nb = 3: batches of 266, 266, 266 and 2.  rs_front_splits is
    evaluated for the 2-positive last batch as well (6 items: one split), so
    the form is still the row-grouped apply; d = 130 (KM = 3, d % 4 != 0)."""
    d, T = 130, 800
    assert RR.entity_apply_form(T, NB, M) == "rows"
    m, upd, kg = _model(d, "sgd", 0.1, _zipf(T))
    r = _runner(m, upd, kg, NB, "rows")
    with torch.cuda.stream(r.stream):
        r.run(1)
        r.synchronize()
    for epoch in (1, 2):
        what = "rescal rows d%d ragged tail sgd e%d" % (d, epoch)
        reg = Regimes(what, full=266)
        v, reg = _replay(m, upd, r, kg, epoch, NB, "sgd", what, reg=reg,
                         sizes=[266, 266, 266, 2])
        assert v > 0 and len(reg.batches) == 4
        reg.check_epoch()


# ---- (f) no violation ----

@pytest.mark.parametrize("d", [30, 200])
def test_fold_batch_without_violation_moves_nothing(d):
    """A margin so negative that no pair violates it (the oracle says 0): the
    gate.  nviol_total stays, E, W, both AdaGrad states and the update counts
    are bit-identical after the epoch (a flipped W buffer would be copied back
    at the epoch's end).  An epoch at the normal margin from those tables then
    matches the oracle."""
    import skge_amd as S
    from skge_amd.device import epoch_records
    xs = _zipf(NB * B)
    m, upd, kg = _model(d, "adagrad", 0.1, xs)
    r = _runner(m, upd, kg, NB, FORM[d])
    with torch.cuda.stream(r.stream):
        r.run(1)                       # warm-up at the normal margin
        r.synchronize()
    del r
    m.add_hyperparam("margin", -1e3)
    r = _runner(m, upd, kg, NB, FORM[d])
    rec, n1 = (x.cpu().numpy() for x in epoch_records(kg, N, SEED, 0))
    params, state = snapshot(m, upd)
    for b in range(NB):
        pos, neg = pairs(rec, n1, b * B, B)
        _, _, nv, grads = O.pairwise_step("rescal", {k: v.copy() for k, v in params.items()},
                                          {k: v.copy() for k, v in state.items()}, pos, neg, 0.1,
                                          -1e3, "adagrad", af=O.Linear)
        assert nv == 0 and grads is None
    keep = {pid: (p.data.clone(), upd[pid].p2.clone(), p.updateCounts.copy())
            for pid, p in m.params.items()}
    with torch.cuda.stream(r.stream):
        r.run(1)
        r.synchronize()
    torch.cuda.synchronize()
    assert int(r.nviol_total.item()) == 0
    for pid, p in m.params.items():
        assert torch.equal(p.data, keep[pid][0]), "%s moved" % pid
        assert torch.equal(upd[pid].p2, keep[pid][1]), "%s AdaGrad state moved" % pid
        assert np.array_equal(p.updateCounts, keep[pid][2]), "%s update counts moved" % pid
    del r
    m.add_hyperparam("margin", MARGIN)
    upd = _updaters(m, "sgd", 0.1)
    r = _runner(m, upd, kg, NB, FORM[d])
    what = "rescal rows d%d after a no-violation epoch sgd" % d
    v, reg = _replay(m, upd, r, kg, 0, NB, "sgd", what, sizes=[B] * NB)
    assert v > 0
    reg.check_epoch()
