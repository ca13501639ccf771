"""The per-batch step kernels at every row-width layout (KM = 2, 3, 8, 16 beside
the 1 and 4 of the fixtures and test_gpu_models.py), every HolE form at its
edges, the RESCAL MFMA path up to 16 column blocks, its bucketing branches and
its per-pair fallback, against the oracle (GPU).

The shapes and what each is for are the table of tests/width_cases.py, which
tests/test_width_cases.py holds to the selection rules on the CPU; here each
test first asserts that the library's own skge_step_path sends the shape to
the path the table names, then runs test_gpu_models' _run / _run_logistic: one
oracle step per device step from the device's own state, parity_util's bar
unchanged, violation counts exact.
"""
import numpy as np
import pytest
import torch

import parity_util
import width_cases as WC
from oracle import skge_oracle as O
from test_gpu_models import _batch, _model, _run, _run_logistic
from test_gpu_parity import close, close_adagrad

pytestmark = pytest.mark.gpu

MODEL_CODE = {"transe_l1": 0, "transe_l2": 1, "hole": 2, "rescal": 3}


def _ids(pred):
    return [c.id for c in WC.CASES if pred(c)]


def _assert_path(c):
    from skge_amd import _lib as L
    items = 2 * c.P if c.mode == "logistic" else c.P
    got = L.lib().skge_step_path(MODEL_CODE[c.model], int(c.mode == "logistic"), c.d, c.n_rel,
                                 items)
    assert got >= 0, L.lib().skge_last_error()
    assert (got & 255, got >> 8) == (c.path, c.km), (c.id, WC.PATH_NAMES[got & 255], got >> 8)


def _assert_init(c, m):
    """The device model starts from the tables the CPU test judged the case on."""
    want = WC.init_params(c)
    for pid, p in m.params.items():
        assert np.array_equal(p.data.cpu().numpy(), want[pid].astype(np.float32)), (c.id, pid)


def _step(c):
    n0 = len(parity_util.RECORDS)
    try:
        return _step_checked(c)
    finally:   # the headroom records of this case under its id
        parity_util.RECORDS[n0:] = [(c.id + ": " + r[0],) + tuple(r[1:])
                                    for r in parity_util.RECORDS[n0:]]


def _step_checked(c):
    _assert_path(c)
    name = WC.oracle_name(c)
    if c.mode == "pairwise":
        return _run(name, c.n_ent, c.n_rel, c.d, c.P, c.nb, margin=c.margin,
                    l1=c.model != "transe_l2", opt=c.opt)
    # HolE's E is projected (normless1) after the step: the pairwise bar, which
    # follows an element's allowance through the row's scale, for that table.
    # Measured with close_adagrad alone at d = 250: one element with oracle
    # gradient 1.4e-8 (under AdaGrad's 1e-7 floor, device 1.9e-8, row norm 0.39)
    # moves 1.6e-3, inside its own 1e-2 allowance, and rescales the 84 other
    # elements of its row past the plain bar (headroom 0.66).
    return _run_logistic(name, c.n_ent, c.n_rel, c.d, c.P, c.nb, opt=c.opt,
                         projected_by_step=True)


@pytest.mark.parametrize("cid", _ids(lambda c: c.api == "step" and c.model.startswith("transe")))
def test_transe_step(cid):
    _step(WC.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids(lambda c: c.api == "step" and c.model == "hole"))
def test_hole_step(cid):
    _step(WC.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids(lambda c: c.api == "step" and
                                     c.path == WC.RESCAL_MFMA_SMALL))
def test_rescal_mfma_step(cid):
    _step(WC.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids(lambda c: c.path == WC.RESCAL_MFMA_SORT))
def test_rescal_bucketing_step(cid):
    _step(WC.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids(lambda c: c.api == "step" and c.path == WC.RESCAL_VALU))
def test_rescal_valu_step(cid):
    _step(WC.BY_ID[cid])


def test_device_models_start_from_the_judged_tables():
    for cid in ("transe_l1-pairwise-step-d129", "hole-pairwise-step-d68",
                "rescal-pairwise-step-d130"):
        c = WC.BY_ID[cid]
        m, _ = _model(WC.oracle_name(c), c.n_ent, c.n_rel, c.d)
        _assert_init(c, m)


@pytest.mark.parametrize("cid", _ids(lambda c: c.api == "protocol"))
def test_protocol_path(cid):
    """_pairwise_gradients / _gradients, then the updaters (k_gather_mean<KM>,
    k_update_rows<KM>): the gradient rows at the plain bar plus the row
    rounding of parity_util.grad_rounding, their indices exactly, and the
    tables after the updaters as test_gpu_parity's protocol test compares them."""
    c = WC.BY_ID[cid]
    if c.model != "rescal":    # (RESCAL's protocol gradients: always the per-pair kernels)
        _assert_path(c)
    name = WC.oracle_name(c)
    m, upd = _model(name, c.n_ent, c.n_rel, c.d, margin=c.margin, l1=c.model != "transe_l2")
    params = {pid: p.data.cpu().numpy().astype(np.float64) for pid, p in m.params.items()}
    state = {pid: np.zeros_like(v) for pid, v in params.items()}
    if c.mode == "pairwise":
        pos, neg = _batch(np.random.RandomState(5), c.n_ent, c.n_rel, c.P)
        g = m._pairwise_gradients(pos, neg)
        _, _, nv, want = O.pairwise_step(name, params, state, pos, neg, 0.1, c.margin, "adagrad",
                                         **WC.oracle_kw(c))
        assert m.nviolations == nv
    else:
        pos, neg = _batch(np.random.RandomState(9), c.n_ent, c.n_rel, c.P, diff_rel=0.0)
        trip = np.concatenate([pos, neg]).astype(np.int32)
        ys = np.concatenate([np.ones(c.P), -np.ones(c.P)])
        g = m._gradients([(tuple(t), y) for t, y in zip(trip.tolist(), ys.tolist())])
        _, want_loss, want = O.logistic_step(name, params, state, trip, ys, 0.1, "adagrad")
        np.testing.assert_allclose(m.loss, want_loss, rtol=1e-5)
    assert g is not None and want is not None
    for pid, (gv, gi) in g.items():
        wg, wi = want[pid]
        np.testing.assert_array_equal(gi.cpu().numpy(), wi, err_msg=cid)
        eps = parity_util.grad_rounding(params[pid].shape, want[pid])[np.asarray(wi)]
        parity_util.check(gv, np.asarray(wg).reshape(tuple(gv.shape)), "%s grad %s" % (cid, pid),
                          atol=parity_util.ATOL + eps.reshape(tuple(gv.shape)))
    for pid in m.params:          # _batch_step: E first, then R / W
        upd[pid](*g[pid])
    for pid in m.params:
        close_adagrad(m.params[pid].data, params[pid], state[pid], 0.1, "%s %s" % (cid, pid))
        close(upd[pid].p2, state[pid], "%s p2 %s" % (cid, pid))


# ---- k_transe_pos_multi<KM>: three negatives per positive, one per mode ----

@pytest.fixture(scope="module")
def kg():
    import multineg_ref as MR
    from skge_amd.device import DeviceKG
    return DeviceKG(MR.XS, torch.device("cuda", 0))


def _both_forms(kind, d, kg, monkeypatch):
    import test_gpu_multineg as MN
    outs = {}
    for form, env in MN.FORMS.items():
        monkeypatch.setenv("SKGE_TRANSE_PAIRS", env)
        a, upd, v = MN._pair_loop_epoch(kind, d, 1, [0, 1, 2], kg)
        outs[form] = (v, {pid: p.data.cpu().numpy() for pid, p in a.params.items()},
                      {pid: upd[pid].p2.cpu().numpy() for pid in a.params})
    assert outs["pos"][0] > 0
    return outs["pos"], outs["pairs"]


@pytest.mark.parametrize("d,km", WC.MULTI_D)
def test_transe_l1_pos_multi_equals_pairs_bitwise(kg, d, km, monkeypatch):
    assert WC.km_for(d) == km
    x, y = _both_forms("transe_l1", d, kg, monkeypatch)
    assert x[0] == y[0]
    for pid in x[1]:
        assert np.array_equal(x[1][pid], y[1][pid]) and np.array_equal(x[2][pid], y[2][pid]), pid


@pytest.mark.parametrize("d,km", WC.MULTI_D)
def test_transe_l2_pos_multi_within_1e5_of_pairs(kg, d, km, monkeypatch):
    assert WC.km_for(d) == km
    x, y = _both_forms("transe_l2", d, kg, monkeypatch)
    assert x[0] == y[0]
    for pid in x[1]:
        parity_util.check(x[1][pid], y[1][pid], "pos multi l2 d%d %s" % (d, pid))
        parity_util.check(x[2][pid], y[2][pid], "pos multi l2 d%d p2 %s" % (d, pid))
