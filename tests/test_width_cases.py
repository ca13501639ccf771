"""CPU checks of the row-width case table (tests/width_cases.py): every case
reaches the path it names under the restated selection rules (and under the
library's own skge_step_path, which answers without a GPU), every (kernel
family, KM) instantiation the table is there for is reached, and the oracle
step of each case's first batch is neither vacuous nor slow."""
import time

import numpy as np
import pytest

import width_cases as WC
from oracle import skge_oracle as O
from test_gpu_models import _batch

IDS = [c.id for c in WC.CASES]
MODEL_CODE = {"transe_l1": 0, "transe_l2": 1, "hole": 2, "rescal": 3}


def test_restated_rules_at_their_edges():
    assert [WC.km_for(d) for d in (1, 64, 65, 128, 129, 192, 193, 256, 257, 512, 513, 1024, 1025)] \
        == [1, 1, 2, 2, 3, 3, 4, 4, 8, 8, 16, 16, 0]
    assert WC.hole_fast(256) and not WC.hole_fast(260) and not WC.hole_fast(250)
    assert [d for d in (68, 100, 128, 132, 160, 192, 240, 252, 256) if WC.hole_fft_ok(d)] \
        == [100, 128, 160, 192, 240]
    assert WC.rescal_mfma_ok(1024, 8192) and not WC.rescal_mfma_ok(8, 8193)
    assert WC.rs_small_bucket(256, 1024) and not WC.rs_small_bucket(257, 400)
    assert not WC.rs_small_bucket(100, 1025)
    assert WC.generic_lds_bytes(16) == 96 * 1024
    assert WC.rs_scan_lds_bytes(8192) == 65540


@pytest.mark.parametrize("cid", IDS)
def test_case_reaches_its_path(cid):
    c = WC.BY_ID[cid]
    if c.api == "protocol" and c.model == "rescal":
        # the protocol's RESCAL gradients come from the per-pair kernels at any shape
        assert (c.path, c.km) == (WC.RESCAL_VALU, WC.km_for(c.d))
    else:
        assert WC.step_path(c.model, c.mode, c.d, c.n_rel, _items(c)) == (c.path, c.km)


def _items(c):
    return 2 * c.P if c.mode == "logistic" else c.P


@pytest.mark.parametrize("cid", [c.id for c in WC.CASES if c.api == "step"])
def test_library_agrees_with_the_table(cid):
    from skge_amd import _lib as L
    c = WC.BY_ID[cid]
    got = L.load().skge_step_path(MODEL_CODE[c.model], int(c.mode == "logistic"), c.d, c.n_rel,
                                  _items(c))
    assert got >= 0, L.load().skge_last_error()
    assert (got & 255, got >> 8) == (c.path, c.km), (WC.PATH_NAMES[got & 255], got >> 8)


def test_every_family_and_width_is_reached():
    reached = set()
    for c in WC.CASES:
        reached |= WC.families(c)
    assert not WC.REQUIRED - reached, sorted(WC.REQUIRED - reached)
    assert [WC.km_for(d) for d, _ in WC.MULTI_D] == [k for _, k in WC.MULTI_D] == list(WC.WIDE)


def test_bucketing_cases_sit_on_their_branches():
    by = {(c.n_rel, c.P): c for c in WC.CASES if c.path == WC.RESCAL_MFMA_SORT
          and c.mode == "pairwise"}
    assert set(by) == {(100, 600), (300, 200), (8192, 300)}
    assert WC.rs_memset_branch(100, 1200) and 1200 > WC.SB_MAXN and 100 <= WC.SB_MAXM
    assert WC.rs_memset_branch(300, 400) and 400 <= WC.SB_MAXN     # sorted because M > 256
    assert WC.rs_scan_lds_bytes(8192) > 64 * 1024
    # every other MFMA case buckets in the one-workgroup kernel
    assert all(c.path == WC.RESCAL_MFMA_SMALL for c in WC.CASES
               if c.model == "rescal" and c.api == "step" and c.d > 8
               and c.path != WC.RESCAL_VALU)


def test_split_cases_land_on_each_side_of_rs_wsplit():
    sp = {c.id: WC.rs_wsplit(2 * c.P, c.n_rel, c.d) for c in WC.CASES
          if c.model == "rescal" and c.d == 260 and c.api == "step"}
    assert len(sp) == 4
    for cid, s in sp.items():
        assert (s == 1) == cid.endswith("-split1") and (s > 1) == cid.endswith("-splitk"), (cid, s)


@pytest.mark.parametrize("cid", IDS)
def test_oracle_step_is_not_vacuous_and_quick(cid):
    c = WC.BY_ID[cid]
    params = WC.init_params(c)
    state = {k: np.zeros_like(v) for k, v in params.items()}
    name = WC.oracle_name(c)
    if c.mode == "pairwise":
        pos, neg = _batch(np.random.RandomState(5), c.n_ent, c.n_rel, c.P)
        t0 = time.perf_counter()
        _, _, nv, grads = O.pairwise_step(name, params, state, pos, neg, 0.1, c.margin, c.opt,
                                          **WC.oracle_kw(c))
        dt = time.perf_counter() - t0
        assert 0 < nv < c.P, (nv, c.P)
    else:
        pos, neg = _batch(np.random.RandomState(9), c.n_ent, c.n_rel, c.P, diff_rel=0.0)
        trip = np.concatenate([pos, neg]).astype(np.int32)
        ys = np.concatenate([np.ones(c.P), -np.ones(c.P)])
        t0 = time.perf_counter()
        _, loss, grads = O.logistic_step(name, params, state, trip, ys, 0.1, c.opt)
        dt = time.perf_counter() - t0
        assert np.isfinite(loss) and loss > 0
        for pid, (g, idx) in grads.items():
            g = np.asarray(g).reshape(len(idx), -1)
            assert len(idx) > 0 and (np.abs(g).max(axis=1) > 0).all(), pid
    # (a pairwise row may cancel exactly: a pair whose negative equals its positive)
    assert all(len(idx) > 0 and np.abs(np.asarray(g)).max() > 0 for g, idx in grads.values())
    print("%s: oracle step %.3f s" % (cid, dt))
    assert dt < 2.0, dt
