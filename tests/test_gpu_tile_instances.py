"""The template instances of the shared score tile and list epilogue, pinned
to each other on float tables.

The selection kernels pick their query block from k (skge_topk: 64 vectors
for k <= 32, else 32; skge_neighbours: 128 / 64 / 32 at k <= 16 / 32 / above),
and every instance has to run the same fp32 chain: the list order is total
(descending score, then ascending id), so the first entries of a longer list
are the shorter list, BIT FOR BIT.  The integer-table tests cannot see a
reordered chain and the float tests allow an envelope; these cannot pass with
one.

Shapes: d = 33 is no multiple of the 16-byte load and spans two 32-dim chunks
(d = 64: the 16-byte path); N = 300 is three candidate tiles, the last
partial, in three slices, so the merge runs; 70 queries (140 neighbour rows)
leave a partial query block at every block size.
"""
import numpy as np
import pytest
import torch

import eval_ref as X
import neighbours_ref as NR

pytestmark = pytest.mark.gpu

N, NQ = 300, 70
# (name, model, squared-L2 scoring)
SCORERS = [("transe", "transe", False), ("transe-l2", "transe", True), ("hole", "hole", False),
           ("rescal", "rescal", False)]


def _predictor(name, model, l2, d):
    """A LinkPredictor over fixed-seed float tables, its test triples (s, o, p)."""
    import skge_amd as S
    E, R, test, known = X.make_float_case(model, d, 1.0, X.case_seed("tile-instances", name, d),
                                          N=N, nq=NQ)
    cls = {"transe": S.TransE, "hole": S.HolE, "rescal": S.RESCAL}[model]
    m = cls((N, N, R.shape[0]), d, init="device_nunif", **({"l1": False} if l2 else {}))
    rid = "W" if model == "rescal" else "R"
    assert m.params["E"].shape == E.shape and m.params[rid].shape == R.shape
    m.params["E"].data.copy_(torch.tensor(E, dtype=torch.float32))
    m.params[rid].data.copy_(torch.tensor(R, dtype=torch.float32))
    return S.LinkPredictor(m, known, scoring="model" if l2 else "eval"), test


def _assert_prefix(short, long, what):
    n = short[0].shape[1]
    assert short[0].shape[0] == long[0].shape[0] and long[0].shape[1] > n
    np.testing.assert_array_equal(short[0], long[0][:, :n], err_msg="ids, " + what)
    assert short[1].tobytes() == np.ascontiguousarray(long[1][:, :n]).tobytes(), "scores, " + what


def _both_blocks(lp, test, what, **kw):
    """k = 32 (query block 64) against the first 32 of k = 33 (query block 32),
    both directions, with the known answers excluded and without."""
    for fn, anchor in ((lp.tails, test[:, 0]), (lp.heads, test[:, 1])):
        for filtered in (True, False):
            a = fn(anchor, test[:, 2], k=32, filtered=filtered, **kw)
            b = fn(anchor, test[:, 2], k=33, filtered=filtered, **kw)
            assert (a[0] >= 0).all()
            _assert_prefix(a, b, "%s %s filtered=%s" % (what, fn.__name__, filtered))


@pytest.mark.parametrize("d", [33, 64])
@pytest.mark.parametrize("name,model,l2", SCORERS)
def test_topk_query_blocks_agree(name, model, l2, d):
    lp, test = _predictor(name, model, l2, d)
    _both_blocks(lp, test, "%s d=%d" % (name, d))


@pytest.mark.parametrize("d", [33, 64])
@pytest.mark.parametrize("name,model,l2", SCORERS)
def test_topk_pools_query_blocks_agree(name, model, l2, d):
    """The gathered instances: one pool of 200 ids, every third query on pool -1."""
    lp, test = _predictor(name, model, l2, d)
    rs = np.random.RandomState(X.case_seed("tile-instances-pool", name, d))
    pool = np.sort(rs.choice(N, 200, replace=False))
    query_pool = np.where(np.arange(NQ) % 3 == 0, -1, 0)
    _both_blocks(lp, test, "%s d=%d pools" % (name, d), candidates=([pool], query_pool))


@pytest.mark.parametrize("metric", NR.METRICS)
def test_neighbour_query_blocks_agree(metric):
    """k = 16, 17 and 33: the 128-, 64- and 32-query instances."""
    import skge_amd as S
    carrier = S.TransE((4, 4, 2), 4, init="device_nunif")   # the device the table is put on
    nn = S.Neighbours(carrier, table=NR.make_float_table(N, 33, 503).astype(np.float32),
                      metric=metric)
    rows = np.arange(2 * NQ)
    got = {k: nn.topk(k=k, rows=rows) for k in (16, 17, 33)}
    _assert_prefix(got[16], got[17], "%s k 16 / 17" % metric)
    _assert_prefix(got[17], got[33], "%s k 17 / 33" % metric)
