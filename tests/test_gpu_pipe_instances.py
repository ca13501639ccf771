"""The k_pipe_batch instances whose occupancy is pinned (csrc/skge_pipeline.hip
pipe_batch_waves) and their neighbours, bit for bit against the two-launch
runner.

300 entities and batches of 333 positives: nearly every row batch b reads is
pending from batch b-1, so the claim, wait and re-read paths of the hand-off
all run.  nb = 3 leaves a ragged last batch (333, 333, 334), nb = 1 is a batch
and the flush alone.  d = 200 is one quad per lane with int8 entity sums (the
flagship's instance) or, with SKGE_PIPE_E8=0, int16 sums; d = 260 is two quads
per lane.  A Zipf KG of 2,000 entities runs the hot-row instance.  Every case
asserts the runner it got (pipelined, k_pipe_batch, the sum encoding, hot rows),
so none can pass through another path.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPOCHS = 2


def _uniform_kg(n_ent, n_rel, T, seed=3):
    rs = np.random.RandomState(seed)
    seen, out = set(), []
    while len(out) < T:
        t = (int(rs.randint(n_ent)), int(rs.randint(n_ent)), int(rs.randint(n_rel)))
        if t not in seen:
            seen.add(t)
            out.append(t)
    return np.array(out, dtype=np.int32)


def _kg(kind):
    if kind == "zipf":
        from bench import make_zipf_kg
        return 2000, 11, make_zipf_kg(2000, 11, 12000, seed=3)
    return 300, 5, _uniform_kg(300, 5, 1000)


def _runner(trip, n_ent, n_rel, d, nb, pipelined):
    import skge_amd as S
    from skge_amd.device import DeviceKG, EpochRunner
    np.random.seed(11)
    m = S.TransE((n_ent, n_ent, n_rel), d)
    m.add_hyperparam("margin", 2.0)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    r = EpochRunner(m, upd, DeviceKG(trip, m.device), nbatches=nb, seed=11,
                    pipelined=pipelined)
    assert r.pipelined == pipelined
    return m, upd, r


def _state(m, upd, r):
    r.synchronize()
    return {"E": m.E.data.cpu().numpy().copy(), "R": m.R.data.cpu().numpy().copy(),
            "pE": upd["E"].p2.cpu().numpy().copy(), "pR": upd["R"].p2.cpu().numpy().copy(),
            "nviol": int(r.nviol_total.item())}


def _same(a, b, what):
    assert a["nviol"] == b["nviol"], (what, a["nviol"], b["nviol"])
    for k in ("E", "R", "pE", "pR"):
        assert np.array_equal(a[k], b[k]), (what, k)


_REF = {}


def _reference(kind, d, nb):
    """The two-launch runner's tables after EPOCHS epochs (computed once per
    geometry, never modified)."""
    key = (kind, d, nb)
    if key not in _REF:
        n_ent, n_rel, trip = _kg(kind)
        m, upd, r = _runner(trip, n_ent, n_rel, d, nb, pipelined=False)
        r.run(EPOCHS)
        _REF[key] = _state(m, upd, r)
        del r
    return _REF[key]


# (kg, d, nb, int8 entity sums asked for, hot rows expected)
CASES = [
    ("uniform", 200, 3, True, False),    # the flagship's instance, ragged last batch
    ("uniform", 200, 1, True, False),    # one batch and the flush
    ("uniform", 260, 3, True, False),    # two quads per lane
    ("uniform", 260, 1, True, False),
    ("uniform", 200, 3, False, False),   # int16 entity sums
    ("uniform", 200, 1, False, False),
    ("zipf", 200, 10, True, True),       # hub rows: the hot-row instance (int16 sums)
]


@pytest.mark.parametrize("kind,d,nb,e8,hot", CASES)
def test_pipe_batch_instance_equals_two_launch(kind, d, nb, e8, hot, monkeypatch):
    if not e8:
        monkeypatch.setenv("SKGE_PIPE_E8", "0")
    n_ent, n_rel, trip = _kg(kind)
    ref = _reference(kind, d, nb)
    assert ref["nviol"] > 0

    m, upd, r = _runner(trip, n_ent, n_rel, d, nb, pipelined=True)
    assert r.pipelined and r.kernel == "k_pipe_batch"
    # hub rows leave the int8 range: the runner itself picks int16 sums there
    assert r.ent_i8 == (e8 and not hot)
    assert (r.hot_rows > 0) == hot, r.hot_rows
    r.run(EPOCHS)
    one = _state(m, upd, r)
    del r
    _same(ref, one, "run(%d) against the two-launch runner" % EPOCHS)

    m, upd, r = _runner(trip, n_ent, n_rel, d, nb, pipelined=True)
    for _ in range(EPOCHS):
        r.run(1)
    two = _state(m, upd, r)
    del r
    _same(one, two, "run(1) x %d against run(%d)" % (EPOCHS, EPOCHS))
