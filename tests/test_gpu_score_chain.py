"""The scoring wave of k_pipe_batch after its load burst was reordered
(csrc/skge_pipeline.hip: the relation row's loads first, its update behind a
partial wait while the entity rows are in flight; csrc/skge_pipe.h
rel_row_issue / rel_row_finish), bit for bit against the two-launch runner.

Every case trains 2 epochs on a tiny KG with both runners and compares E, R,
both AdaGrad states and the violation total with torch.equal; the pipelined
runner is forced onto k_pipe_batch (SKGE_PIPE_FUSED=0) and every case asserts
the instance it got.  The shapes are the smallest at which the reorder can go
wrong:

  d = 4      one quad: 63 lanes past the row
  d = 200    lanes 50-63 past the row must enter the scores as zeros
  d = 260    two quads per lane (KQ = 2)
  nb         batches of 50 positives (fewer than a wave's 64 lanes) and of 333
  |R| = 1    every wave recomputes the same relation row
  rare       a relation with three triples: most batches do not touch it, so a
             wave that scores with it finds its count 0 (the branch of the
             finish half that zeroes the lanes past the row without an update;
             the first batch of every epoch takes it for every relation)
  SGD        no AdaGrad state (null state pointers)
  W32        int32x2 relation sums need more than 8191 positives of one
             relation in a batch (4 x count > 32767), so this one case has
             T = 9,000 in one batch over 300 entities -- the only case above
             2,000 triples; it also runs the owner-mark (GRP) instance
  zipf       bench.make_zipf_kg at 300 entities: hub rows, the HOT instance
  DP         the data-parallel form at world size 1
  |E| = 32   nearly every scoring wave finds pending rows: claim, wait and
             re-read after the reordered burst; the error word must be 0
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPOCHS = 2
SEED = 11


def _uniform_kg(n_ent, n_rel, T, seed=3):
    rs = np.random.RandomState(seed)
    seen, out = set(), []
    while len(out) < T:
        t = (int(rs.randint(n_ent)), int(rs.randint(n_ent)), int(rs.randint(n_rel)))
        if t not in seen:
            seen.add(t)
            out.append(t)
    return np.array(out, dtype=np.int32)


def _rare_kg():
    """1000 triples over 4 relations and three more of relation 4."""
    trip = _uniform_kg(300, 4, 1000)
    trip[[100, 500, 900], 2] = 4
    return trip


_KGS = {}


def _kg(kind):
    """(entities, relations, triples) of a named KG, built once."""
    if kind not in _KGS:
        if kind == "zipf":
            from bench import make_zipf_kg
            _KGS[kind] = (300, 5, make_zipf_kg(300, 5, 2000, seed=3))
        elif kind == "rare":
            _KGS[kind] = (300, 5, _rare_kg())
        elif kind == "one_rel":
            _KGS[kind] = (300, 1, _uniform_kg(300, 1, 1000))
        elif kind == "one_rel_9000":
            _KGS[kind] = (300, 1, _uniform_kg(300, 1, 9000))
        elif kind == "e32":
            _KGS[kind] = (32, 5, _uniform_kg(32, 5, 1000))
        else:
            _KGS[kind] = (300, 5, _uniform_kg(300, 5, 1000))
    return _KGS[kind]


def _model(n_ent, n_rel, d, opt):
    import skge_amd as S
    np.random.seed(SEED)
    m = S.TransE((n_ent, n_ent, n_rel), d)
    m.add_hyperparam("margin", 2.0)
    if n_rel == 1:   # the reference's initialisers squeeze a one-row table to a vector
        m.R.data = m.R.data.reshape(1, d).contiguous()
    make =S.AdaGrad if opt == "adagrad" else S.SGD
    return m, {pid: make(p, 0.1) for pid, p in m.params.items()}


def _state(m, upd, nviol):
    out = {"E": m.E.data.detach().cpu().clone(), "R": m.R.data.detach().cpu().clone(),
           "nviol": int(nviol)}
    for pid in ("E", "R"):
        p2 = getattr(upd[pid], "p2", None)
        if p2 is not None:
            out["p" + pid] = p2.detach().cpu().clone()
    return out


def _error_word(r):
    from skge_amd import _lib as L
    r.stream.synchronize()
    return L.lib().skge_pipe_runner_error(r.handle, L.stream_ptr(r.stream))


def _train(kind, d, nb, opt, pipelined):
    from skge_amd.device import DeviceKG, EpochRunner
    n_ent, n_rel, trip = _kg(kind)
    m, upd = _model(n_ent, n_rel, d, opt)
    r = EpochRunner(m, upd, DeviceKG(trip, m.device), nbatches=nb, seed=SEED, pipelined=pipelined)
    assert r.pipelined == pipelined
    r.run(EPOCHS)
    r.synchronize()
    info = None
    if pipelined:
        info = {"kernel": r.kernel, "e8": bool(r.ent_i8), "w32": bool(r.rel_w32),
                "hot": int(r.hot_rows), "err": _error_word(r)}
    out = _state(m, upd, r.nviol_total.item())
    del r
    return out, info


_REF = {}


def _reference(kind, d, nb, opt):
    """The two-launch runner's tables after EPOCHS epochs (computed once per
    geometry, never modified)."""
    key = (kind, d, nb, opt)
    if key not in _REF:
        _REF[key] = _train(kind, d, nb, opt, pipelined=False)[0]
    return _REF[key]


def _same(got, want):
    assert got["nviol"] == want["nviol"] > 0, (got["nviol"], want["nviol"])
    assert set(got) == set(want)
    for k in want:
        if k != "nviol":
            assert torch.equal(got[k], want[k]), k


# (kg, d, nb, optimiser, what the instance must be: int32x2 relation sums, hot rows)
CASES = [
    ("uniform", 4, 3, "adagrad", False, False),      # one quad, 63 lanes past the row
    ("uniform", 4, 20, "adagrad", False, False),
    ("uniform", 200, 20, "adagrad", False, False),   # 50 positives per batch (< 64)
    ("uniform", 200, 3, "adagrad", False, False),    # 333 per batch, ragged last batch
    ("uniform", 260, 20, "adagrad", False, False),   # KQ = 2
    ("uniform", 260, 3, "adagrad", False, False),
    ("one_rel", 200, 3, "adagrad", False, False),    # every wave recomputes the same row
    ("rare", 200, 10, "adagrad", False, False),      # count 0 at the finish half
    ("rare", 260, 10, "adagrad", False, False),
    ("uniform", 200, 3, "sgd", False, False),        # null state pointers
    ("uniform", 260, 20, "sgd", False, False),
    ("one_rel_9000", 200, 1, "adagrad", True, False),   # W32 (and owner marks)
    ("zipf", 200, 5, "adagrad", False, True),        # the HOT instance
]


@pytest.mark.parametrize("kind,d,nb,opt,w32,hot", CASES)
def test_reordered_scoring_wave_equals_two_launch(kind, d, nb, opt, w32, hot, monkeypatch):
    monkeypatch.setenv("SKGE_PIPE_FUSED", "0")
    want = _reference(kind, d, nb, opt)
    got, info = _train(kind, d, nb, opt, pipelined=True)
    assert info["kernel"] == "k_pipe_batch"
    assert info["w32"] == w32
    assert (info["hot"] > 0) == hot, info["hot"]
    if hot:
        assert not info["e8"]   # hub rows leave the int8 range
    assert info["err"] == 0
    _same(got, want)


def test_rare_relation_is_absent_from_most_batches():
    """The rare-relation KG is what its cases say: relation 4 has three
    triples, so at most three of an epoch's ten batches touch it."""
    _, _, trip = _kg("rare")
    assert int((trip[:, 2] == 4).sum()) == 3


@pytest.mark.parametrize("d,nb", [(200, 3), (260, 20)])
def test_pending_rows_with_few_entities(d, nb, monkeypatch):
    """32 entities: with 50 or 333 positives per batch nearly every row a
    wave reads was touched by the previous batch."""
    monkeypatch.setenv("SKGE_PIPE_FUSED", "0")
    want = _reference("e32", d, nb, "adagrad")
    got, info = _train("e32", d, nb, "adagrad", pipelined=True)
    assert info["kernel"] == "k_pipe_batch"
    assert info["err"] == 0
    _same(got, want)


@pytest.mark.parametrize("d,nb", [(200, 3), (260, 20), (4, 3)])
def test_data_parallel_world_1_equals_two_launch(d, nb):
    """The DP instance of k_pipe_batch (a slice of the batch scored, records
    written, k_pipe_dp_scatter) with one rank and no group."""
    from skge_amd.device import DeviceKG
    from skge_amd.dp import DataParallelRunner
    n_ent, n_rel, trip = _kg("uniform")
    want = _reference("uniform", d, nb, "adagrad")
    m, upd = _model(n_ent, n_rel, d, "adagrad")
    r = DataParallelRunner(m, upd, DeviceKG(trip, m.device), nb, seed=SEED, group=None)
    r.run(EPOCHS)
    r.synchronize()
    assert _error_word(r) == 0
    got = _state(m, upd, r.total_violations())
    del r
    _same(got, want)
