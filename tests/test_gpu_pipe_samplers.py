"""Typed and LCWA negatives on the pipelined, fused and two-launch epoch
runners (GPU; device_runner="pipe").

The KG, its pools and the record checks are those of test_gpu_samplers.py
(64 entities, 4 relations: relation 1 has one subject, relation 2 two
subjects, relation 3 -- the id n_rel - 1 -- never occurs); the replay is
test_gpu_pairloop's.  Training cases run nbatches = 3 over the first 299
triples: batches of 99, 99, 99 and 2.

  1. the runners' draw launch writes skge_epoch_sample_ex's records;
  2. pipelined (k_pipe_fused, k_pipe_batch) == two-launch, bit for bit;
  3. device_runner="pipe" == the per-batch replay of the kind's records;
  4. pool edges: an absent relation, a one-entity object pool, id n_rel - 1;
  5. the count bound sees a two-entity pool's corruptions (int16, not int8);
  6. the hot-row weight changes no bit;
  7. routing and refusals.
"""
import functools
import math

import numpy as np
import pytest
import torch

import test_gpu_pairloop as TP
import test_gpu_samplers as TS

pytestmark = pytest.mark.gpu

N, M, XS = TS.N, TS.M, TS.XS
TYPED, LCWA = TS.R.TYPED, TS.R.LCWA
KINDS = {"typed": TYPED, "lcwa": LCWA}


# ---- 1. the draw launch's records ----

def _pipe_draw(kg, n_ent, n_rel, kind, seed, key, ntries, err=0):
    """The pipelined runners' draw launch on its own: records, key copy."""
    from skge_amd import _lib as L
    dev = kg.trip.device
    ek = torch.tensor([key], dtype=torch.int64, device=dev)
    rec = torch.full((kg.T, 4), -7, dtype=torch.int32, device=dev)
    n1 = torch.full((kg.T,), -7, dtype=torch.int32, device=dev)
    errw = torch.tensor([err], dtype=torch.int32, device=dev)
    copy = torch.full((1,), -1, dtype=torch.int64, device=dev)
    L.check(L.lib().skge_pipe_epoch_sample(
        L.stream_ptr(), L.ptr(kg.trip), kg.T, L.ptr(kg.slots), kg.capacity, n_ent, seed,
        L.ptr(ek), ntries, L.ptr(rec), L.ptr(n1), kg.sampler(kind, n_rel), L.ptr(errw),
        L.ptr(copy)), "pipe draw")
    torch.cuda.synchronize()
    return rec.cpu().numpy().astype(np.int64), n1.cpu().numpy().astype(np.int64), int(copy.item())


@pytest.mark.parametrize("key", [0, 5])
@pytest.mark.parametrize("which", ["typed", "lcwa"])
def test_draw_launch_writes_the_records_of_epoch_sample_ex(kg_full, which, key):
    kind = KINDS[which]
    for ntries in (1, 100):
        rec, n1, copy = _pipe_draw(kg_full, N, M, kind, 21, key, ntries)
        want, want1 = TS._records(kg_full, kind, 21, key, ntries)
        assert np.array_equal(rec, want) and np.array_equal(n1, want1), (which, key, ntries)
        assert copy == key                      # block 0 wrote the runner's key copy
    assert (want[:, 3] >= 0).sum() > 200 and (want1 >= 0).sum() > 200   # (100 tries: drawn)
    # ntries = 0 draws none; an error word that is set draws none either
    for ntries, err in ((0, 0), (100, 2)):
        rec, n1, copy = _pipe_draw(kg_full, N, M, kind, 21, key, ntries, err)
        assert np.array_equal(rec[:, :3], want[:, :3]) and copy == key
        assert (rec[:, 3] == -1).all() and (n1 == -1).all(), (which, key, ntries, err)


def test_draw_launch_random_kind_is_the_plain_draw(kg_full):
    from skge_amd import _lib as L
    rec, n1, copy = _pipe_draw(kg_full, N, M, L.SKGE_SAMPLER_RANDOM, 77, 3, 100)
    want, want1 = TS._records(kg_full, L.SKGE_SAMPLER_RANDOM, 77, 3, 100)
    assert np.array_equal(rec, want) and np.array_equal(n1, want1) and copy == 3


@pytest.fixture(scope="module")
def kg_full():
    from skge_amd.device import DeviceKG
    return DeviceKG(XS, torch.device("cuda", 0))


# ---- 2. bitwise across runners ----

def _epoch_runner(xs, n_ent, n_rel, d, nb, kind, pipelined, width=None, seed=11, margin=2.0, **kw):
    """EpochRunner on a TransE-L1 model of width `width` (default d) whose
    first d columns are the d-wide model's and the rest zero."""
    import skge_amd as S
    from skge_amd.device import DeviceKG, EpochRunner
    np.random.seed(seed)
    m = S.TransE((n_ent, n_ent, n_rel), d)
    if width is not None and width != d:
        E0, R0 = m.E.data.clone(), m.R.data.clone()
        m = S.TransE((n_ent, n_ent, n_rel), width)
        m.E.data.zero_()
        m.R.data.zero_()
        m.E.data[:, :d].copy_(E0)
        m.R.data[:, :d].copy_(R0)
    m.add_hyperparam("margin", margin)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    r = EpochRunner(m, upd, DeviceKG(xs, m.device), nbatches=nb, seed=seed, pipelined=pipelined,
                    sampler=kind, **kw)
    assert r.pipelined == pipelined and r.sampler == kind and r.packed
    return m, upd, r


def _state(m, upd, r, d):
    r.synchronize()
    torch.cuda.synchronize()
    return {"E": m.E.data[:, :d].cpu().numpy().copy(), "R": m.R.data[:, :d].cpu().numpy().copy(),
            "pE": upd["E"].p2[:, :d].cpu().numpy().copy(),
            "pR": upd["R"].p2[:, :d].cpu().numpy().copy(),
            "nviol": int(r.nviol_total.item()), "key": int(r.epoch_key.item())}


def _same(a, b, what):
    assert a["nviol"] == b["nviol"] and a["key"] == b["key"], (what, a["nviol"], b["nviol"])
    for k in ("E", "R", "pE", "pR"):
        assert np.array_equal(a[k], b[k]), (what, k)


_REF = {}


def _two_launch(which, d):
    """The two-launch runner's tables after 2 epochs (once per case, never
    modified).  d = 50: the packed two-launch runner needs d % 4 == 0, so it
    runs the 52-wide twin whose extra columns are zero and stay zero."""
    if (which, d) not in _REF:
        m, upd, r = _epoch_runner(XS[:299], N, M, d, 3, KINDS[which], False,
                                  width=52 if d == 50 else None)
        assert r.kernel == "k_transe_sample_grad"
        r.run(2)
        _REF[(which, d)] = _state(m, upd, r, d)
        del r
    return _REF[(which, d)]


@pytest.mark.parametrize("kernel", ["k_pipe_fused", "k_pipe_batch"])
@pytest.mark.parametrize("d", [8, 50, 200])
@pytest.mark.parametrize("which", ["typed", "lcwa"])
def test_pipelined_equals_two_launch_bit_for_bit(which, d, kernel, monkeypatch):
    import skge_amd.device as DV
    assert DV.batch_sizes(299, 3) == [99, 99, 99, 2]
    monkeypatch.setenv("SKGE_PIPE_FUSED", "1" if kernel == "k_pipe_fused" else "0")
    monkeypatch.setenv("SKGE_PIPE_PAD_TO", "4")          # d = 50 -> 52
    want = _two_launch(which, d)
    m, upd, r = _epoch_runner(XS[:299], N, M, d, 3, KINDS[which], True)
    assert r.kernel == kernel
    if d == 50:
        assert r._pad and r.d_pad == 52
    r.run(2)
    got = _state(m, upd, r, d)
    del r
    assert want["nviol"] > 0 and got["key"] == 2
    _same(want, got, "%s d=%d %s" % (which, d, kernel))


# ---- 3. device_runner="pipe" against the per-batch replay ----

def _fit_pipe(kind, which, xs, sz, d, nb, epochs, seed, margin):
    import skge_amd as S
    a = TP.make_model(kind, sz, d)
    smp = (S.CorruptedSampler(1, xs, S.type_index(xs)) if which == "typed"
           else S.LCWASampler(1, [0, 1], xs, sz))
    seen = []
    tr = S.PairwiseStochasticTrainer(a, nbatches=nb, max_epochs=epochs, learning_rate=0.1,
                                     margin=margin, device_loop=True, device_runner="pipe",
                                     seed=seed, samplef=smp.sample, file_grad=None,
                                     file_embed=None,
                                     post_epoch=[lambda t: seen.append(t.nviolations) or True])
    tr.fit(xs, [1] * len(xs))
    return a, tr, seen


def _replay_twin(kind, which, xs, sz, d, nb, epochs, seed, margin, monkeypatch):
    import skge_amd as S
    import skge_amd.device as DV
    b = TP.make_model(kind, sz, d)
    b.add_hyperparam("margin", margin)
    kg = DV.DeviceKG(xs, b.device)
    monkeypatch.setattr(DV, "epoch_records",
                        functools.partial(DV.epoch_records, sampler=KINDS[which], n_rel=sz[2]))
    upd_b = {pid: S.AdaGrad(p, 0.1) for pid, p in b.params.items()}
    want_nv = TP.replay(b, upd_b, kg, sz[0], nb, epochs, seed, 100)
    torch.cuda.synchronize()
    return b, want_nv


def _check_against_replay(kind, which, xs, sz, d, nb, monkeypatch, recwarn, seed=13, margin=0.5,
                          epochs=2):
    import skge_amd.device as DV
    monkeypatch.setenv("SKGE_HOLE_DIRECT", "1")   # as test_gpu_pairloop: the replay's arithmetic
    a, tr, seen = _fit_pipe(kind, which, xs, sz, d, nb, epochs, seed, margin)
    assert not [w for w in recwarn.list if "device_loop" in str(w.message)]
    cls = DV.HolePipeRunner if kind == "hole" else DV.EpochRunner
    assert type(tr._runner) is cls and tr._runner.sampler == KINDS[which]
    if kind == "transe_l2":
        assert not tr._runner.pipelined and tr._runner.kernel == "k_transe_sample_grad"
    else:
        assert tr._runner.pipelined
    b, want_nv = _replay_twin(kind, which, xs, sz, d, nb, epochs, seed, margin, monkeypatch)
    print("%s %s: violations %r want %d" % (kind, which, seen, want_nv))
    for pid in a.params:
        err = float((a.params[pid].data - b.params[pid].data).abs().max().item())
        print("%s %s %s: max |diff| %.3g" % (kind, which, pid, err))
    assert sum(seen) == want_nv and want_nv > 0
    for pid in a.params:
        np.testing.assert_allclose(a.params[pid].data.cpu().numpy(),
                                   b.params[pid].data.cpu().numpy(), rtol=TP.RTOL, atol=TP.ATOL,
                                   err_msg="%s %s %s" % (kind, which, pid))


@pytest.mark.parametrize("which", ["typed", "lcwa"])
@pytest.mark.parametrize("kind", ["transe_l1", "transe_l2", "hole"])
def test_pipe_runner_equals_replay(kind, which, monkeypatch, recwarn):
    _check_against_replay(kind, which, XS[:299], (N, N, M), TS.D, 3, monkeypatch, recwarn)


# ---- 4. pool edges in one KG ----

EN, EM = 40, 5
ONE_OBJ = 30          # relation 1's only object


def _edge_kg():
    """Relation 0: broad.  Relation 1: twelve subjects, the one object 30 --
    every typed o-corruption draws 30, a known triple, so o' = -1 for all of
    them (and every s-corruption is another subject of 30: s' = -1 too).
    Relation 2: absent (two empty pools).  Relation 3: a few triples.
    Relation 4 = n_rel - 1: eight triples."""
    xs = [(s, ONE_OBJ, 1) for s in range(12)]
    xs += [(s, 20 + s, 4) for s in range(8)] + [(s, s + 1, 3) for s in range(5)]
    rs = np.random.RandomState(2)
    seen = set()
    while len(xs) < 131:
        t = (int(rs.randint(EN)), int(rs.randint(EN)), 0)
        if t not in seen:
            seen.add(t)
            xs.append(t)
    return xs


EDGE = _edge_kg()


@pytest.mark.parametrize("which", ["typed", "lcwa"])
def test_pool_edge_records(which):
    from skge_amd.device import DeviceKG
    kind = KINDS[which]
    kg = DeviceKG(EDGE, torch.device("cuda", 0))
    off = kg.pools(EM)[0].cpu().numpy()
    assert off[4] == off[5] == off[6]                   # relation 2: two empty pools
    assert off[4] - off[3] == 1                         # relation 1's object pool: {30}
    assert off[10] - off[9] == 8                        # the last relation's pools end the CSR
    rec, n1, _ = _pipe_draw(kg, EN, EM, kind, 5, 1, 100)
    want, want1 = TS.R.replay_records(kind, EDGE, _perm(kg, 5, 1), 5, 1,
                                      TS._pools_numpy(EDGE, EM), 100, EN)
    assert np.array_equal(rec, want) and np.array_equal(n1, want1)
    r1, r4 = rec[:, 2] == 1, rec[:, 2] == 4
    assert r1.sum() == 12 and r4.sum() == 8 and not (rec[:, 2] == 2).any()
    assert (rec[r1, 3] == -1).all()                     # every subject is known with 30
    if kind == TYPED:
        assert (n1[r1] == -1).all()                     # the pool's one object is known
        assert (n1[r4] >= 20).all() and (n1[r4] < 28).all() and (n1[r4] != rec[r4, 1]).all()
    assert (rec[r4, 3] >= 0).all() and (rec[r4, 3] < 8).all()


def _perm(kg, seed, key):
    return TS._perm(kg, seed, key)


@pytest.mark.parametrize("which", ["typed", "lcwa"])
@pytest.mark.parametrize("kind", ["transe_l1", "hole"])
def test_pool_edge_epoch_equals_replay(kind, which, monkeypatch, recwarn):
    import skge_amd.device as DV
    assert DV.batch_sizes(len(EDGE), 2) == [65, 65, 1]
    _check_against_replay(kind, which, EDGE, (EN, EN, EM), 8, 2, monkeypatch, recwarn, epochs=1)


# ---- 5. / 6. the count bound and the hot rows ----

BN, HALF = 1024, 34
ROW_A, ROW_B = 1000, 1001


def _bound_kg(copies=1):
    """`copies` x: relation 0 with 68 subjects, 34 linked to object a and 34
    to b (neither a subject): its object pool is {a, b}; and 60 filler triples
    of relation 1 over distinct entities.  copies > 1 repeats the subjects on
    fresh entities (the same a and b), for more than one batch."""
    xs = []
    for c in range(copies):
        base = 200 * c
        xs += [(base + i, ROW_A if i < HALF else ROW_B, 0) for i in range(2 * HALF)]
        xs += [(base + 70 + i, base + 130 + i, 1) for i in range(60)]
    return xs


def _old_uniform_bound(xs, n_ent, batch, tail):
    """The count bound before it knew pool draws: corruptions uniform over
    all entities (lambda = 2 batch / n_ent)."""
    T, B = float(len(xs)), float(min(batch, len(xs)))
    a = np.asarray(xs)

    def per_batch(col):
        c = np.bincount(col, minlength=n_ent).astype(np.float64)
        return np.minimum(np.minimum(c, B), tail(c * (B / T)))
    occ = per_batch(a[:, 0]) + per_batch(a[:, 1])
    det = 3 * min(int(math.ceil(float(occ.max()))), 2 * int(batch))
    return det + min(2 * int(batch), int(math.ceil(tail(2.0 * batch / n_ent))))


def _record_counts(rec, n1, n_ent):
    """A row's largest possible count from the epoch's records: a positive
    with both negatives adds 3 to its s and o (skge/transe.py:103-136), one
    per accepted corruption."""
    has0, has1 = (rec[:, 3] >= 0).astype(np.int64), (n1 >= 0).astype(np.int64)
    cnt = np.bincount(rec[:, 0], weights=has0 + 2 * has1, minlength=n_ent)
    cnt += np.bincount(rec[:, 1], weights=2 * has0 + has1, minlength=n_ent)
    cnt += np.bincount(rec[has0 > 0, 3], minlength=n_ent)
    cnt += np.bincount(n1[has1 > 0], minlength=n_ent)
    return cnt.astype(np.int64)


def test_count_bound_sees_the_two_entity_pool():
    import skge_amd.device as DV
    xs = _bound_kg()
    T = len(xs)
    assert T == 128
    # premises: the uniform bound admits int8 sums, the records do not
    old8 = _old_uniform_bound(xs, BN, T, lambda m: m + 8.0 * m ** 0.5 + 20.0)
    print("uniform-corruption bound (int8 tail): %d" % old8)
    assert old8 <= 127
    kg = DV.DeviceKG(xs, torch.device("cuda", 0))
    rec, n1 = DV.epoch_records(kg, BN, 11, 0, 100, sampler=TYPED, n_rel=2)
    torch.cuda.synchronize()
    cnt = _record_counts(rec.cpu().numpy().astype(np.int64), n1.cpu().numpy().astype(np.int64), BN)
    print("row a: count %d, row b: %d" % (cnt[ROW_A], cnt[ROW_B]))
    assert cnt[ROW_A] == 3 * HALF + HALF == 136
    new8 = DV.packed_count_bound(kg, BN, T, DV._tail8, sampler=TYPED, n_rel=2)
    new16 = DV.packed_count_bound(kg, BN, T, sampler=TYPED, n_rel=2)
    print("per-row bound: int8 tail %d, int16 tail %d" % (new8, new16))
    assert new8 >= 136 and new16 >= 136
    assert DV.packed_count_bound(kg, BN, T, DV._tail8) == old8      # RANDOM: as it was
    # the runner chooses int16 sums up front, and its epoch is the two-launch runner's
    out = []
    for pipelined in (False, True):
        m, upd, r = _epoch_runner(xs, BN, 2, 200, 1, TYPED, pipelined)
        if pipelined:
            assert r.kernel == "k_pipe_batch" and r.ent_i8 is False and r.count_bound >= 136
        r.run(1)
        out.append(_state(m, upd, r, 200))              # synchronize(): the error word is clean
        del r
    assert out[0]["nviol"] > 0
    _same(out[0], out[1], "two-entity pool")


def test_hot_row_weight_changes_no_bit(monkeypatch):
    """The KG of the bound test three times over (batches of 128): rows a and
    b are hubs by occurrence already; relation 2's object pool {c, d} is a hub
    only through its negatives (8 occurrences each, below the bar of 12; with
    the 8 corruptions an epoch sends each of them, above it)."""
    c, d = 1010, 1011
    xs = _bound_kg(3)
    xs = xs[:-16] + [(900 + i, c if i < 8 else d, 2) for i in range(16)]
    assert len(xs) == 384
    out, hot = [], []
    for flag in ("0", "1"):
        monkeypatch.setenv("SKGE_PIPE_HOT_NEG", flag)
        m, upd, r = _epoch_runner(xs, BN, 3, 200, 3, TYPED, True)
        assert r.kernel == "k_pipe_batch" and not r.ent_i8
        hot.append(r.hot_rows)
        r.run(2)
        out.append(_state(m, upd, r, 200))
        del r
    print("hot rows: occurrences only %d, with the corruption weight %d" % tuple(hot))
    assert hot[0] == 2 and hot[1] == 4
    assert out[0]["nviol"] > 0
    _same(out[0], out[1], "hot-row weight")


# ---- 7. routing and refusals ----

def test_pipe_refuses_rescal_and_other_negatives():
    import skge_amd as S
    for kind, n, dn in (("rescal", 1, False), ("transe_l1", 2, True)):
        m = TP.make_model(kind, (N, N, M), TS.D)
        smp = S.CorruptedSampler(n, XS, S.type_index(XS))
        tr = S.PairwiseStochasticTrainer(m, nbatches=3, max_epochs=1, margin=1.0, device_loop=True,
                                         device_runner="pipe", device_negatives=dn,
                                         samplef=smp.sample, file_grad=None, file_embed=None)
        with pytest.raises(ValueError, match="'pairs'"):
            tr.fit(XS, [1] * len(XS))


def test_dp_form_refuses_a_pool_sampler_without_a_launch(kg_full):
    import skge_amd as S
    from skge_amd import _lib as L
    from skge_amd.device import EpochRunner
    lib, dev = L.lib(), kg_full.trip.device
    m = TP.make_model("transe_l1", (N, N, M), TS.D)
    m.add_hyperparam("margin", 1.0)
    upd = {pid: S.SGD(p, 0.1) for pid, p in m.params.items()}
    good = EpochRunner(m, upd, kg_full, 3, pipelined=True)       # its tables are what the entry takes
    E0 = m.E.data.clone()
    ek = torch.zeros(1, dtype=torch.int64, device=dev)
    nv = torch.zeros(1, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    args = (L.stream_ptr(st), good.te, good.tr, TS.D, L.ptr(kg_full.trip), kg_full.T,
            L.ptr(kg_full.slots), kg_full.capacity, 3, 1, L.ptr(ek), 1.0, 100, L.ptr(nv))
    h = lib.skge_pipe_runner_create_smp(*args, 1, kg_full.sampler(TYPED, M))
    assert not h and b"SKGE_PIPE_DP" in lib.skge_last_error()
    bad = L.SkgeSampler(7, M, None, None)
    h = lib.skge_pipe_runner_create_smp(*args, 0, bad)
    assert not h and b"kind" in lib.skge_last_error()
    torch.cuda.synchronize()
    assert torch.equal(E0, m.E.data) and int(nv.item()) == 0 and int(ek.item()) == 0
