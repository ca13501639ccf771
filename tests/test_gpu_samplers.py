"""Typed (CorruptedSampler) and LCWA negatives in the device epochs (GPU).

The records skge_epoch_sample_ex draws are compared exactly with a host
replay of the draws' definition (tests/sampler_ref.py: the device's own epoch
permutation, a Python set as the rejection set, the type index as CSR arrays
built here in numpy) and checked for the properties the samplers promise;
the pair loop and the logistic loop trained with them through the trainers
are compared with the replays of tests/test_gpu_pairloop.py and
tests/test_gpu_logistic_loop.py fed the same records, at those files'
tolerances.

Test KG: 64 entities, 4 relations, 300 triples (more than one 256-thread
block).  Relation 0 is broad (240 random triples).  Relation 1 has the one
subject 7: a typed or LCWA s-corruption can only draw 7 itself, so none
exists.  Relation 2 has the two subjects 3 and 9: objects 0-9 are known with
both (no s-corruption exists), 10-19 with 3 only and 20-29 with 9 only (the
s-corruption is the other subject).  Relation 3 never occurs: empty pools.

The training cases run nbatches = 3 over the KG's first 299 triples (batches
of 99, 99, 99 and a remainder of 2; 300 would split evenly), which drops one
of relation 0's triples and leaves the structure above as it is.
"""
import functools

import numpy as np
import pytest
import torch

import parity_util
import sampler_ref as R
import test_gpu_logistic_loop as TL
import test_gpu_pairloop as TP

pytestmark = pytest.mark.gpu

N, M, D, T = 64, 4, 8, 300
ONE, A, B = 7, 3, 9


def _make_kg():
    xs = [(ONE, o, 1) for o in range(30, 50)]
    xs += [(s, o, 2) for o in range(10) for s in (A, B)]
    xs += [(A, o, 2) for o in range(10, 20)] + [(B, o, 2) for o in range(20, 30)]
    rs = np.random.RandomState(5)
    seen = set()
    while len(xs) < T:
        t = (int(rs.randint(N)), int(rs.randint(N)), 0)
        if t not in seen:
            seen.add(t)
            xs.append(t)
    return xs


XS = _make_kg()
KNOWN = set(XS)


def _pools_numpy(xs, n_rel):
    off, ent = [0], []
    for p in range(n_rel):
        for side in (0, 1):
            ent += sorted(set(x[side] for x in xs if x[2] == p))
            off.append(len(ent))
    return np.asarray(off, dtype=np.int64), np.asarray(ent, dtype=np.int64)


OFF, ENT = _pools_numpy(XS, M)


def _pool(p, side):
    return set(ENT[OFF[2 * p + side]:OFF[2 * p + side + 1]].tolist())


@pytest.fixture(scope="module")
def kg():
    from skge_amd.device import DeviceKG
    return DeviceKG(XS, torch.device("cuda", 0))


def _perm(kg, seed, key):
    from skge_amd import _lib as L
    ek = torch.tensor([key], dtype=torch.int64, device=kg.trip.device)
    out = torch.empty(kg.T, dtype=torch.int64, device=kg.trip.device)
    L.check(L.lib().skge_epoch_permutation(L.stream_ptr(), kg.T, seed, L.ptr(ek), L.ptr(out), kg.T))
    return out.cpu().numpy()


def _records(kg, kind, seed, key, ntries):
    from skge_amd.device import epoch_records
    rec, n1 = epoch_records(kg, N, seed, key, ntries, sampler=kind, n_rel=M)
    torch.cuda.synchronize()
    return rec.cpu().numpy().astype(np.int64), n1.cpu().numpy().astype(np.int64)


def test_kg_is_the_one_described():
    assert len(XS) == len(KNOWN) == T
    assert len(_pool(0, 0)) >= 20 and len(_pool(0, 1)) >= 20
    assert _pool(1, 0) == {ONE} and _pool(2, 0) == {A, B}
    assert OFF[6] == OFF[7] == OFF[8] == len(ENT)


def test_device_type_index_is_the_csr_of_the_triples(kg):
    off, ent = kg.pools(M)
    assert off.dtype == torch.int64 and ent.dtype == torch.int32
    assert np.array_equal(off.cpu().numpy(), OFF) and np.array_equal(ent.cpu().numpy(), ENT)
    assert kg.pools(M)[0] is off            # built once
    with pytest.raises(ValueError, match="relation ids"):
        kg.pools(2)                         # relation 2 occurs: ids must be below M


# ---- 1. RANDOM through the _ex entry is today's draw ----

@pytest.mark.parametrize("key", [0, 5])
def test_random_kind_is_bitwise_the_plain_entry(kg, key):
    from skge_amd import _lib as L
    lib, dev = L.lib(), kg.trip.device
    ek = torch.tensor([key], dtype=torch.int64, device=dev)

    def run(fn, *smp):
        rec = torch.full((kg.T, 4), -7, dtype=torch.int32, device=dev)
        n1 = torch.full((kg.T,), -7, dtype=torch.int32, device=dev)
        L.check(getattr(lib, fn)(L.stream_ptr(), L.ptr(kg.trip), kg.T, L.ptr(kg.slots),
                                 kg.capacity, N, 77, L.ptr(ek), 100, L.ptr(rec), L.ptr(n1), *smp),
                fn)
        torch.cuda.synchronize()
        return rec.cpu().numpy(), n1.cpu().numpy()

    want = run("skge_epoch_sample")
    for smp in (None, L.SkgeSampler(L.SKGE_SAMPLER_RANDOM, 0, None, None)):
        got = run("skge_epoch_sample_ex", smp)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (want[0] != -7).all() and (want[1] != -7).all()
    # and it is the draw the replay defines
    rec, n1 = R.replay_records(R.RANDOM, XS, _perm(kg, 77, key), 77, key, None, 100, N)
    assert np.array_equal(want[0], rec) and np.array_equal(want[1], n1)


# ---- 2. / 3. the typed and LCWA records ----

def _check_common(rec, n1, perm, kind):
    assert np.array_equal(rec[:, :3], np.asarray(XS)[perm])
    for (s, o, p, a), b in zip(rec.tolist(), n1.tolist()):
        assert a < 0 or ((a, o, p) not in KNOWN and a in _pool(p, 0))
        assert b < 0 or (s, b, p) not in KNOWN
        if kind == R.TYPED:
            assert b < 0 or b in _pool(p, 1)
        if p == 1:
            assert a == -1                       # the only subject is s itself
        if p == 2 and o < 10:
            assert a == -1                       # known with both subjects
        if p == 2 and o >= 10:
            assert a in (-1, A + B - s)          # the other subject, if a try found it


@pytest.mark.parametrize("ntries", [1, 100])
@pytest.mark.parametrize("key", [0, 5])
def test_typed_records_equal_host_replay(kg, ntries, key):
    perm = _perm(kg, 21, key)
    rec, n1 = _records(kg, R.TYPED, 21, key, ntries)
    want, want1 = R.replay_records(R.TYPED, XS, perm, 21, key, (OFF, ENT), ntries, N)
    assert np.array_equal(rec, want) and np.array_equal(n1, want1)
    _check_common(rec, n1, perm, R.TYPED)
    if ntries == 100:   # pools of two: a miss has probability 2^-100
        two = (rec[:, 2] == 2) & (rec[:, 1] >= 10)
        assert two.sum() == 20 and np.array_equal(rec[two, 3], A + B - rec[two, 0])
        assert (rec[rec[:, 2] == 0, 3] >= 0).all() and (n1[rec[:, 2] == 0] >= 0).all()
    else:
        assert (rec[:, 3] < 0).sum() > (rec[:, 2] != 0).sum() - 20   # one try: some rejected


@pytest.mark.parametrize("ntries", [1, 100])
@pytest.mark.parametrize("key", [0, 5])
def test_lcwa_records_equal_host_replay(kg, ntries, key):
    perm = _perm(kg, 21, key)
    rec, n1 = _records(kg, R.LCWA, 21, key, ntries)
    want, want1 = R.replay_records(R.LCWA, XS, perm, 21, key, (OFF, ENT), ntries, N)
    assert np.array_equal(rec, want) and np.array_equal(n1, want1)
    _check_common(rec, n1, perm, R.LCWA)
    rnd = _records(kg, R.RANDOM, 21, key, ntries)
    assert np.array_equal(rec[:, :3], rnd[0][:, :3]) and np.array_equal(n1, rnd[1])
    if ntries == 100:
        assert (rec[rec[:, 2] == 0, 3] >= 0).all()    # broad pools: found


def test_lcwa_finds_the_other_subject_given_enough_tries(kg):
    """A try hits the one acceptable entity of 64 with probability 1/64: at
    2000 tries a miss has probability (63/64)^2000 < 1e-13 per positive."""
    rec, _ = _records(kg, R.LCWA, 21, 0, 2000)
    two = (rec[:, 2] == 2) & (rec[:, 1] >= 10)
    assert two.sum() == 20 and np.array_equal(rec[two, 3], A + B - rec[two, 0])
    assert (rec[(rec[:, 2] == 1) | ((rec[:, 2] == 2) & (rec[:, 1] < 10)), 3] == -1).all()


# ---- 4. argument errors ----

def test_sampler_argument_errors_do_not_launch(kg):
    from skge_amd import _lib as L
    lib, dev = L.lib(), kg.trip.device
    off, ent = kg.pools(M)
    ek = torch.zeros(1, dtype=torch.int64, device=dev)
    rec = torch.full((kg.T, 4), -7, dtype=torch.int32, device=dev)
    n1 = torch.full((kg.T,), -7, dtype=torch.int32, device=dev)
    bad = [(L.SkgeSampler(7, M, off.data_ptr(), ent.data_ptr()), b"kind"),
           (L.SkgeSampler(L.SKGE_SAMPLER_TYPED, M, None, None), b"NULL"),
           (L.SkgeSampler(L.SKGE_SAMPLER_TYPED, M, off.data_ptr(), None), b"NULL"),
           (L.SkgeSampler(L.SKGE_SAMPLER_LCWA, M, None, ent.data_ptr()), b"NULL"),
           (L.SkgeSampler(L.SKGE_SAMPLER_LCWA, 0, off.data_ptr(), ent.data_ptr()), b"n_rel"),
           (L.SkgeSampler(L.SKGE_SAMPLER_TYPED, -3, off.data_ptr(), ent.data_ptr()), b"n_rel")]
    for smp, what in bad:
        rc = lib.skge_epoch_sample_ex(L.stream_ptr(), L.ptr(kg.trip), kg.T, L.ptr(kg.slots),
                                      kg.capacity, N, 1, L.ptr(ek), 100, L.ptr(rec), L.ptr(n1), smp)
        assert rc == -1 and what in lib.skge_last_error(), (rc, lib.skge_last_error())
    torch.cuda.synchronize()
    assert (rec == -7).all().item() and (n1 == -7).all().item()
    # the runners' constructors refuse the same
    import skge_amd as S
    m = TP.make_model("transe_l1", (N, N, M), D)
    m.add_hyperparam("margin", 1.0)
    upd = {pid: S.SGD(p, 0.1) for pid, p in m.params.items()}
    te, tr = m._tables("pairwise", upd, slots=m._pair_slots(2 * kg.T))
    nv = torch.zeros(1, dtype=torch.int32, device=dev)
    h = lib.skge_pair_runner_create_ex(L.stream_ptr(), m._kernel_model(), m._af_code(), te, tr, D,
                                       L.ptr(kg.trip), kg.T, L.ptr(kg.slots), kg.capacity, 1, 1,
                                       L.ptr(ek), 1.0, 100, L.ptr(nv), bad[0][0])
    assert not h and b"kind" in lib.skge_last_error()


def test_runner_keeps_the_updaters_state_alive(kg):
    """The captured graph names the AdaGrad state's addresses: a runner built
    directly (the sampler= argument invites it) holds those tensors, so a
    caller that drops its updaters frees nothing the graph writes."""
    import gc
    import skge_amd as S
    from skge_amd.device import LogisticLoopRunner, PairLoopRunner
    for cls, kind in ((PairLoopRunner, "transe_l1"), (LogisticLoopRunner, "hole")):
        m = TP.make_model(kind, (N, N, M), D)
        m.add_hyperparam("margin", 0.5)
        upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
        ptrs = sorted(u.p2.data_ptr() for u in upd.values())
        r = cls(m, upd, kg, 3, seed=1, sampler=R.TYPED)
        del upd
        gc.collect()
        assert sorted(st.data_ptr() for _, st in r._state_held) == ptrs
        r.run(1)
        r.synchronize()
        assert all(bool(torch.isfinite(st).all()) and float(st.sum()) > 0 for _, st in r._state_held)


# ---- 5. pairwise training ----

def _sampler(S, which, xs):
    if which == "typed":
        return S.CorruptedSampler(1, xs, S.type_index(xs)), R.TYPED
    return S.LCWASampler(1, [0, 1], xs, (N, N, M)), R.LCWA


@pytest.mark.parametrize("which", ["typed", "lcwa"])
@pytest.mark.parametrize("kind", ["transe_l1", "hole", "rescal"])
def test_pairwise_trainer_device_loop_equals_replay(kind, which, monkeypatch, recwarn):
    import skge_amd as S
    import skge_amd.device as DV
    monkeypatch.setenv("SKGE_HOLE_DIRECT", "1")   # as test_gpu_pairloop: the replay's arithmetic
    xs = XS[:299]
    seed, margin, nb, epochs = 13, 0.5, 3, 2
    assert DV.batch_sizes(len(xs), nb) == [99, 99, 99, 2]
    a = TP.make_model(kind, (N, N, M), D)
    b = TP.make_model(kind, (N, N, M), D)
    b.add_hyperparam("margin", margin)
    smp, code = _sampler(S, which, xs)
    seen = []
    tr = S.PairwiseStochasticTrainer(a, nbatches=nb, max_epochs=epochs, learning_rate=0.1,
                                     margin=margin, device_loop=True, seed=seed,
                                     samplef=smp.sample, file_grad=None, file_embed=None,
                                     post_epoch=[lambda t: seen.append(t.nviolations) or True])
    tr.fit(xs, [1] * len(xs))
    assert not [w for w in recwarn.list if "device_loop" in str(w.message)]
    assert isinstance(tr._runner, DV.PairLoopRunner) and tr._runner.sampler == code
    # the same records through the per-batch step of a twin model
    kg = DV.DeviceKG(xs, b.device)
    monkeypatch.setattr(DV, "epoch_records",
                        functools.partial(DV.epoch_records, sampler=code, n_rel=M))
    upd_b = {pid: S.AdaGrad(p, 0.1) for pid, p in b.params.items()}
    want_nv = TP.replay(b, upd_b, kg, N, nb, epochs, seed, 100)
    torch.cuda.synchronize()
    print("%s %s: violations %r want %d" % (kind, which, seen, want_nv))
    for pid in a.params:
        err = float((a.params[pid].data - b.params[pid].data).abs().max().item())
        print("%s %s %s: max |diff| %.3g" % (kind, which, pid, err))
    assert sum(seen) == want_nv and want_nv > 0
    for pid in a.params:
        np.testing.assert_allclose(a.params[pid].data.cpu().numpy(),
                                   b.params[pid].data.cpu().numpy(), rtol=TP.RTOL, atol=TP.ATOL,
                                   err_msg="%s %s %s" % (kind, which, pid))


# ---- 6. logistic training ----

@pytest.mark.parametrize("which", ["typed", "lcwa"])
@pytest.mark.parametrize("kind", ["hole", "rescal"])
def test_logistic_trainer_device_loop_equals_oracle_replay(kind, which, recwarn):
    import skge_amd as S
    import skge_amd.device as DV
    xs = XS[:299]
    seed, nb, epochs = 5, 3, 2
    np.random.seed(42)
    m = getattr(S, TL.CLS[kind])((N, N, M), D)
    params = {pid: p.data.detach().cpu().numpy().astype(np.float64) for pid, p in m.params.items()}
    state = {k: np.zeros_like(v) for k, v in params.items()}
    smp, code = _sampler(S, which, xs)
    seen = []
    tr = S.StochasticTrainer(m, device_loop=True, max_epochs=epochs, nbatches=nb, seed=seed,
                             samplef=smp.sample,
                             post_epoch=[lambda t: seen.append((t.epoch, t.loss)) or True])
    tr.fit(xs, [1] * len(xs))
    assert not [w for w in recwarn.list if "device_loop" in str(w.message)]
    assert isinstance(tr._runner, DV.LogisticLoopRunner) and tr._runner.sampler == code
    assert [e for e, _ in seen] == [1, 2]
    kg = DV.DeviceKG(xs, m.device)
    for e in range(epochs):
        rec, n1 = DV.epoch_records(kg, N, seed, e, sampler=code, n_rel=M)
        want, _, _ = TL._oracle_epoch(kind, params, state, rec.cpu().numpy(), n1.cpu().numpy(),
                                      DV.batch_sizes(len(xs), nb), "adagrad")
        print("%s %s epoch %d: loss %.9g want %.9g" % (kind, which, e + 1, seen[e][1], want))
        np.testing.assert_allclose(seen[e][1], want, rtol=1e-5)
    for pid in m.params:   # as test_gpu_logistic_loop._epoch_vs_oracle's multi-batch bar
        what = "%s %s logistic %s" % (kind, which, pid)
        parity_util.check(m.params[pid].data, params[pid], what, lr=0.1, p2=state[pid])
        parity_util.check(tr._updaters[pid].p2, state[pid], what + " p2")


# ---- 7. routing ----

def test_explicit_fused_runner_with_typed_sampler_raises():
    import skge_amd as S
    m = TP.make_model("transe_l1", (N, N, M), D)
    smp = S.CorruptedSampler(1, XS, S.type_index(XS))
    for runner in ("epoch", "hole_pipe"):
        tr = S.PairwiseStochasticTrainer(m, nbatches=3, max_epochs=1, margin=1.0, device_loop=True,
                                         device_runner=runner, samplef=smp.sample, file_grad=None,
                                         file_embed=None)
        with pytest.raises(ValueError, match="pairs"):
            tr.fit(XS, [1] * T)


def test_auto_runner_with_new_sampler_is_the_pair_loop_for_transe_and_hole():
    import skge_amd as S
    from skge_amd.device import PairLoopRunner
    for kind in ("transe_l1", "hole"):
        m = TP.make_model(kind, (N, N, M), D)
        tr = S.PairwiseStochasticTrainer(m, nbatches=3, max_epochs=1, margin=0.5, device_loop=True,
                                         samplef=S.LCWASampler(1, [0, 1], XS, (N, N, M)).sample,
                                         file_grad=None, file_embed=None)
        tr.fit(XS, [1] * T)
        assert isinstance(tr._runner, PairLoopRunner) and tr.nviolations > 0


def test_ineligible_lcwa_sampler_warns_and_trains_per_batch():
    import skge_amd as S
    m = TP.make_model("transe_l1", (N, N, M), D)
    E0 = m.E.data.clone()
    np.random.seed(3)
    tr = S.PairwiseStochasticTrainer(m, nbatches=3, max_epochs=1, margin=1.0, device_loop=True,
                                     samplef=S.LCWASampler(1, [0, 1, 2], XS, (N, N, M)).sample,
                                     file_grad=None, file_embed=None)
    with pytest.warns(UserWarning, match=r"device_loop: LCWASampler\(n=1, modes=\[0, 1, 2\]\)"):
        tr.fit(XS, [1] * T)
    assert tr._runner is None and not tr._on_device
    assert not torch.equal(E0, m.E.data) and np.isfinite(m.E.data.cpu().numpy()).all()
