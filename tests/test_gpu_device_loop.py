"""Device batch loop (throughput path): permutation, device sampler, fused
sample+score+scatter kernel, native hipGraph epoch runner (GPU).

Parity: the negatives drawn on the device are recorded (neg_out) and the
exact pairs are replayed through the CPU oracle; parameters after the update
must agree within the fp32 tolerance of test_gpu_parity.  Full-size
(WN18-shaped) runs are checked through size-independent properties.
"""
import numpy as np
import pytest
import torch

from oracle import skge_oracle as O

pytestmark = pytest.mark.gpu


def make_kg(n_ent, n_rel, n_triples, seed=0):
    rs = np.random.RandomState(seed)
    trip = set()
    out = np.empty((n_triples, 3), dtype=np.int32)
    k = 0
    while k < n_triples:
        m = (n_triples - k) * 2
        s = rs.randint(n_ent, size=m)
        o = rs.randint(n_ent, size=m)
        p = rs.randint(n_rel, size=m)
        for a, b, c in zip(s, o, p):
            t = (int(a), int(b), int(c))
            if t not in trip:
                trip.add(t)
                out[k] = t
                k += 1
                if k == n_triples:
                    break
    return out, trip


def _setup(n_ent, n_rel, T, d, lr=0.1, margin=2.0, seed=3):
    import skge_amd as S
    from skge_amd.device import DeviceKG
    np.random.seed(seed)
    m = S.TransE((n_ent, n_ent, n_rel), d)
    m.add_hyperparam("margin", margin)
    upd = {pid: S.AdaGrad(p, lr) for pid, p in m.params.items()}
    trip, tset = make_kg(n_ent, n_rel, T)
    kg = DeviceKG(trip, m.device)
    return S, m, upd, trip, tset, kg


def test_epoch_permutation_is_a_bijection():
    from skge_amd import _lib as L
    for T in (1, 7, 1000, 141442):
        key = torch.tensor([5], dtype=torch.int64, device="cuda")
        out = torch.empty(T, dtype=torch.int64, device="cuda")
        L.check(L.lib().skge_epoch_permutation(L.stream_ptr(), T, 123, L.ptr(key), L.ptr(out), T))
        p = out.cpu().numpy()
        assert np.array_equal(np.sort(p), np.arange(T))
        if T > 100:
            assert not np.array_equal(p, np.arange(T))


@pytest.mark.parametrize("packed,dense_r,reps", [(False, False, 1), (True, True, 1),
                                                 (False, True, 1), (True, True, 32),
                                                 (False, True, 8)])
def test_sampler_kernel_parity_with_oracle_replay(packed, dense_r, reps):
    """Device sampler + fused score/scatter + apply, in every accumulator form
    (fp32 / exact packed int16x2; relation table with slots / dense), against
    the oracle replaying the recorded pairs."""
    from skge_amd import _lib as L
    from skge_amd.param import Accumulator
    S, m, upd, trip, tset, kg = _setup(300, 5, 2000, 200)
    E0 = np.asarray(m.E, dtype=np.float64)
    R0 = np.asarray(m.R, dtype=np.float64)
    dev = m.device
    key = torch.tensor([0], dtype=torch.int64, device=dev)
    count, start = 256, 512
    negs = torch.full((count, 2), -7, dtype=torch.int32, device=dev)
    perm = torch.empty(kg.T, dtype=torch.int64, device=dev)
    nviol = torch.zeros(1, dtype=torch.int32, device=dev)
    mode = L.SKGE_ACC_I16X4 if packed else L.SKGE_ACC_F32
    accE = Accumulator(m.E.rows, m.E.width, dev, slots=4 * count, mode=mode)
    accR = Accumulator(m.R.rows, m.R.width, dev, slots=count, mode=mode, dense=dense_r,
                       replicas=reps)
    te = upd["E"].table(accE)
    tr = upd["R"].table(accR)
    lib = L.lib()
    st = L.stream_ptr()
    L.check(lib.skge_epoch_permutation(st, kg.T, 99, L.ptr(key), L.ptr(perm), kg.T))
    L.check(lib.skge_transe_sample_grad(st, 1, te, tr, m.d, L.ptr(kg.trip), kg.T, L.ptr(kg.slots),
                                        kg.capacity, start, count, 99, L.ptr(key), float(m.margin),
                                        100, L.ptr(nviol), None, L.ptr(negs)))
    arr = (L.SkgeTable * 2)(te, tr)
    L.check(lib.skge_accum_apply(st, arr, 2, L.int_array(4 * count, count)))
    negs = negs.cpu().numpy()
    pidx = perm.cpu().numpy()[start:start + count]
    pos_list, neg_list = [], []
    for j in range(count):
        s, o, p = trip[pidx[j]]
        for mode in (0, 1):
            c = negs[j, mode]
            assert c >= 0, "a WN18-sparse KG never exhausts 100 tries"
            nt = (int(c), int(o), int(p)) if mode == 0 else (int(s), int(c), int(p))
            assert nt not in tset                     # rejection against the training set
            assert nt != (s, o, p)
            pos_list.append((s, o, p))
            neg_list.append(nt)
    pos = np.array(pos_list)
    neg = np.array(neg_list)
    params = {"E": E0.copy(), "R": R0.copy()}
    state = {"E": np.zeros_like(E0), "R": np.zeros_like(R0)}
    _, _, nv, g = O.pairwise_step("transe", params, state, pos, neg, 0.1, float(m.margin),
                                  "adagrad", l1=True)
    assert int(nviol.item()) == nv
    np.testing.assert_allclose(np.asarray(m.E), params["E"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(np.asarray(m.R), params["R"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(upd["E"].p2.cpu().numpy(), state["E"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(upd["R"].p2.cpu().numpy(), state["R"], rtol=1e-5, atol=1e-5)
    for acc in (accE, accR):   # accumulators are clean again
        assert int(acc.cnt.abs().sum().item()) == 0
        assert float(acc.sum.abs().sum().item()) == 0.0


def test_sampler_mode_balance():
    """Mode 0 corrupts s, mode 1 corrupts o, drawn uniformly over entities."""
    from skge_amd import _lib as L
    S, m, upd, trip, tset, kg = _setup(64, 3, 500, 8, margin=-1e9)  # no violations: pure sampling
    dev = m.device
    key = torch.tensor([1], dtype=torch.int64, device=dev)
    negs = torch.empty((kg.T, 2), dtype=torch.int32, device=dev)
    te = upd["E"].table(m.accumulator("E").ensure_slots(4 * kg.T))
    tr = upd["R"].table(m.accumulator("R").ensure_slots(kg.T))
    L.check(L.lib().skge_transe_sample_grad(L.stream_ptr(), 1, te, tr, m.d, L.ptr(kg.trip), kg.T,
                                            L.ptr(kg.slots), kg.capacity, 0, kg.T, 7, L.ptr(key),
                                            -1e9, 100, None, None, L.ptr(negs)))
    n = negs.cpu().numpy()
    assert (n >= 0).all()
    hist = np.bincount(n.ravel(), minlength=64)
    # 1000 uniform draws over 64 entities: every entity drawn, none wildly over-represented
    assert hist.min() > 0 and hist.max() < 60


def test_runner_small_two_epochs_invariants():
    S, m, upd, trip, tset, kg = _setup(500, 7, 3000, 52)
    from skge_amd.device import EpochRunner
    tr = EpochRunner(m, upd, kg, nbatches=10, seed=1)
    assert tr.pipelined
    # 3000 = 10 x 300, no remainder batch: epoch sample + 10 batches + flush + advance
    assert tr.nlaunches == 10 + 3
    tr.run(2)
    tr.synchronize()
    E = np.asarray(m.E, dtype=np.float64)
    assert np.isfinite(E).all()
    np.testing.assert_allclose(np.linalg.norm(E, axis=1), 1.0, atol=1e-5)
    nv = int(tr.nviol_total.item())
    assert 0 < nv <= 2 * 2 * kg.T
    assert tr.packed
    for acc in (tr.accE, tr.accR):
        assert int(acc.cnt.abs().sum().item()) == 0
        assert float(acc.sum.abs().sum().item()) == 0.0
    assert int(tr.epoch_key.item()) == 2


@pytest.mark.parametrize("l1", [True, False])
def test_runner_wn18_full_size_properties(l1):
    """WN18 geometry (|E|=40943, |R|=18, T=141442, d=200, nb=100): one epoch."""
    import skge_amd as S
    from skge_amd.device import DeviceKG, EpochRunner
    np.random.seed(42)
    m = S.TransE((40943, 40943, 18), 200, l1=l1)
    m.add_hyperparam("margin", 2.0)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    trip, _ = make_kg(40943, 18, 141442)
    kg = DeviceKG(trip, m.device)
    R0 = np.asarray(m.R).copy()
    runner = EpochRunner(m, upd, kg, nbatches=100, seed=0)
    assert runner.pipelined == l1
    assert runner.nlaunches == (101 + 3 if l1 else 2 * 101 + 1)
    runner.run(1)
    runner.synchronize()
    E = np.asarray(m.E, dtype=np.float64)
    assert np.isfinite(E).all()
    np.testing.assert_allclose(np.linalg.norm(E, axis=1), 1.0, atol=1e-5)
    nv = int(runner.nviol_total.item())
    assert 0 < nv <= 2 * kg.T
    assert not np.allclose(np.asarray(m.R), R0)
    assert runner.packed == l1
    for acc in (runner.accE, runner.accR):
        assert int(acc.cnt.abs().sum().item()) == 0
        assert float(acc.sum.abs().sum().item()) == 0.0


def _runner_result(n_ent, n_rel, T, d, nb, pipelined, epochs=2, seed=11, trip=None):
    import skge_amd as S
    from skge_amd.device import DeviceKG, EpochRunner
    np.random.seed(seed)
    m = S.TransE((n_ent, n_ent, n_rel), d)
    m.add_hyperparam("margin", 2.0)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    if trip is None:
        trip, _ = make_kg(n_ent, n_rel, T)
    kg = DeviceKG(trip, m.device)
    r = EpochRunner(m, upd, kg, nbatches=nb, seed=seed, pipelined=pipelined)
    assert r.pipelined == pipelined
    r.run(epochs)
    r.synchronize()
    for acc in (r.accE, r.accR):
        assert int(acc.cnt.abs().sum().item()) == 0
        assert float(acc.sum.abs().sum().item()) == 0.0
    out = {"E": m.E.data.cpu().numpy().copy(), "R": m.R.data.cpu().numpy().copy(),
           "pE": upd["E"].p2.cpu().numpy().copy(), "pR": upd["R"].p2.cpu().numpy().copy(),
           "nviol": int(r.nviol_total.item()), "key": int(r.epoch_key.item()),
           "hot": r.hot_rows}
    del r
    return out, trip


@pytest.mark.parametrize("n_ent,n_rel,T,d,nb", [
    (500, 7, 3000, 52, 10),       # even batches
    (500, 7, 3001, 200, 7),       # ragged remainder batch (np.split geometry)
    (40, 3, 1200, 200, 4),        # tiny graph: most rows pending every batch (claim/wait stress)
    (2000, 11, 8000, 400, 20),    # two quads per lane
    (1000, 5, 4000, 1024, 8),     # widest packed row
    (40943, 18, 141442, 200, 100),  # WN18 geometry
    (20000, 11, 40000, 64, 2),    # large batch: the apply waves loop over their slots
    (40943, 18, 141442, 200, 2),  # WN18 at nb = 2: relation sums in 16 replicas (k_rel_fold)
])
def test_pipelined_runner_bitwise_equals_two_launch(n_ent, n_rel, T, d, nb, monkeypatch):
    """The pipelined runner (one launch per batch: k_pipe_batch's
    cross-workgroup hand-off, and -- forced with SKGE_PIPE_FUSED=1 wherever it
    applies, below 16k slot records and d <= 256 -- k_pipe_fused, where a
    pending row is updated by its readers themselves) must reproduce the
    two-launch loop exactly."""
    a, trip = _runner_result(n_ent, n_rel, T, d, nb, pipelined=False)
    for mode in ("hand-off", "fused"):
        monkeypatch.setenv("SKGE_PIPE_FUSED", {"hand-off": "0", "fused": "1"}[mode])
        b, _ = _runner_result(n_ent, n_rel, T, d, nb, pipelined=True, trip=trip)
        assert a["key"] == b["key"] == 2
        assert a["nviol"] == b["nviol"] > 0, mode
        for k in ("E", "R", "pE", "pR"):
            assert np.array_equal(a[k], b[k]), (k, mode)


def race_scenario(d=200, nb=10, sleep_cycles=int(2e8), unordered=False):
    """(fresh, racy) one-epoch results of the same TransE run: `fresh` from
    freshly zeroed accumulators; `racy` with the runner's accumulators placed
    (through the caching allocator) in blocks a previous user left holding
    nonzero counts, sums and slot records, their zero fill queued on the
    caller's stream behind a long torch.cuda._sleep, and run(1) called at
    once.  The runner must order its first launch after that fill (round 5's
    fix: EpochRunner syncs the caller's stream after building its tables, and
    run() waits on it).  unordered=True neutralises exactly that ordering
    (tools/race_check.py: shows the scenario catches the race)."""
    from unittest import mock
    import skge_amd as S
    from skge_amd import param as P
    from skge_amd.device import DeviceKG, EpochRunner
    n_ent, n_rel, T = 3000, 11, 12000
    trip, _ = make_kg(n_ent, n_rel, T, seed=4)

    def one(racy):
        np.random.seed(21)
        m = S.TransE((n_ent, n_ent, n_rel), d)
        m.add_hyperparam("margin", 2.0)
        upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
        kg = DeviceKG(trip, m.device)
        torch.cuda.synchronize()
        orig = P.Accumulator.__init__

        def dirty_init(self, rows, width, device, slots=1024, mode=0, dense=False, replicas=1):
            reps = replicas if dense else 1
            dw = width // 2 if mode == 1 else (2 * width if mode == 3 else
                                               (width // 4 if mode == 4 else width))
            # blocks of exactly the sizes about to be allocated, left dirty
            # (counts 3, packed sums 0x00010001 per word, slot records = row 1)
            junk = [torch.full((reps * rows * dw,), 65537, dtype=torch.int32, device=device),
                    torch.full((reps * rows,), 3, dtype=torch.int32, device=device)]
            if not dense:
                junk.append(torch.full((max(slots, 1),), 1, dtype=torch.int32, device=device))
            del junk
            torch.cuda._sleep(sleep_cycles)   # the zero fill below waits behind this
            orig(self, rows, width, device, slots=slots, mode=mode, dense=dense,
                 replicas=replicas)

        patches = [mock.patch.object(P.Accumulator, "__init__", dirty_init)] if racy else []
        if racy and unordered:
            patches += [mock.patch.object(torch.cuda.Stream, "synchronize", lambda self: None),
                        mock.patch.object(torch.cuda.Stream, "wait_stream", lambda self, o: None)]
        for p_ in patches:
            p_.start()
        try:
            r = EpochRunner(m, upd, kg, nbatches=nb, seed=9)
            assert r.pipelined
            r.run(1)
        finally:
            for p_ in reversed(patches):
                p_.stop()
        torch.cuda.synchronize()
        err = L_error(r)
        out = {"E": m.E.data.cpu().numpy().copy(), "R": m.R.data.cpu().numpy().copy(),
               "pE": upd["E"].p2.cpu().numpy().copy(), "nviol": int(r.nviol_total.item()),
               "err": err}
        del r
        torch.cuda.synchronize()
        return out
    return one(False), one(True)


def L_error(r):
    from skge_amd import _lib as L
    return int(L.lib().skge_pipe_runner_error(r.handle, L.stream_ptr(r.stream)))


@pytest.mark.parametrize("d", [200, 64])   # the hand-off kernel; the fused kernel (d <= 64)
def test_runner_first_launch_ordered_after_zero_fill(d):
    """Regression test for round 5's stream-ordering race (a reused
    allocation reached the runner's first launch before its zero fill; seen
    once as a spurious 'count exceeded 32767'): dirty reused blocks, the fill
    delayed behind a long kernel on the caller's stream, run(1) at once --
    the result must equal the run from fresh tables bit for bit."""
    fresh, racy = race_scenario(d=d)
    assert fresh["err"] == 0 and racy["err"] == 0
    assert fresh["nviol"] == racy["nviol"] > 0
    for k in ("E", "R", "pE"):
        assert np.array_equal(fresh[k], racy[k]), k


def test_pipelined_error_stops_updates_and_refuses_runs():
    """A packed sum that wraps (ERR_PACKED: a row's per-batch count past
    32767, forced here with packed=True on a star KG whose hub is the subject
    of every triple) must not go on corrupting the tables: epochs queued after
    the failing one change nothing (run(3) leaves the tables as run(1) does),
    synchronize() raises, and the runner refuses every later run()."""
    import skge_amd as S
    from skge_amd import _lib as L
    from skge_amd.device import DeviceKG, EpochRunner
    n_ent, n_rel, T = 3000, 11, 24000
    rs = np.random.RandomState(2)
    pairs = set()
    while len(pairs) < T:
        pairs.add((int(rs.randint(1, n_ent)), int(rs.randint(n_rel))))
    trip = np.array([(0, o, p) for o, p in sorted(pairs)], dtype=np.int32)
    res = []
    for epochs in (1, 3):
        np.random.seed(8)
        m = S.TransE((n_ent, n_ent, n_rel), 64)
        m.add_hyperparam("margin", 2.0)
        upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
        kg = DeviceKG(trip, m.device)
        r = EpochRunner(m, upd, kg, nbatches=2, seed=1, pipelined=True, packed=True)
        r.run(epochs)
        with pytest.raises(L.SkgeError, match="32767"):
            r.synchronize()
        with pytest.raises(L.SkgeError, match="refuses"):
            r.run(1)
        res.append((m.E.data.cpu().numpy().copy(), m.R.data.cpu().numpy().copy(),
                    upd["E"].p2.cpu().numpy().copy()))
        del r
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)


def test_trainer_device_loop_fit():
    import skge_amd as S
    np.random.seed(42)
    m = S.TransE((400, 400, 6), 32)
    trip, _ = make_kg(400, 6, 3000)
    seen = []
    xs = [tuple(x) for x in trip.tolist()]
    tr = S.PairwiseStochasticTrainer(m, nbatches=10, max_epochs=3, learning_rate=0.1, margin=2.0,
                                     device_loop=True, file_grad=None, file_embed=None,
                                     samplef=S.RandomModeSampler(1, [0, 1], xs, (400, 400, 6)).sample,
                                     post_epoch=[lambda t: seen.append((t.epoch, t.nviolations))
                                                 or True])
    tr.fit(xs, [1] * len(trip))
    assert tr._on_device
    assert [e for e, _ in seen] == [1, 2, 3]
    assert all(v > 0 for _, v in seen)


def test_pipelined_large_batch_matches_fp32_runner():
    """Batches past the static packed bound (4 * 10000 > 32767): the pipelined
    runner's exact packed sums, checked per row at run time, against the
    two-launch runner's fp32 sums of the same integer contributions (exact in
    fp32 too).  Same negatives; only the projections' summation order differs
    (quad vs lane-strided layout), so the parameters agree to fp32 rounding."""
    import skge_amd as S
    from skge_amd.device import DeviceKG, EpochRunner
    trip, _ = make_kg(3000, 11, 20000)
    out = []
    for pipelined in (True, False):
        np.random.seed(7)
        m = S.TransE((3000, 3000, 11), 64)
        m.add_hyperparam("margin", 2.0)
        upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
        kg = DeviceKG(trip, m.device)
        r = EpochRunner(m, upd, kg, nbatches=2, seed=3, pipelined=pipelined,
                        force_f32=not pipelined)
        assert r.pipelined == pipelined and r.packed == pipelined
        r.run(1)
        r.synchronize()   # raises on a packed-sum overflow
        out.append((m.E.data.cpu().numpy().copy(), m.R.data.cpu().numpy().copy(),
                    int(r.nviol_total.item())))
        del r
    (E1, R1, v1), (E2, R2, v2) = out
    assert v1 > 0
    assert abs(v1 - v2) <= 2   # a margin test may flip on a rounding-level score difference
    np.testing.assert_allclose(E1, E2, atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(R1, R2, atol=1e-5, rtol=1e-5)


def test_pipelined_wn18_two_batches_per_epoch():
    """WN18 geometry at nb=2 (70721 positives per batch) on the pipelined runner."""
    import skge_amd as S
    from skge_amd.device import DeviceKG, EpochRunner
    np.random.seed(42)
    m = S.TransE((40943, 40943, 18), 200)
    m.add_hyperparam("margin", 2.0)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    trip, _ = make_kg(40943, 18, 141442)
    kg = DeviceKG(trip, m.device)
    runner = EpochRunner(m, upd, kg, nbatches=2, seed=0)
    assert runner.pipelined and runner.packed
    runner.run(2)
    runner.synchronize()
    E = np.asarray(m.E, dtype=np.float64)
    assert np.isfinite(E).all()
    np.testing.assert_allclose(np.linalg.norm(E, axis=1), 1.0, atol=1e-5)
    assert 0 < int(runner.nviol_total.item()) <= 2 * 2 * kg.T
    for acc in (runner.accE, runner.accR):
        assert int(acc.cnt.abs().sum().item()) == 0
        assert float(acc.sum.abs().sum().item()) == 0.0


def _padded_pair_runs(n_ent, n_rel, T, d, nb, epochs=2, seed=13):
    """The same KG and draws on (a) a d-wide TransE-L1 model (d % 4 != 0: the
    pipelined runner on zero-padded copies) and (b) a model four-aligned wide
    whose extra columns are zero."""
    import torch
    import skge_amd as S
    from skge_amd.device import DeviceKG, EpochRunner
    trip, _ = make_kg(n_ent, n_rel, T)
    dp = (d + 3) // 4 * 4
    out = []
    for width in (d, dp):
        np.random.seed(seed)
        m = S.TransE((n_ent, n_ent, n_rel), d)
        E0, R0 = m.E.data.clone(), m.R.data.clone()
        if width != d:
            m = S.TransE((n_ent, n_ent, n_rel), width)
            m.E.data.zero_()
            m.R.data.zero_()
            m.E.data[:, :d].copy_(E0)
            m.R.data[:, :d].copy_(R0)
        m.add_hyperparam("margin", 2.0)
        upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
        kg = DeviceKG(trip, m.device)
        r = EpochRunner(m, upd, kg, nbatches=nb, seed=seed)
        assert r.pipelined and r.packed
        assert r._pad == (width % 4 != 0)
        r.run(epochs)
        r.synchronize()
        torch.cuda.synchronize()
        out.append({"E": m.E.data[:, :d].cpu().numpy().copy(),
                    "R": m.R.data[:, :d].cpu().numpy().copy(),
                    "pE": upd["E"].p2[:, :d].cpu().numpy().copy(),
                    "pR": upd["R"].p2[:, :d].cpu().numpy().copy(),
                    "Ez": m.E.data[:, d:].abs().sum().item(),
                    "nviol": int(r.nviol_total.item())})
        del r
    return out


@pytest.mark.parametrize("n_ent,n_rel,T,d,nb", [
    (40943, 18, 141442, 50, 100),   # BASELINE configs[0]'s width at WN18 shape
    (500, 7, 3001, 30, 7),          # ragged batches, d % 4 == 2
    (300, 5, 2000, 13, 4),          # odd width
])
def test_pipelined_padded_width_equals_aligned_model(n_ent, n_rel, T, d, nb):
    """d % 4 != 0 runs the pipelined runner on zero-padded tables: bit for bit
    the run of a model four-aligned wide whose extra columns are zero (they
    stay zero: sign(0) contributions, AdaGrad and the projection keep 0).
    With the aligned runner's own oracle replays (test_gpu_runner_oracle) this
    pins the padded path to the reference; a whole-epoch comparison with the
    two-launch fp32 runner is not a usable check: measured (round 4,
    tools/diag_pad_runners.py, round 3's dense 2000-entity geometry, AdaGrad,
    10 batches) the padded runner equals this aligned twin and the packed
    two-launch runner bit for bit, while the packed and the fp32 two-launch
    runners (fast rcp/sqrt vs correctly rounded AdaGrad step) stay within
    1.5e-7 for 7 batches, then a few residual components (1-4 of ~36k per
    batch) change sign between them and the sign sub-gradients move those rows
    by up to 0.016, 0.027, 0.068 -- rounding amplified by the L1 sub-gradient,
    not an error of either path."""
    a, b = _padded_pair_runs(n_ent, n_rel, T, d, nb)
    assert a["nviol"] == b["nviol"] > 0
    assert b["Ez"] == 0.0
    for k in ("E", "R", "pE", "pR"):
        assert np.array_equal(a[k], b[k]), k



# ---- the runners' shared core (csrc/skge_graph_runner.h): ownership, geometry ----

CORE_KG = dict(n_ent=11, n_rel=3, T=37, d=8)
CORE_RUNNERS = ["epoch", "hole_pipe", "pairs", "logistic"]


def _core_make(which, nb, seed=5, **kw):
    """A fresh model (fixed initial parameters), its updaters and a factory of
    the runner class `which`."""
    import skge_amd as S
    from skge_amd import device as D
    c = CORE_KG
    np.random.seed(31)
    cls = S.TransE if which in ("epoch", "pairs") else S.HolE
    m = cls((c["n_ent"], c["n_ent"], c["n_rel"]), c["d"])
    if which != "logistic":
        m.add_hyperparam("margin", 2.0)
    # SGD for the float-atomic runner: its tolerance below is argued for linear steps
    U = S.SGD if which == "hole_pipe" else S.AdaGrad
    upd = {pid: U(p, 0.1) for pid, p in m.params.items()}
    kg = D.DeviceKG(make_kg(c["n_ent"], c["n_rel"], c["T"], seed=4)[0], m.device)
    rcls = {"epoch": D.EpochRunner, "hole_pipe": D.HolePipeRunner, "pairs": D.PairLoopRunner,
            "logistic": D.LogisticLoopRunner}[which]
    return m, upd, lambda: rcls(m, upd, kg, nb, seed=seed, **kw)


def _core_train(m, upd, r):
    r.run(2)
    r.synchronize()
    out = {pid: p.data.cpu().numpy().copy() for pid, p in m.params.items()}
    for pid, u in upd.items():
        if u.state() is not None:
            out[pid + "_state"] = u.state().cpu().numpy().copy()
    return out


@pytest.mark.parametrize("which", CORE_RUNNERS)
def test_runner_made_after_twenty_destroyed_trains_like_the_first(which):
    """Create and destroy a runner 20 times, then one more: it trains a fresh
    model to what a runner made first trains it to (a buffer dropped from the
    core's ownership list, or freed twice, would show here).  Bitwise for the
    TransE-L1 runners (integer sign sums) and for the logistic loop under
    set_deterministic (fixed-point sums).  HolePipeRunner adds fp32 atomics in
    any order: a row's per-batch sum has <= 4 * 7 = 28 terms, so two orders
    differ by <= 28 * 2^-24 = 1.7e-6 of the terms' magnitude (O(1)); an SGD
    step (lr 0.1) carries 1.7e-7 of that, 12 steps (2 epochs x 6 batches)
    with the feedback through the O(1)-Lipschitz gradient (e^1.2 = 3.3) stay
    below 12 * 1.7e-7 * 3.3 = 6.7e-6; bound 1e-5."""
    import skge_amd as S
    prev = S.deterministic()
    S.set_deterministic(which == "logistic")
    try:
        m, upd, make = _core_make(which, 5)
        want = _core_train(m, upd, make())
        m, upd, make = _core_make(which, 5)
        for _ in range(20):
            r = make()
            del r
        got = _core_train(m, upd, make())
    finally:
        S.set_deterministic(prev)
    for k in want:
        if which == "hole_pipe":
            assert float(np.max(np.abs(got[k] - want[k]))) <= 1e-5, k
        else:
            assert np.array_equal(got[k], want[k]), k


# nlaunches at T = 37, nbatches = 5 (bs = 7: five batches of 7 and a remainder
# of 2), as the runners reported before they shared epoch_batches: the
# two-launch runner ("epoch2") counts 2 launches per batch + the epoch end, the
# pipelined ones a launch per batch + the flush + the draw + the end, the pair
# and logistic loops their graph's nodes
CORE_NLAUNCHES = {"epoch": 9, "epoch2": 13, "hole_pipe": 9, "pairs": 15, "logistic": 14}


def test_remainder_batch_geometry_is_the_runners():
    from skge_amd import device as D
    c = CORE_KG
    sizes = D.batch_sizes(c["T"], 5)
    assert sizes == [7, 7, 7, 7, 7, 2]
    got = {}
    for which in CORE_RUNNERS:
        got[which] = _core_make(which, 5)[2]().nlaunches
    two = _core_make("epoch", 5, pipelined=False)[2]()
    assert not two.pipelined
    got["epoch2"] = two.nlaunches
    print("nlaunches", got)
    assert got == CORE_NLAUNCHES
    assert len(sizes) == (got["epoch2"] - 1) // 2 == got["epoch"] - 3 == got["hole_pipe"] - 3
