"""Device epochs with n negatives per positive over any modes, relation
corruption included (GPU): skge_epoch_sample_multi, the _multi pair and
logistic runners and the trainers that reach them.

The records are compared exactly with the host replay of tests/multineg_ref.py
on its KG (60 entities, 5 relations of which relation 4 never occurs, 299
triples = 3 batches of 99 and a remainder of 2, relation 0 a complete 6 x 6
block so that one try leaves slots at -1; test_multineg_ref.py checks the KG
on the CPU).  A device epoch is compared with the replayed pairs (labelled
triples) fed batch by batch to a twin model's _pairwise_step (_logistic_step)
-- the same kernels on the same input, so TransE-L1, whose contributions are
signs and whose sums are exact, must agree bit for bit, counters included, and
the float models within test_gpu_pairloop's 1e-5 -- and every one of the
twin's steps with one fp64 oracle step from the twin's state before it, at
parity_util's tolerances and sign-flip ceiling.
"""
import ctypes

import numpy as np
import pytest
import torch

import multineg_ref as MR
import parity_util
import sampler_ref as R
import test_gpu_pairloop as TP
from oracle import skge_oracle as O

pytestmark = pytest.mark.gpu

N, M, T, SEED = MR.N, MR.M, MR.T, MR.SEED
SZ = (N, N, M)
NB = 3
KIND_IDS = ["random", "typed", "lcwa"]
KINDS = [R.RANDOM, R.TYPED, R.LCWA]


@pytest.fixture(scope="module")
def kg():
    from skge_amd.device import DeviceKG
    return DeviceKG(MR.XS, torch.device("cuda", 0))


def _rel_range(kind):
    return MR.REL_RANGE if kind == R.TYPED else None


def _records(kg, kind, n, modes, ntries, key, seed=SEED):
    from skge_amd.device import epoch_records_multi
    pos, neg = epoch_records_multi(kg, N, M, seed, key, n, modes, ntries, sampler=kind,
                                   rel_range=_rel_range(kind))
    torch.cuda.synchronize()
    return pos.cpu().numpy().astype(np.int64), neg.cpu().numpy().astype(np.int64)


# ---- 1. records ----

@pytest.mark.parametrize("key", [0, 5])
def test_device_permutation_is_the_host_restatement(kg, key):
    from skge_amd import _lib as L
    ek = torch.tensor([key], dtype=torch.int64, device=kg.trip.device)
    out = torch.empty(kg.T, dtype=torch.int64, device=kg.trip.device)
    L.check(L.lib().skge_epoch_permutation(L.stream_ptr(), kg.T, SEED, L.ptr(ek), L.ptr(out), kg.T))
    assert np.array_equal(out.cpu().numpy(), MR.perm_of(key))


@pytest.mark.parametrize("key", [0, 5])
@pytest.mark.parametrize("ntries", [1, 100])
@pytest.mark.parametrize("n,modes", MR.CASES)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_records_equal_host_replay(kg, kind, n, modes, ntries, key):
    pos, neg = _records(kg, kind, n, modes, ntries, key)
    want_pos, want_neg = MR.kg_replay(kind, n, modes, ntries, key)
    assert np.array_equal(pos, want_pos)
    bad = np.argwhere(neg != want_neg)
    assert len(bad) == 0, (bad[:5].tolist(), neg[neg != want_neg][:5], want_neg[neg != want_neg][:5])
    if ntries == 1 and 2 not in modes:
        assert (neg < 0).any()              # the block: one try leaves slots empty
    if ntries == 100 and kind == R.RANDOM:
        assert (neg >= 0).all()
    for k in range(neg.shape[1]):           # a mode-2 slot holds a relation id
        if modes[k % len(modes)] == 2:
            assert neg[:, k].max() < (MR.REL_RANGE if kind == R.TYPED else M)


@pytest.mark.parametrize("key", [0, 5])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_one_negative_per_mode_is_bitwise_the_ex_entry(kg, kind, key):
    from skge_amd.device import epoch_records
    for ntries in (1, 100):
        rec, n1 = epoch_records(kg, N, SEED, key, ntries, sampler=kind, n_rel=M)
        pos, neg = _records(kg, kind, 1, [0, 1], ntries, key)
        rec, n1 = rec.cpu().numpy(), n1.cpu().numpy()
        assert np.array_equal(pos, rec[:, :3])
        assert np.array_equal(neg[:, 0], rec[:, 3]) and np.array_equal(neg[:, 1], n1)


# ---- 2. argument errors ----

def _negs(n, modes, rel_range=M):
    from skge_amd import _lib as L
    return L.SkgeNegatives(n, len(modes), (ctypes.c_int * 8)(*modes), rel_range)


BAD_NEGATIVES = [((0, [0, 1]), b"n = 0"), ((-2, [0]), b"n = -2"), ((1, []), b"nmodes"),
                 ((1, [0, 3]), b"mode 3"), ((1, [-1]), b"mode -1"), ((33, [0, 1]), b"at most 64"),
                 ((9, [0] * 8), b"at most 64"), ((1, [2], 0), b"rel_range"),
                 ((1, [0, 2], M + 1), b"rel_range")]


def test_negatives_argument_errors_do_not_launch(kg):
    from skge_amd import _lib as L
    lib, dev = L.lib(), kg.trip.device
    ek = torch.zeros(1, dtype=torch.int64, device=dev)
    pos = torch.full((kg.T, 3), -7, dtype=torch.int32, device=dev)
    neg = torch.full((kg.T, 64), -7, dtype=torch.int32, device=dev)

    def call(negs, smp=None):
        return lib.skge_epoch_sample_multi(L.stream_ptr(), L.ptr(kg.trip), kg.T, L.ptr(kg.slots),
                                           kg.capacity, N, M, 1, L.ptr(ek), 100, L.ptr(pos),
                                           L.ptr(neg), smp, negs)
    for args, what in BAD_NEGATIVES:
        negs = _negs(*args)
        if args[1] == []:
            negs.nmodes = 0
        rc = call(negs)
        assert rc == -1 and what in lib.skge_last_error(), (args, lib.skge_last_error())
    nine = _negs(1, [0] * 8)
    nine.nmodes = 9
    assert call(nine) == -1 and b"nmodes" in lib.skge_last_error()
    assert call(None) == -1 and b"NULL" in lib.skge_last_error()
    off, ent = kg.pools(M)
    other = L.SkgeSampler(L.SKGE_SAMPLER_LCWA, M + 1, off.data_ptr(), ent.data_ptr())
    assert call(_negs(1, [2]), other) == -1 and b"n_rel" in lib.skge_last_error()
    torch.cuda.synchronize()
    assert (pos == -7).all().item() and (neg == -7).all().item()
    assert call(_negs(1, [0, 1])) == 0      # and the same call with good arguments draws
    torch.cuda.synchronize()
    flat = neg.view(-1)                     # neg [T][2] fills the buffer's first 2 T ints
    assert (pos != -7).all().item() and (flat[:2 * kg.T] != -7).all().item()
    assert (flat[2 * kg.T:] == -7).all().item()


@pytest.mark.parametrize("loop", ["pairs", "triples"])
def test_runner_create_refuses_bad_negatives_and_small_tables(kg, loop):
    import skge_amd as S
    from skge_amd import _lib as L
    lib, dev = L.lib(), kg.trip.device
    kind = "transe_l1" if loop == "pairs" else "hole"
    m = TP.make_model(kind, SZ, 8)
    m.add_hyperparam("margin", 1.0)
    upd = {pid: S.SGD(p, 0.1) for pid, p in m.params.items()}
    ek = torch.zeros(1, dtype=torch.int64, device=dev)
    tot = torch.zeros(1, dtype=torch.int32 if loop == "pairs" else torch.float32, device=dev)
    st = torch.cuda.Stream(device=dev)
    K, B = 6, 99

    def create(te, tr, negs):
        if loop == "pairs":
            return lib.skge_pair_runner_create_multi(
                L.stream_ptr(st), m._kernel_model(), m._af_code(), te, tr, 8, L.ptr(kg.trip), kg.T,
                L.ptr(kg.slots), kg.capacity, NB, 1, L.ptr(ek), 1.0, 100, L.ptr(tot), None, negs)
        return lib.skge_triple_runner_create_multi(
            L.stream_ptr(st), m._kernel_model(), te, tr, 8, L.ptr(kg.trip), kg.T, L.ptr(kg.slots),
            kg.capacity, NB, 1, L.ptr(ek), 100, L.ptr(tot), None, negs)

    if loop == "pairs":
        te, tr = m._tables("pairwise", upd, slots=m._pair_slots(K * B))
        need = 4 * K * B
    else:
        te, tr = m._tables("logistic", upd, slots=m._triple_slots((1 + K) * B))
        need = 2 * (1 + K) * B
    torch.cuda.synchronize()
    for args, what in BAD_NEGATIVES:
        if args[1]:
            assert not create(te, tr, _negs(*args)) and what in lib.skge_last_error(), args
    assert te.touched_cap >= need
    te.touched_cap = need - 1               # one slot short of 4 K batch (2 (1 + K) batch)
    assert not create(te, tr, _negs(3, [0, 1]))
    assert b"touched slots" in lib.skge_last_error() and str(need).encode() in lib.skge_last_error()
    te.touched_cap = need
    h = create(te, tr, _negs(3, [0, 1]))
    assert h, lib.skge_last_error()
    (lib.skge_pair_runner_destroy if loop == "pairs" else lib.skge_triple_runner_destroy)(h)


# ---- 3. the pair loop against the replay ----

ORACLE = {"transe_l1": ("transe", {"l1": True}), "transe_l2": ("transe", {"l1": False}),
          "hole": ("hole", {"rparam": 0.05}), "rescal": ("rescal", {"rparam": 0.05})}
MARGIN = {"transe_l1": 1.0, "transe_l2": 1.0, "hole": 0.5, "rescal": 0.5}


def _snapshot(m, upd):
    params = {pid: p.data.detach().cpu().numpy().astype(np.float64) for pid, p in m.params.items()}
    state = {pid: upd[pid].p2.detach().cpu().numpy().astype(np.float64) for pid in m.params}
    return params, state


def _counters(m):
    out = {pid: np.asarray(p.updateCounts).copy() for pid, p in m.params.items()}
    if m.E.violations is not None:
        out["viol"] = np.asarray(m.E.violations).copy()
    return out


def _pair_twin_epoch(kind, b, upd, pos, neg, modes):
    """The replayed pairs through the twin's _pairwise_step, batch by batch;
    each step is also taken by the fp64 oracle from the twin's state before it."""
    from skge_amd.device import batch_sizes
    name, kw = ORACLE[kind]
    dev = b.device
    nv = torch.zeros(1, dtype=torch.int32, device=dev)
    total, start = 0, 0
    for bi, c in enumerate(batch_sizes(T, NB)):
        pp, nn = MR.batch_pairs(pos, neg, modes, start, c)
        start += c
        params, state = _snapshot(b, upd)
        before = {k: v.copy() for k, v in params.items()}
        nv.zero_()
        b._pairwise_step(torch.tensor(pp, dtype=torch.int32, device=dev),
                         torch.tensor(nn, dtype=torch.int32, device=dev), upd, nv)
        _, _, want_v, grads = O.pairwise_step(name, params, state, np.array(pp), np.array(nn), 0.1,
                                              MARGIN[kind], "adagrad", **kw)
        assert int(nv.item()) == want_v, (kind, bi)
        for pid in b.params:
            what = "multineg %s %r b%d %s" % (kind, modes, bi, pid)
            parity_util.check_step(b.params[pid].data, params[pid], before[pid],
                                   grads[pid] if grads else None, state[pid], 0.1, what,
                                   post=parity_util.POSTS[name].get(pid))
            parity_util.check(upd[pid].p2, state[pid], what + " p2")
        total += want_v
    return total


def _pair_loop_epoch(kind, d, n, modes, kg, sampler=R.RANDOM):
    import skge_amd as S
    from skge_amd.device import PairLoopRunner
    a = TP.make_model(kind, SZ, d)
    a.add_hyperparam("margin", MARGIN[kind])
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in a.params.items()}
    r = PairLoopRunner(a, upd, kg, NB, seed=SEED, sampler=sampler,
                       negatives=(n, modes, _rel_range(sampler)))
    with torch.cuda.stream(r.stream):
        r.run(1)
    r.synchronize()
    assert int(r.epoch_key.item()) == 1
    return a, upd, int(r.nviol_total.item())


FORMS = {"pos": "0", "pairs": "1"}   # SKGE_TRANSE_PAIRS: k_transe_pos_multi / explicit pairs


@pytest.mark.parametrize("n,modes", [(3, [0, 1]), (2, [0, 1, 2])])
@pytest.mark.parametrize("d", [8, 50, 200])
@pytest.mark.parametrize("kind", ["transe_l1", "transe_l2", "hole", "rescal"])
def test_pair_loop_equals_replay(kg, kind, d, n, modes, monkeypatch):
    """The default form of every model (TransE: whatever the library selects)."""
    monkeypatch.delenv("SKGE_TRANSE_PAIRS", raising=False)
    _check_against_replay(kg, kind, d, n, modes)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("n,modes", [(3, [0, 1]), (2, [0, 1, 2])])
@pytest.mark.parametrize("d", [8, 50, 200])
def test_transe_l2_both_forms_equal_oracle_replay(kg, d, n, modes, form, monkeypatch):
    """TransE-L2 through the per-positive kernel and through the explicit
    pairs, each forced through the switch: within 1e-5 of the replay."""
    monkeypatch.setenv("SKGE_TRANSE_PAIRS", FORMS[form])
    _check_against_replay(kg, "transe_l2", d, n, modes)


@pytest.mark.parametrize("n,modes", [(3, [0, 1]), (2, [0, 1, 2]), (4, [1, 0, 0]), (1, [2])])
@pytest.mark.parametrize("d", [8, 50, 200])
def test_transe_l1_forms_give_the_same_bits(kg, d, n, modes, monkeypatch):
    """k_transe_pos_multi against the explicit pairs (SKGE_TRANSE_PAIRS=1) on
    the same draws, each form forced through the switch: the same tables,
    AdaGrad state, violation total, updateCounts and E.violations."""
    outs = {}
    for form, env in FORMS.items():
        monkeypatch.setenv("SKGE_TRANSE_PAIRS", env)
        a, upd, v = _pair_loop_epoch("transe_l1", d, n, modes, kg)
        outs[form] = (v, {pid: p.data.cpu().numpy() for pid, p in a.params.items()},
                      {pid: upd[pid].p2.cpu().numpy() for pid in a.params}, _counters(a))
        for acc in a._acc.values():   # accumulators drained after every batch
            assert int(acc.cnt.abs().sum().item()) == 0
    x, y = outs["pos"], outs["pairs"]
    assert x[0] == y[0] > 0
    for pid in x[1]:
        assert np.array_equal(x[1][pid], y[1][pid]) and np.array_equal(x[2][pid], y[2][pid]), pid
    assert sorted(x[3]) == sorted(y[3])
    for k in x[3]:
        assert np.array_equal(x[3][k], y[3][k]) and x[3][k].sum() > 0, k


@pytest.mark.parametrize("kind", [R.TYPED, R.LCWA], ids=["typed", "lcwa"])
def test_transe_l1_forms_give_the_same_bits_with_skipped_slots(kg, kind, monkeypatch):
    """Three tries leave slots at -1 (the block, the pool kinds' misses)."""
    import skge_amd as S
    from skge_amd.device import PairLoopRunner
    assert (MR.kg_replay(kind, 2, [0, 1, 2], 3, 0)[1] < 0).any()
    outs = []
    for env in FORMS.values():
        monkeypatch.setenv("SKGE_TRANSE_PAIRS", env)
        a = TP.make_model("transe_l1", SZ, 50)
        a.add_hyperparam("margin", 1.0)
        upd = {pid: S.AdaGrad(p, 0.1) for pid, p in a.params.items()}
        r = PairLoopRunner(a, upd, kg, NB, seed=SEED, ntries=3, sampler=kind,
                           negatives=(2, [0, 1, 2], _rel_range(kind)))
        r.run(1)
        r.synchronize()
        outs.append((int(r.nviol_total.item()), a.E.data.cpu().numpy(), a.R.data.cpu().numpy(),
                     _counters(a)))
    assert outs[0][0] == outs[1][0] > 0
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    for k in outs[0][3]:
        assert np.array_equal(outs[0][3][k], outs[1][3][k]), k


def _check_against_replay(kg, kind, d, n, modes):
    import skge_amd as S
    a, upd_a, got_v = _pair_loop_epoch(kind, d, n, modes, kg)
    b = TP.make_model(kind, SZ, d)
    b.add_hyperparam("margin", MARGIN[kind])
    upd_b = {pid: S.AdaGrad(p, 0.1) for pid, p in b.params.items()}
    pos, neg = MR.kg_replay(R.RANDOM, n, modes, 100, 0)
    want_v = _pair_twin_epoch(kind, b, upd_b, pos, neg, modes)
    torch.cuda.synchronize()
    print("%s d=%d %r: violations %d want %d" % (kind, d, modes, got_v, want_v))
    assert got_v == want_v > 0
    ca, cb = _counters(a), _counters(b)
    for pid in a.params:
        ga, gb = a.params[pid].data.cpu().numpy(), b.params[pid].data.cpu().numpy()
        sa, sb = upd_a[pid].p2.cpu().numpy(), upd_b[pid].p2.cpu().numpy()
        print("%s %s: max |diff| %.3g, p2 %.3g" % (kind, pid, np.abs(ga - gb).max(),
                                                  np.abs(sa - sb).max()))
        if kind == "transe_l1":
            assert np.array_equal(ga, gb) and np.array_equal(sa, sb), pid
        else:
            np.testing.assert_allclose(ga, gb, rtol=TP.RTOL, atol=TP.ATOL, err_msg=pid)
            np.testing.assert_allclose(sa, sb, rtol=TP.RTOL, atol=TP.ATOL, err_msg=pid)
    if kind == "transe_l1":
        assert sorted(ca) == sorted(cb) and "viol" in ca
        for k in ca:
            assert np.array_equal(ca[k], cb[k]) and ca[k].sum() > 0, k
    for acc in a._acc.values():   # accumulators drained after every batch
        assert int(acc.cnt.abs().sum().item()) == 0


def test_pair_loop_transe_l1_repeats_its_bits(kg, monkeypatch):
    """Two runs of the per-positive form."""
    monkeypatch.setenv("SKGE_TRANSE_PAIRS", FORMS["pos"])
    outs = []
    for _ in range(2):
        a, upd, v = _pair_loop_epoch("transe_l1", 50, 3, [0, 1], kg)
        outs.append((v, a.E.data.cpu().numpy(), a.R.data.cpu().numpy(), _counters(a)["viol"]))
    assert outs[0][0] == outs[1][0]
    for x, y in zip(outs[0][1:], outs[1][1:]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kind", [R.TYPED, R.LCWA], ids=["typed", "lcwa"])
def test_pair_loop_typed_and_lcwa_relation_corruption(kg, kind):
    """(2, [0, 1, 2]) with the pool kinds, one try fewer than always finds a
    negative (skipped pairs in place): TransE-L1 equals the replay's bits."""
    import skge_amd as S
    from skge_amd.device import PairLoopRunner
    pos, neg = MR.kg_replay(kind, 2, [0, 1, 2], 3, 0)
    assert (neg < 0).any()
    a = TP.make_model("transe_l1", SZ, 8)
    a.add_hyperparam("margin", 1.0)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in a.params.items()}
    r = PairLoopRunner(a, upd, kg, NB, seed=SEED, ntries=3, sampler=kind,
                       negatives=(2, [0, 1, 2], _rel_range(kind)))
    r.run(1)
    r.synchronize()
    b = TP.make_model("transe_l1", SZ, 8)
    b.add_hyperparam("margin", 1.0)
    upd_b = {pid: S.AdaGrad(p, 0.1) for pid, p in b.params.items()}
    want_v = _pair_twin_epoch("transe_l1", b, upd_b, pos, neg, [0, 1, 2])
    assert int(r.nviol_total.item()) == want_v > 0
    for pid in a.params:
        assert torch.equal(a.params[pid].data, b.params[pid].data), pid


# ---- 4. the logistic loop against the oracle replay ----

@pytest.mark.parametrize("n,modes", [(3, [0, 1]), (2, [0, 1, 2])])
@pytest.mark.parametrize("d", [8, 50])
@pytest.mark.parametrize("kind", ["hole", "rescal"])
def test_logistic_loop_equals_oracle_replay(kg, kind, d, n, modes):
    import skge_amd as S
    from skge_amd.device import LogisticLoopRunner, batch_sizes
    np.random.seed(42)
    m = getattr(S, {"hole": "HolE", "rescal": "RESCAL"}[kind])(SZ, d, rparam=0.05)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    params, state = _snapshot(m, upd)
    r = LogisticLoopRunner(m, upd, kg, NB, seed=SEED, negatives=(n, modes, None))
    r.run(1)
    r.synchronize()
    pos, neg = MR.kg_replay(R.RANDOM, n, modes, 100, 0)
    want, start = 0.0, 0
    for c in batch_sizes(T, NB):
        trip, ys = MR.batch_triples(pos, neg, modes, start, c)
        assert len(trip) == (1 + n * len(modes)) * c
        start += c
        _, li, _ = O.logistic_step(kind, params, state, trip, ys, 0.1, "adagrad", rparam=0.05)
        want += float(li)
    got = float(r.loss_total.item())
    print("%s d=%d %r: loss %.9g want %.9g" % (kind, d, modes, got, want))
    np.testing.assert_allclose(got, want, rtol=1e-5)
    for pid in m.params:   # as test_gpu_logistic_loop._epoch_vs_oracle's multi-batch bar
        what = "multineg logistic %s %r %s" % (kind, modes, pid)
        parity_util.check(m.params[pid].data, params[pid], what, lr=0.1, p2=state[pid])
        parity_util.check(upd[pid].p2, state[pid], what + " p2")
    for acc in m._acc.values():
        assert int(acc.cnt.abs().sum().item()) == 0


# ---- 5. the trainers ----

def test_pairwise_trainer_trains_more_negatives_on_the_device(kg, recwarn):
    import skge_amd as S
    import skge_amd.device as DV
    a = TP.make_model("transe_l1", SZ, 8)
    seen = []
    tr = S.PairwiseStochasticTrainer(a, nbatches=NB, max_epochs=1, learning_rate=0.1, margin=1.0,
                                     device_loop=True, device_negatives=True, seed=SEED,
                                     samplef=S.RandomModeSampler(3, [0, 1], MR.XS, SZ).sample,
                                     file_grad=None, file_embed=None,
                                     post_epoch=[lambda t: seen.append(t.nviolations) or True])
    tr.fit(MR.XS, [1] * T)
    assert not [w for w in recwarn.list if "device_loop" in str(w.message)]
    assert isinstance(tr._runner, DV.PairLoopRunner)
    assert (tr._runner.n, tr._runner.modes, tr._runner.K) == (3, [0, 1], 6)
    b = TP.make_model("transe_l1", SZ, 8)
    b.add_hyperparam("margin", 1.0)
    upd_b = {pid: S.AdaGrad(p, 0.1) for pid, p in b.params.items()}
    pos, neg = MR.kg_replay(R.RANDOM, 3, [0, 1], 100, 0)
    want_v = _pair_twin_epoch("transe_l1", b, upd_b, pos, neg, [0, 1])
    assert seen == [want_v]
    for pid in a.params:
        assert torch.equal(a.params[pid].data, b.params[pid].data), pid


def test_logistic_trainer_trains_relation_corruption_on_the_device(kg, recwarn):
    import skge_amd as S
    import skge_amd.device as DV
    from skge_amd.device import batch_sizes
    np.random.seed(42)
    m = S.HolE(SZ, 8)
    upd0 = {pid: p.data.detach().cpu().numpy().astype(np.float64) for pid, p in m.params.items()}
    state = {k: np.zeros_like(v) for k, v in upd0.items()}
    seen = []
    tr = S.StochasticTrainer(m, device_loop=True, device_negatives=True, max_epochs=1,
                             nbatches=NB, seed=SEED,
                             samplef=S.RandomModeSampler(2, [0, 1, 2], MR.XS, SZ).sample,
                             post_epoch=[lambda t: seen.append(t.loss) or True])
    tr.fit(MR.XS, [1] * T)
    assert not [w for w in recwarn.list if "device_loop" in str(w.message)]
    assert isinstance(tr._runner, DV.LogisticLoopRunner) and tr._runner.K == 6
    pos, neg = MR.kg_replay(R.RANDOM, 2, [0, 1, 2], 100, 0)
    want, start = 0.0, 0
    for c in batch_sizes(T, NB):
        trip, ys = MR.batch_triples(pos, neg, [0, 1, 2], start, c)
        start += c
        want += float(O.logistic_step("hole", upd0, state, trip, ys, 0.1, "adagrad")[1])
    np.testing.assert_allclose(seen[0], want, rtol=1e-5)
    for pid in m.params:
        parity_util.check(m.params[pid].data, upd0[pid], "multineg trainer %s" % pid, lr=0.1,
                          p2=state[pid])


def test_one_negative_per_mode_still_picks_todays_runners():
    import skge_amd as S
    import skge_amd.device as DV
    for kind, d, want in (("transe_l1", 16, DV.EpochRunner), ("hole", 16, DV.HolePipeRunner),
                          ("rescal", 8, DV.PairLoopRunner)):
        m = TP.make_model(kind, SZ, d)
        tr = S.PairwiseStochasticTrainer(m, nbatches=NB, max_epochs=1, margin=0.5,
                                         device_loop=True, device_negatives=True,
                                         samplef=S.RandomModeSampler(1, [0, 1], MR.XS, SZ).sample,
                                         file_grad=None, file_embed=None)
        tr.fit(MR.XS, [1] * T)
        assert type(tr._runner) is want, kind
        assert getattr(tr._runner, "_neg", None) is None


def test_out_of_scope_negatives_warn_and_train_per_batch():
    import skge_amd as S
    m = TP.make_model("transe_l1", SZ, 8)
    E0 = m.E.data.clone()
    np.random.seed(3)
    xs = MR.XS[:60]
    tr = S.PairwiseStochasticTrainer(m, nbatches=NB, max_epochs=1, margin=1.0, device_loop=True,
                                     device_negatives=True,
                                     samplef=S.RandomModeSampler(33, [0, 1], xs, SZ).sample,
                                     file_grad=None, file_embed=None)
    with pytest.warns(UserWarning, match=r"device_loop: RandomModeSampler\(n=33.*66 negatives"):
        tr.fit(xs, [1] * len(xs))
    assert tr._runner is None and not tr._on_device
    assert not torch.equal(E0, m.E.data)


def test_explicit_fused_runner_with_more_negatives_raises():
    import skge_amd as S
    for kind, runner in (("transe_l1", "epoch"), ("hole", "hole_pipe")):
        m = TP.make_model(kind, SZ, 16)
        tr = S.PairwiseStochasticTrainer(m, nbatches=NB, max_epochs=1, margin=1.0,
                                         device_loop=True, device_negatives=True,
                                         device_runner=runner,
                                         samplef=S.RandomModeSampler(3, [0, 1], MR.XS, SZ).sample,
                                         file_grad=None, file_embed=None)
        with pytest.raises(ValueError, match="pairs"):
            tr.fit(MR.XS, [1] * T)


def test_without_the_switch_more_negatives_warn_and_train_per_batch():
    """device_negatives is off by default: the sampler that trains on the
    device above keeps the per-batch path and its warning."""
    import skge_amd as S
    m = TP.make_model("transe_l1", SZ, 8)
    E0 = m.E.data.clone()
    np.random.seed(3)
    xs = MR.XS[:60]
    tr = S.PairwiseStochasticTrainer(m, nbatches=NB, max_epochs=1, margin=1.0, device_loop=True,
                                     samplef=S.RandomModeSampler(3, [0, 1], xs, SZ).sample,
                                     file_grad=None, file_embed=None)
    with pytest.warns(UserWarning, match=r"RandomModeSampler\(n=3.*device_negatives=True"):
        tr.fit(xs, [1] * len(xs))
    assert tr._runner is None and not tr._on_device
    assert not torch.equal(E0, m.E.data)

