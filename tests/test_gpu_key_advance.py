"""The pipelined runners' key advance inside the flush launch.

The epoch's launches read the runner's own copy of the epoch key (filled by
k_epoch_sample at the head of every epoch from the caller's word) and the
flush launch writes key + 1 into the caller's word; there is no key-advance
launch.  None of that may change a result: the pipelined runners must still
equal the two-launch runner bit for bit over several epochs of one run(),
whatever the batch geometry, the number of run() calls, or the key a run
starts at -- the properties a sampler running ahead of its epoch would have
to keep too (the cases are those of its issue).
"""
import numpy as np
import pytest
import torch

from oracle import skge_oracle as O

pytestmark = pytest.mark.gpu

ATOL = RTOL = 1e-5   # the HolE runner tests' fp32 bar (test_gpu_pairloop.py)


def make_kg(n_ent, n_rel, T, seed=3):
    rs = np.random.RandomState(seed)
    seen, out = set(), []
    while len(out) < T:
        t = (int(rs.randint(n_ent)), int(rs.randint(n_ent)), int(rs.randint(n_rel)))
        if t not in seen:
            seen.add(t)
            out.append(t)
    return np.array(out, dtype=np.int32)


def _transe(trip, n_ent, n_rel, d, nb, pipelined, seed=11, key=0, **kw):
    import skge_amd as S
    from skge_amd.device import DeviceKG, EpochRunner
    np.random.seed(seed)
    m = S.TransE((n_ent, n_ent, n_rel), d)
    m.add_hyperparam("margin", 2.0)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    r = EpochRunner(m, upd, DeviceKG(trip, m.device), nbatches=nb, seed=seed,
                    pipelined=pipelined, **kw)
    assert r.pipelined == pipelined
    if key:
        r.epoch_key.fill_(key)
    return m, upd, r


def _state(m, upd, r):
    r.synchronize()
    return {"E": m.E.data.cpu().numpy().copy(), "R": m.R.data.cpu().numpy().copy(),
            "pE": upd["E"].p2.cpu().numpy().copy(), "pR": upd["R"].p2.cpu().numpy().copy(),
            "nviol": int(r.nviol_total.item()), "key": int(r.epoch_key.item())}


def _same(a, b, what):
    assert a["nviol"] == b["nviol"] and a["key"] == b["key"], (what, a["nviol"], b["nviol"],
                                                                 a["key"], b["key"])
    for k in ("E", "R", "pE", "pR"):
        assert np.array_equal(a[k], b[k]), (what, k)


def _train(trip, n_ent, n_rel, d, nb, pipelined, runs=(3,), key=0, seed=11):
    m, upd, r = _transe(trip, n_ent, n_rel, d, nb, pipelined, seed=seed, key=key)
    for n in runs:
        r.run(n)
    out = _state(m, upd, r)
    out["kernel"] = r.kernel
    del r
    return out


# (n_ent, n_rel, T, d, nb, kernel)
GEOMETRIES = [
    (200, 3, 130, 8, 4, None),            # batches of 32 and a remainder of 2: under one wave of lanes
    (500, 5, 1000, 200, 3, "k_pipe_batch"),   # remainder of 1
    (300, 4, 64 * 3 + 1, 200, 1, "k_pipe_batch"),   # T = 64 k + 1, one batch: the last item has one lane
    (2000, 7, 64 * 9 + 1, 8, 2, None),    # T = 64 k + 1, two batches and a remainder of 1
]


@pytest.mark.parametrize("n_ent,n_rel,T,d,nb,kernel", GEOMETRIES)
def test_pipelined_equals_two_launch_after_three_epochs(n_ent, n_rel, T, d, nb, kernel):
    """Epochs 2 and 3 run at the keys the flushes of epochs 1 and 2 wrote: E,
    R, both AdaGrad states, the violation total and the key must equal the
    two-launch runner's."""
    trip = make_kg(n_ent, n_rel, T)
    a = _train(trip, n_ent, n_rel, d, nb, pipelined=False)
    b = _train(trip, n_ent, n_rel, d, nb, pipelined=True)
    if kernel:
        assert b["kernel"] == kernel
    assert a["nviol"] > 0 and b["key"] == 3
    _same(a, b, "3 epochs")


def test_fused_padded_d50_equals_two_launch_on_aligned_twin():
    """d = 50 runs k_pipe_fused on 64-wide zero-padded tables.  The two-launch
    runner takes d = 50 only with fp32 sums, whose AdaGrad step rounds
    differently (test_pipelined_padded_width_equals_aligned_model), so the
    bitwise reference is the packed two-launch runner on a 52-wide twin whose
    extra columns are zero -- they stay zero and add nothing to a score."""
    import skge_amd as S
    from skge_amd.device import DeviceKG, EpochRunner
    n_ent, n_rel, T, d, nb, seed = 400, 4, 1500 + 3, 50, 5, 13
    trip = make_kg(n_ent, n_rel, T)
    out = []
    for width, pipelined in ((d, True), (52, False)):
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
        r = EpochRunner(m, upd, DeviceKG(trip, m.device), nbatches=nb, seed=seed,
                        pipelined=pipelined)
        assert r.pipelined == pipelined and r.packed
        if pipelined:
            assert r._pad and r.d_pad == 64 and r.kernel == "k_pipe_fused"
        r.run(3)
        r.synchronize()
        torch.cuda.synchronize()
        out.append({"E": m.E.data[:, :d].cpu().numpy().copy(),
                    "R": m.R.data[:, :d].cpu().numpy().copy(),
                    "pE": upd["E"].p2[:, :d].cpu().numpy().copy(),
                    "pR": upd["R"].p2[:, :d].cpu().numpy().copy(),
                    "nviol": int(r.nviol_total.item()), "key": int(r.epoch_key.item())})
        del r
    assert out[0]["nviol"] > 0
    _same(out[1], out[0], "d = 50")


def test_both_transe_kernels_equal_two_launch(monkeypatch):
    """The same geometry through k_pipe_batch and k_pipe_fused (forced)."""
    n_ent, n_rel, T, d, nb = 300, 4, 700, 64, 3
    trip = make_kg(n_ent, n_rel, T)
    a = _train(trip, n_ent, n_rel, d, nb, pipelined=False)
    for force, kernel in (("0", "k_pipe_batch"), ("1", "k_pipe_fused")):
        monkeypatch.setenv("SKGE_PIPE_FUSED", force)
        b = _train(trip, n_ent, n_rel, d, nb, pipelined=True)
        assert b["kernel"] == kernel
        _same(a, b, kernel)


def _hole(cls, xs, n_ent, n_rel, d, nb, runs, opt="sgd"):
    import skge_amd as S
    from skge_amd.device import DeviceKG
    np.random.seed(42)
    m = S.HolE((n_ent, n_ent, n_rel), d, rparam=0.05)
    m.add_hyperparam("margin", 0.2)
    U = S.SGD if opt == "sgd" else S.AdaGrad
    upd = {pid: U(p, 0.1) for pid, p in m.params.items()}
    r = cls(m, upd, DeviceKG(xs, m.device), nb, seed=9)
    for n in runs:
        with torch.cuda.stream(r.stream):
            r.run(n)
    r.synchronize()
    return (int(r.nviol_total.item()), int(r.epoch_key.item()),
            {pid: p.data.cpu().numpy().copy() for pid, p in m.params.items()})


@pytest.mark.parametrize("n_ent,n_rel,T,d,nb,opt", [
    (300, 7, 64 * 8 + 1, 32, 4, "sgd"),       # remainder of 1
    (500, 5, 1300, 200, 3, "sgd"),            # d = 200: the two-waves-per-positive FFT form
])
def test_hole_pipelined_matches_pair_loop_after_three_epochs(n_ent, n_rel, T, d, nb, opt):
    """HolE's pipelined runner against the pair loop (which keeps its
    stand-alone sampling), three epochs: fp32 sums add in any order, so the
    HolE runner tests' bar -- totals within a tie or two, parameters within
    1e-5 + 1e-5 |x|.

    SGD, as every d = 200 case of test_gpu_pairloop.py: an SGD step carries
    the two paths' rounding difference (FFT against direct correlations,
    atomics in any order) through unchanged -- measured 1.5e-8 here, with this
    change and without.  AdaGrad's first steps divide by the root of a tiny
    sum of squares and amplify it: at this geometry the build before this
    change and this one both measured 1.5e-6 .. 3.0e-6 in a process of their
    own and 2.2e-5 .. 2.3e-5 on 6 of 100000 elements after this file's other
    tests, so AdaGrad here would test the order of the file.  AdaGrad state
    through look-ahead epochs is pinned bit for bit by the TransE tests."""
    from skge_amd.device import HolePipeRunner, PairLoopRunner
    xs = [tuple(int(v) for v in t) for t in make_kg(n_ent, n_rel, T)]
    a = _hole(PairLoopRunner, xs, n_ent, n_rel, d, nb, (3,), opt)
    b = _hole(HolePipeRunner, xs, n_ent, n_rel, d, nb, (3,), opt)
    assert a[1] == b[1] == 3
    assert a[0] > 0 and abs(a[0] - b[0]) <= 2, (a[0], b[0])
    for pid in a[2]:
        np.testing.assert_allclose(b[2][pid], a[2][pid], rtol=RTOL, atol=ATOL, err_msg=pid)


@pytest.mark.parametrize("d,nb,kernel", [(200, 4, "k_pipe_batch"), (8, 3, "k_pipe_fused")])
def test_three_runs_of_one_epoch_equal_one_run_of_three(d, nb, kernel):
    """run(1) x 3 starts every epoch from the caller's key word (keys 0, 1, 2);
    run(3) carries the key from flush to draw inside one stream of replays."""
    n_ent, n_rel, T = 300, 4, 900 + 1
    trip = make_kg(n_ent, n_rel, T)
    a = _train(trip, n_ent, n_rel, d, nb, True, runs=(3,))
    b = _train(trip, n_ent, n_rel, d, nb, True, runs=(1, 1, 1))
    c = _train(trip, n_ent, n_rel, d, nb, True, runs=(2, 1))
    assert a["kernel"] == kernel
    _same(a, b, "run(1) x 3")
    _same(a, c, "run(2); run(1)")


@pytest.mark.parametrize("key", [7, 12])
def test_key_set_before_run_matches_two_launch_at_that_key(key):
    """The caller's key word, set to an odd and to an even value after a first
    run, is what the next run() starts from -- not the runner's own copy of
    the key."""
    n_ent, n_rel, T, d, nb = 300, 4, 700, 200, 3
    trip = make_kg(n_ent, n_rel, T)
    m, upd, r = _transe(trip, n_ent, n_rel, d, nb, True)
    r.run(1)
    r.synchronize()
    r.epoch_key.fill_(key)
    r.run(2)
    got = _state(m, upd, r)
    del r
    # the same schedule on the two-launch runner, and on a fresh pipelined
    # runner per key
    m2, upd2, r2 = _transe(trip, n_ent, n_rel, d, nb, False)
    r2.run(1)
    r2.synchronize()
    r2.epoch_key.fill_(key)
    r2.run(2)
    want = _state(m2, upd2, r2)
    del r2
    assert got["key"] == key + 2
    _same(want, got, "key %d" % key)
    # a fresh runner started at the key, from the zero key's initial tables
    a = _train(trip, n_ent, n_rel, d, nb, True, runs=(2,), key=key)
    b = _train(trip, n_ent, n_rel, d, nb, False, runs=(2,), key=key)
    _same(b, a, "fresh at key %d" % key)


def _pairs(rec, n1, start, count):
    pos, neg = [], []
    for j in range(start, start + count):
        s, o, p, a = (int(x) for x in rec[j])
        b = int(n1[j])
        if a >= 0:
            pos.append((s, o, p))
            neg.append((a, o, p))
        if b >= 0:
            pos.append((s, o, p))
            neg.append((s, b, p))
    return np.array(pos, dtype=np.int64), np.array(neg, dtype=np.int64)


def test_epochs_of_one_run_score_the_records_of_their_keys():
    """The runner's records are not reachable through the library, so the
    chain is: run(3) from key 5 on the pipelined runner (epochs at keys 6 and 7
    drawn at keys its flush launches wrote) equals, bit for bit, three run(1)s of the
    two-launch runner -- and each of those epochs' violation counts equals the
    fp64 oracle's replay of skge_epoch_sample's records at keys 5, 6, 7 from
    the device state before the epoch (test_gpu_runner_oracle.py's replay)."""
    from skge_amd.device import batch_sizes, epoch_records
    n_ent, n_rel, T, d, nb, key, seed = 500, 5, 600, 200, 2, 5, 11
    trip = make_kg(n_ent, n_rel, T)
    got = _train(trip, n_ent, n_rel, d, nb, True, runs=(3,), key=key, seed=seed)
    m, upd, r = _transe(trip, n_ent, n_rel, d, nb, False, seed=seed, key=key)
    total = 0
    for e in range(3):
        params = {pid: p.data.cpu().numpy().astype(np.float64) for pid, p in m.params.items()}
        state = {pid: upd[pid].p2.cpu().numpy().astype(np.float64) for pid in m.params}
        rec, n1 = epoch_records(r.kg, n_ent, seed, key + e)
        rec, n1 = rec.cpu().numpy(), n1.cpu().numpy()
        r.run(1)
        r.synchronize()
        nv = int(r.nviol_total.item()) - total
        total += nv
        want, start = 0, 0
        for c in batch_sizes(T, nb):
            pos, neg = _pairs(rec, n1, start, c)
            start += c
            want += O.pairwise_step("transe", params, state, pos, neg, 0.1, 2.0, "adagrad",
                                    l1=True)[2]
        print("epoch key %d: nviol device %d oracle %d" % (key + e, nv, want))
        assert nv == want > 0, (key + e, nv, want)
    want = _state(m, upd, r)
    del r
    assert got["key"] == key + 3
    _same(want, got, "run(3) from key %d" % key)


def test_error_stop_keeps_tables_key_and_counts():
    """A packed sum that wraps in the first epoch (the star KG of
    test_gpu_device_loop.py, packed sums forced): the epochs queued behind it
    draw no negatives -- run(3) leaves the tables, both AdaGrad states and the
    violation total as run(1) does, the key still advances once per epoch,
    and the next run() is refused."""
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
        r = EpochRunner(m, upd, DeviceKG(trip, m.device), nbatches=2, seed=1, pipelined=True,
                        packed=True)
        r.run(epochs)
        with pytest.raises(L.SkgeError, match="32767"):
            r.synchronize()
        with pytest.raises(L.SkgeError, match="refuses"):
            r.run(1)
        res.append((m.E.data.cpu().numpy().copy(), m.R.data.cpu().numpy().copy(),
                    upd["E"].p2.cpu().numpy().copy(), upd["R"].p2.cpu().numpy().copy(),
                    int(r.nviol_total.item()), int(r.epoch_key.item())))
        del r
    assert res[0][5] == 1 and res[1][5] == 3
    assert res[0][4] == res[1][4]       # the stopped epochs violate nothing
    for a, b in zip(res[0][:4], res[1][:4]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("d,kernel", [(200, "k_pipe_batch"), (8, "k_pipe_fused")])
def test_profile_keeps_its_layout_and_trains_like_run(d, kernel):
    """profile(): one timing per launch as before (the draw, nb1 batches, the
    flush, the key advance), and its eager epoch -- also in the middle of a
    run sequence -- trains exactly like run(1)."""
    n_ent, n_rel, T, nb = 300, 4, 900 + 1, 4   # 4 batches of 225 and a remainder of 1
    trip = make_kg(n_ent, n_rel, T)
    want = _train(trip, n_ent, n_rel, d, nb, True, runs=(3,))
    m, upd, r = _transe(trip, n_ent, n_rel, d, nb, True)
    assert r.kernel == kernel and r.nlaunches == (nb + 1) + 1 + 2
    r.run(1)
    us, stats = r.profile()
    assert len(us) == r.nlaunches == len(stats) and (us > 0).all()
    assert int(stats[1:nb + 2, 2].sum()) > 0 and int(stats[0].sum()) == 0
    r.run(1)
    got = _state(m, upd, r)
    del r
    _same(want, got, "run(1); profile(); run(1)")
