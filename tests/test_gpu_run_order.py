"""run()'s ordering against the caller's stream, paid for on the host
(skge_run_order_begin / _end, include/skge_hip.h; device._Runner.run).

Ordered before: parameters written on the caller's stream behind a long
torch.cuda._sleep, run(1) called at once, against the same steps with a full
synchronise before run(1) -- on every runner family, from the default stream
and from a side stream.  Ordered after: a clone queued on the caller's stream
right after run(2).  The path codes (runner.last_order) in the situations of
the fit loop / the benchmark (0: nothing enqueued) and with work pending (1:
the host waited).  profile() takes the same two calls.

Sizes: the race scenario's of tests/test_gpu_device_loop.py (3000 entities,
11 relations, 12000 triples, 10 batches, AdaGrad, fixed seeds)."""
import contextlib
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_ENT, N_REL, T, NB, SEED = 3000, 11, 12000, 10, 9
SLEEP = int(2e8)

# case -> (model, d, runner keywords, the kernel / path it is there for)
CASES = {
    "pipelined_d200": ("transe", 200, {}),                  # k_pipe_batch
    "fused_d64": ("transe", 64, {}),                        # k_pipe_fused
    "padded_d50": ("transe", 50, {}),                       # _pad_in / _pad_out
    "two_launch_d64": ("transe", 64, {"pipelined": False}),  # skge_runner_*
    "hole_d32": ("hole", 32, {}),                           # k_hole_pipe
}


@functools.lru_cache(maxsize=None)
def triples():
    rs = np.random.RandomState(4)
    codes = np.unique(rs.randint(0, N_ENT * N_ENT * N_REL, size=2 * T, dtype=np.int64))
    codes = rs.permutation(codes)[:T]
    assert len(codes) == T
    out = np.stack([codes // (N_ENT * N_REL), codes // N_REL % N_ENT, codes % N_REL], axis=1)
    return np.ascontiguousarray(out.astype(np.int32))


def build(case, **kw):
    import skge_amd as S
    from skge_amd.device import DeviceKG, EpochRunner, HolePipeRunner
    kind, d, ckw = CASES[case]
    np.random.seed(21)
    if kind == "transe":
        m, cls, margin = S.TransE((N_ENT, N_ENT, N_REL), d), EpochRunner, 2.0
    else:
        m, cls, margin = S.HolE((N_ENT, N_ENT, N_REL), d, rparam=0.05), HolePipeRunner, 0.2
    m.add_hyperparam("margin", margin)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    r = cls(m, upd, DeviceKG(triples(), m.device), nbatches=NB, seed=SEED, **dict(ckw, **kw))
    if case == "padded_d50":
        assert r._pad
    if case != "two_launch_d64":
        assert r.pipelined
    return m, upd, r


def error_word(r):
    from skge_amd import _lib as L
    if r.pipelined:
        return int(L.lib().skge_pipe_runner_error(r.handle, L.stream_ptr(r.stream)))
    return int(L.lib().skge_device_error(L.stream_ptr(r.stream), 0))


def result(m, upd, r):
    r.synchronize()
    torch.cuda.synchronize()
    out = {pid: p.data.cpu().numpy().copy() for pid, p in m.params.items()}
    out.update({"p" + pid: u.state().cpu().numpy().copy() for pid, u in upd.items()})
    out["nviol"] = int(r.nviol_total.item())
    out["err"] = error_word(r)
    return out


def late_write_then_run(case, sync_first, side_stream):
    """Other parameters copied in on the caller's stream behind a long sleep,
    then run(1): at once, or (the reference) after a full synchronise."""
    m, upd, r = build(case)
    other = {pid: p.data.roll(1, 0).clone() for pid, p in m.params.items()}
    torch.cuda.synchronize()
    ctx = torch.cuda.stream(torch.cuda.Stream()) if side_stream else contextlib.nullcontext()
    with ctx:
        torch.cuda._sleep(SLEEP)
        for pid, p in m.params.items():
            p.data.copy_(other[pid])
        if sync_first:
            torch.cuda.synchronize()
        r.run(1)
    out = result(m, upd, r)
    out["order"] = r.last_order
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    return late_write_then_run(case, True, False)


def assert_same_training(case, got, ref):
    """TransE-L1 sums are exact integers: bit-equal.  The pipelined HolE
    runner adds fp32 atomics in any order, so two runs of the same ordered
    steps already differ in the last bits and by a tie or two in the
    violation count (tests/test_gpu_pairloop.py: 1e-5, two violations, for
    this runner at d = 32); a run that read parameters from before the copy
    would be off by the size of the parameters themselves (~1e-1)."""
    assert got["err"] == 0 and ref["err"] == 0
    keys = [k for k in ref if k not in ("nviol", "err", "order")]
    assert len(keys) == 4
    if CASES[case][0] == "hole":
        assert ref["nviol"] > 0 and abs(got["nviol"] - ref["nviol"]) <= 2
        for k in keys:
            np.testing.assert_allclose(got[k], ref[k], rtol=1e-5, atol=1e-5, err_msg=k)
        return
    assert got["nviol"] == ref["nviol"] > 0
    for k in keys:
        assert np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("side_stream", [False, True], ids=["default_stream", "side_stream"])
@pytest.mark.parametrize("case", list(CASES))
def test_run_ordered_after_callers_pending_writes(case, side_stream):
    """The caller's late parameter writes reach the runner's first launch:
    the host waits for them (path 1), nothing is queued on the runner's stream."""
    ref = reference(case)
    assert ref["order"] == 0          # the synchronised caller: nothing enqueued
    got = late_write_then_run(case, False, side_stream)
    assert got["order"] == 1
    assert_same_training(case, got, ref)


@pytest.mark.parametrize("queued", [False, True], ids=["host_wait", "queued_event"])
def test_callers_later_work_ordered_after_run(queued):
    """A clone queued on the caller's stream right after run(2), no
    synchronise in between, holds the tables after both epochs -- with the
    host wait (end path 1) and with the queued event (end path 2)."""
    outs = []
    for sync in (True, False):
        m, upd, r = build("pipelined_d200")
        r.queued_after = queued
        torch.cuda.synchronize()
        r.run(2)
        assert r.last_order == 0 and r.last_order_end == (2 if queued else 1)
        if sync:
            r.synchronize()
            torch.cuda.synchronize()
        clones = {pid: p.data.clone() for pid, p in m.params.items()}
        r.synchronize()
        torch.cuda.synchronize()
        assert error_word(r) == 0
        outs.append({pid: c.cpu().numpy() for pid, c in clones.items()})
    for pid in outs[0]:
        assert np.array_equal(outs[0][pid], outs[1][pid]), pid


@pytest.mark.parametrize("side_stream", [False, True], ids=["default_stream", "side_stream"])
def test_path_codes_of_a_synchronised_caller(side_stream):
    """After a synchronise (the fit loop's and the benchmark's timed
    region's situation) run(1), and run(3) right after runner.synchronize(),
    enqueue nothing: path 0.  On the runner's own stream: 0 both ways."""
    m, upd, r = build("pipelined_d200")
    ctx = torch.cuda.stream(torch.cuda.Stream()) if side_stream else contextlib.nullcontext()
    with ctx:
        torch.cuda.synchronize()
        r.run(1)
        assert r.last_order == 0 and r.last_order_end == 1
        r.synchronize()
        r.run(3)
        assert r.last_order == 0
    with torch.cuda.stream(r.stream):
        r.run(1)
        assert r.last_order == 0 and r.last_order_end == 0
    r.synchronize()
    assert error_word(r) == 0 and int(r.epoch_key.item()) == 5


def test_order_calls_refuse_a_null_runner_stream():
    from skge_amd import _lib as L
    lib = L.lib()
    assert lib.skge_run_order_begin(None, None) == -1
    assert b"stream" in lib.skge_last_error()
    assert lib.skge_run_order_end(None, None, 0) == -1


@pytest.mark.parametrize("case", ["pipelined_d200", "padded_d50"])
def test_profile_trains_like_run(case):
    """profile() (one eager epoch, ordered by the same two calls) leaves the
    tables run(1) leaves from the same start."""
    outs = []
    for prof in (False, True):
        m, upd, r = build(case)
        torch.cuda.synchronize()
        if prof:
            us, stats = r.profile()
            assert len(us) == r.nlaunches and r.last_order == 0
        else:
            r.run(1)
        outs.append(result(m, upd, r))
    assert_same_training(case, outs[1], outs[0])
