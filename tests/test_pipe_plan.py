"""The pipelined runner's plan, asked without a GPU (skge_pipe_runner_plan,
csrc/skge_pipe_plan.h): for each geometry the form that the rules of
pipe_create give, written down here from those rules and not from what the
plan function returns.

The rules (csrc/skge_pipe_plan.h holds them with their measurements):
  grouped  TransE, more than 16k slot records per batch: 4 * (T // nb) > 16384
  fused    TransE, not grouped, not data-parallel, d / 4 <= 64, and by default
           d / 4 <= 16; SKGE_PIPE_FUSED=0 / 1 forces either
  kq       ceil(d / 4 / 64)
  e8, w32  the entity table's SKGE_ACC_I8X4 / the relation table's SKGE_ACC_I32X2
  replicas of the relation sums: TransE, grouped only: doubled while < 16 and
           256 * reps < (T // nb) // M; HolE: doubled while < 32 and
           2048 * reps < T // nb
  fft      HolE: d % 4 == 0 and d / 2 a product of 2, 3, 5 (d = 8 and 200 are,
           d = 28 is not), unless SKGE_HOLE_DIRECT=1
  pair     HolE FFT at d = 200 while 2 * (largest batch) <= 4096
  launches the draw, one per batch, the flush, the key advance; the batches are
           np.split's: T // nb each and the remainder as one more (T = 1000,
           nb = 3: 333 / 333 / 333 / 1)
"""
import ctypes

import pytest

from skge_amd import _lib as L

FAKE = 0x1000   # a pointer that is tested for NULL and never dereferenced
N, M = 300, 5
BATCH, FUSED, HOLE = 0, 1, 2
HOT_MAX, HOT_REPS, SHARD_WORDS = 256, 4, 64 * 32


def table(rows, width, mode, slots=0, ada=True, gate=False):
    t = L.SkgeTable()
    t.param, t.acc_sum, t.acc_cnt = FAKE, FAKE, FAKE
    t.state = FAKE if ada else None
    t.opt = L.SKGE_ADAGRAD if ada else L.SKGE_SGD
    t.rows, t.width, t.acc_mode, t.acc_replicas = rows, width, mode, 1
    if slots:
        t.acc_touched, t.touched_cap = FAKE, slots
    if gate:
        t.gate = FAKE
    return t


def transe_tables(d, T, nb, e8=False, w32=False, m=M, **kw):
    return (table(N, d, L.SKGE_ACC_I8X4 if e8 else L.SKGE_ACC_I16X4, slots=4 * (T // nb), **kw),
            table(m, d, L.SKGE_ACC_I32X2 if w32 else L.SKGE_ACC_I16X4, **kw))


def hole_tables(d, T, nb):
    return table(N, d, L.SKGE_ACC_F32, slots=4 * (T // nb)), table(M, d, L.SKGE_ACC_F32)


def plan(ent, rel, d, T, nb, flags=0, hole=0):
    out = L.SkgePipePlan()
    rc = L.load().skge_pipe_runner_plan(ent, rel, d, T, nb, flags, hole, out)
    return rc, out


def nbatches(T, nb):
    return len(range(0, T, T // nb))


def alloc_bytes(d, T, nb, fused, grouped, e8, w32, reps, m=M, dp=False, hot=True, ada=True):
    """What pipe_create allocates for a TransE runner, buffer by buffer as its
    allocation calls list them (hot-row buffers for HOT_MAX rows)."""
    nq, bs, nb1 = d // 4, T // nb, nbatches(T, nb)
    state = 2 if ada else 1
    if fused:
        ent = N * d * 4 * state + 2 * (N * nq * (4 if e8 else 8) + N * 4 + 4 * bs * 4) + N * 16
    else:
        ent = N * 4 + N * nq * (4 if e8 else 8) + N * 4 + 4 * bs * 4 + 2 * N * 4
        ent += 2 * N * 4 if grouped else 0
        if hot and not e8 and not dp:
            hw = (nq + 15) // 16 * 16
            ent += N * 4 + HOT_MAX * (4 + 3 * (HOT_REPS * hw * 8 + HOT_REPS * 4) +
                                      2 * state * d * 4)
    rw = ((2 * nq if w32 else nq) + 1 + 15) // 16 * 16
    rel = m * d * 4 * state + 3 * reps * m * rw * 8
    common = T * 16 + T * 4 + 4 + (0 if dp else 8) + (nb1 + 3) * 3 * SHARD_WORDS * 4 + \
        SHARD_WORDS * 4
    return ent + rel + common


# (d, T, nb, tables' and call's options, environment) -> (kernel, grouped, e8, w32, kq, replicas)
TRANSE = [
    ("fused", 64, 1000, 3, {}, {}, (FUSED, 0, 0, 0, 1, 1)),
    ("fused-off", 64, 1000, 3, {}, {"SKGE_PIPE_FUSED": "0"}, (BATCH, 0, 0, 0, 1, 1)),
    ("batch-kq1", 200, 1000, 3, {}, {}, (BATCH, 0, 0, 0, 1, 1)),
    ("batch-kq2", 260, 1000, 3, {}, {}, (BATCH, 0, 0, 0, 2, 1)),
    ("w32", 200, 1000, 3, {"w32": True}, {}, (BATCH, 0, 0, 1, 1, 1)),
    ("e8", 200, 1000, 3, {"e8": True}, {}, (BATCH, 0, 1, 0, 1, 1)),
    # bs = 4500: 18000 slot records; bs / M = 900 adds per relation row -> 4 replicas
    ("grouped-reps", 200, 9000, 2, {}, {}, (BATCH, 1, 0, 0, 1, 4)),
    # ... 50 relations: 90 adds per row -> one copy
    ("grouped-one-copy", 200, 9000, 2, {"m": 50}, {}, (BATCH, 1, 0, 0, 1, 1)),
    ("dp", 200, 1000, 3, {"dp": True}, {}, (BATCH, 0, 0, 0, 1, 1)),
    ("dp-never-fused", 64, 1000, 3, {"dp": True}, {}, (BATCH, 0, 0, 0, 1, 1)),
    ("dp-fused-forced", 64, 1000, 3, {"dp": True}, {"SKGE_PIPE_FUSED": "1"},
     (BATCH, 0, 0, 0, 1, 1)),
    ("fused-forced", 200, 1000, 3, {}, {"SKGE_PIPE_FUSED": "1"}, (FUSED, 0, 0, 0, 1, 1)),
    ("fused-forced-too-wide", 260, 1000, 3, {}, {"SKGE_PIPE_FUSED": "1"},
     (BATCH, 0, 0, 0, 2, 1)),
    ("sgd", 200, 1000, 3, {"ada": False}, {}, (BATCH, 0, 0, 0, 1, 1)),
    ("one-batch", 200, 1000, 1, {}, {}, (BATCH, 0, 0, 0, 1, 1)),
]


@pytest.mark.parametrize("name,d,T,nb,opt,env,want", TRANSE, ids=[c[0] for c in TRANSE])
def test_transe_form(name, d, T, nb, opt, env, want, monkeypatch):
    monkeypatch.delenv("SKGE_PIPE_FUSED", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    opt = dict(opt)
    dp = opt.pop("dp", False)
    ent, rel = transe_tables(d, T, nb, **opt)
    rc, p = plan(ent, rel, d, T, nb, flags=1 if dp else 0)
    assert rc == 0, L.load().skge_last_error()
    kernel, grouped, e8, w32, kq, reps = want
    assert (p.kernel, p.grouped, p.e8, p.w32, p.kq, p.rel_reps) == want
    assert (p.fft, p.pair) == (0, 0)
    assert p.nlaunches == nbatches(T, nb) + 3
    assert p.device_bytes == alloc_bytes(d, T, nb, kernel == FUSED, grouped, e8, w32, reps,
                                         m=opt.get("m", M), dp=dp, ada=opt.get("ada", True))


def test_ragged_batches():
    """T = 1000, nb = 3: np.split's batches are 333 / 333 / 333 and the one
    triple left over, so the epoch has four batch launches (seven in all);
    an even split has none left over."""
    assert nbatches(1000, 3) == 4
    rc, p = plan(*transe_tables(200, 1000, 3), 200, 1000, 3)
    assert rc == 0 and p.nlaunches == 7
    rc, p = plan(*transe_tables(200, 999, 3), 200, 999, 3)
    assert rc == 0 and p.nlaunches == 6


# (d, T, nb, environment) -> (fft, pair, replicas)
HOLE_CASES = [
    ("pair-fft", 200, 1000, 3, {}, (1, 1, 1)),
    # one batch of 3000: 6000 scoring waves > 4096; 2048 < 3000 -> 2 replicas
    ("no-pair", 200, 3000, 1, {}, (1, 0, 2)),
    # d / 2 = 4 = 2 * 2: the FFT form applies to d = 8 too
    ("d8", 8, 1000, 3, {}, (1, 0, 1)),
    ("d8-direct", 8, 1000, 3, {"SKGE_HOLE_DIRECT": "1"}, (0, 0, 1)),
    # d / 2 = 14 = 2 * 7: the direct form
    ("d28-direct", 28, 1000, 3, {}, (0, 0, 1)),
    ("rreps", 200, 1000, 3, {"SKGE_HPIPE_RREPS": "8"}, (1, 1, 8)),
]


@pytest.mark.parametrize("name,d,T,nb,env,want", HOLE_CASES, ids=[c[0] for c in HOLE_CASES])
def test_hole_form(name, d, T, nb, env, want, monkeypatch):
    for k in ("SKGE_HOLE_DIRECT", "SKGE_HPIPE_RREPS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ent, rel = hole_tables(d, T, nb)
    rc, p = plan(ent, rel, d, T, nb, hole=1)
    assert rc == 0, L.load().skge_last_error()
    assert (p.fft, p.pair, p.rel_reps) == want
    assert (p.kernel, p.grouped, p.e8, p.w32, p.kq) == (HOLE, 0, 0, 0, 1)
    assert p.nlaunches == nbatches(T, nb) + 3
    assert p.device_bytes > 0


PACKED_TEXT = (b"pipelined runner: needs a packed (SKGE_ACC_I16X4) entity table with slot records, "
               b"a dense single-copy SKGE_ACC_I16X4 / SKGE_ACC_I32X2 relation table, d % 4 == 0, "
               b"no gates")
HOLE_TEXT = (b"pipelined HolE runner: needs fp32 accumulators (entity table with slot records, "
             b"dense single-copy relation table), d % 4 == 0, 4 <= d <= 256, no gates")


def _refusals():
    T, nb = 1000, 3
    ent50, rel50 = transe_tables(50, T, nb)
    ent, rel = transe_tables(52, T, nb)
    gated, _ = transe_tables(200, T, nb, gate=True)
    _, rel200 = transe_tables(200, T, nb)
    hent, hrel = hole_tables(260, T, nb)
    small, _ = transe_tables(200, T, 6)   # slot records for batches of 166
    return [
        ("width-50", ent50, rel50, 50, T, nb, 0, 0,
         b"ent: packed accumulator needs width % 4 == 0 and <= 1024"),
        ("d-50", ent, rel, 50, T, nb, 0, 0, PACKED_TEXT),
        ("gate", gated, rel200, 200, T, nb, 0, 0, PACKED_TEXT),
        ("hole-260", hent, hrel, 260, T, nb, 0, 1, HOLE_TEXT),
        ("hole-packed", gated, rel200, 200, T, nb, 0, 1, HOLE_TEXT),
        ("flags", ent, rel, 52, T, nb, 2, 0, b"pipelined runner: unknown flags 2"),
        ("hole-dp", hent, hrel, 260, T, nb, 1, 1,
         b"pipelined runner: the data-parallel form is TransE-L1 only"),
        ("null", None, rel, 52, T, nb, 0, 0, b"pipelined runner: NULL table"),
        ("T", ent, rel, 52, 0, nb, 0, 0, b"pipelined runner: T must be >= 1"),
        ("nbatches", ent, rel, 52, T, T + 1, 0, 0,
         b"pipelined runner: nbatches must be in [1, T]"),
        ("slots", small, rel200, 200, T, nb, 0, 0,
         b"pipelined runner: batch too large for the slot capacity"),
    ]


@pytest.mark.parametrize("case", _refusals(), ids=[c[0] for c in _refusals()])
def test_refusals_are_the_constructors(case):
    """The plan refuses what the constructors refuse, in their words: the same
    call to the constructor (which refuses before its first HIP call, so this
    runs without a GPU) leaves the same error text."""
    _, ent, rel, d, T, nb, flags, hole, text = case
    lib = L.load()
    rc, _ = plan(ent, rel, d, T, nb, flags, hole)
    assert rc == -1
    assert lib.skge_last_error() == text
    word = ctypes.c_uint64(0)
    args = (ent, rel, d, FAKE, T, FAKE, 4096, nb, 0, ctypes.addressof(word), 1.0, 10, None)
    if hole:
        h = lib.skge_hole_pipe_runner_create_smp(FAKE, 0, *args, None) if not flags else None
    else:
        h = lib.skge_pipe_runner_create_smp(FAKE, *args, flags, None)
    assert not h
    if not (hole and flags):   # (the HolE constructor takes no flags word)
        assert lib.skge_last_error() == text
