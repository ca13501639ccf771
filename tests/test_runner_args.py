"""CPU pin of the device epoch runners' argument refusals.

Every create entry point (skge_runner_create, skge_pipe_runner_create,
skge_pipe_runner_create_ex with SKGE_PIPE_DP, skge_hole_pipe_runner_create,
skge_pair_runner_create, skge_triple_runner_create, skge_pair_runner_create_multi,
skge_triple_runner_create_multi, skge_sadv_runner_create) is called with one bad
argument at a time; each call must return a NULL handle and leave a non-empty
skge_last_error.  Only arguments refused BEFORE the first HIP call are used, so
no device is needed and no capture starts: the pointers are fake (never
dereferenced on the host) and every call carries a "backstop" -- an argument
that is itself refused on the host, but only AFTER the argument check under
test -- so a case that slipped through the check would still stop before HIP
and would show up as the backstop's message:

  two-launch runner     stream == NULL ("non-default stream"), its last check
  every other runner    an entity table with slot records and touched_cap 0
                        ("touched slots" / "slot capacity"), checked right
                        after the arguments

The positive controls are the loosest bad-looking arguments each runner takes:
they must pass the argument check and end at the backstop (read from the code:
csrc/skge_epoch.hip, skge_pipeline.hip, skge_pairloop.hip, skge_tripleloop.hip
check the backstop after the arguments and before the first hipMalloc).

The accept / refuse outcome of every row is the same before and after the
runners moved onto csrc/skge_graph_runner.h.  Message texts that changed with
that move (the outcome did not):
  * pipelined runners (create, create_ex, hole): every row but "NULL tables"
    said "pipelined runner: bad arguments"; they now name the argument, as
    the other runners do ("pipelined runner: ntries >= 1", ...).
  * pair / triple runner: every text gained the "pair runner: " / "triple
    runner: " prefix; a NULL table now says "NULL table"; the T and
    set-capacity texts carry the bound as a number ("T must be in [1,
    2147483647]", "set capacity must be a power of 2 >= 74"); the triple
    runner answers a TransE model code with "logistic loss is defined for HolE
    and RESCAL only" where a code outside the enum said "unknown model".
  * two-launch runner: "nbatches must be in [1, T]" and the stream text gained
    the "runner: " prefix; its other rows are skge_transe_sample_grad's checks
    and did not change.

The rows of the _multi and sadv creates were added, with the texts the library
gave then, before the five loop creates moved onto csrc/skge_loop_runner.h;
every outcome is the same after it.  Texts that move unified:
  * every touched-capacity refusal of the five creates reads "<who>: <entity |
    relation | W> accumulator needs N touched slots, has M".  Before: the pair
    create said "needs 8 * batch_size touched slots" without a number, the
    triple create "needs 6 * batch_size = N touched slots" without "has", the
    _multi and sadv creates spelled the product out before the number ("4 * K
    * batch_size = N"), and the triple _multi create called RESCAL's W the
    relation accumulator.
  * triple runner: a model code outside the enum is "unknown model" again (the
    shared check comes first); TransE is still "logistic loss is defined for
    HolE and RESCAL only".
"""
import ctypes

import pytest

from skge_amd import _lib as L

T, N_ENT, N_REL, D = 37, 11, 3, 8
CAP = 128                      # power of two >= 2T
INT32_MAX = 2 ** 31 - 1
FAKE = ctypes.c_void_p(0x1000)     # a non-NULL pointer no host code reads
NULL = None

RUNNERS = ("epoch", "pipe", "pipe_dp", "hole_pipe", "pair", "triple", "pair_multi", "triple_multi",
           "sadv")
MULTI = ("pair_multi", "triple_multi", "sadv")   # the runners that take a skge_negatives_t
# what the backstop's refusal says, per runner
BACKSTOP = {"epoch": "non-default stream", "pipe": "slot capacity", "pipe_dp": "slot capacity",
            "hole_pipe": "slot capacity", "pair": "touched slots", "triple": "touched slots",
            "pair_multi": "touched slots", "triple_multi": "touched slots",
            "sadv": "touched slots"}


def table(rows, mode, slots):
    t = L.SkgeTable()
    t.param = t.state = t.acc_sum = t.acc_cnt = 0x1000
    t.acc_touched = 0x1000 if slots else None
    t.rows, t.width, t.touched_cap = rows, D, 0
    t.acc_mode, t.acc_replicas = mode, 1
    t.lr = 0.1
    return t


def negs(n=1, modes=(0, 1, 2), rel_range=N_REL):
    m = list(modes) + [0] * (8 - len(modes))
    return L.SkgeNegatives(n, len(modes), (L.c_i * 8)(*m), rel_range)


K = 3                          # slots per positive of the default negs()


def good(runner):
    packed = runner in ("pipe", "pipe_dp")
    mode = L.SKGE_ACC_I16X4 if packed else L.SKGE_ACC_F32
    return dict(stream=NULL if runner == "epoch" else FAKE,
                model=L.SKGE_TRANSE_L1 if runner == "sadv" else L.SKGE_HOLE, d=D,
                ent=ctypes.byref(table(N_ENT, mode, True)),
                rel=ctypes.byref(table(N_REL, mode, False)), trip=FAKE, T=T, set=FAKE, cap=CAP,
                nbatches=5, key=FAKE, ntries=100, negs=negs())


def create(runner, a):
    lib = L.load()
    tail = (a["trip"], a["T"], a["set"], a["cap"], a["nbatches"], 7, a["key"])
    if runner == "epoch":
        return lib.skge_runner_create(a["stream"], 1, a["ent"], a["rel"], D, *tail, 1.0,
                                      a["ntries"], NULL, NULL)
    if runner == "pipe":
        return lib.skge_pipe_runner_create(a["stream"], a["ent"], a["rel"], D, *tail, 1.0,
                                           a["ntries"], NULL)
    if runner == "pipe_dp":
        return lib.skge_pipe_runner_create_ex(a["stream"], a["ent"], a["rel"], D, *tail, 1.0,
                                              a["ntries"], NULL, 1)
    if runner == "hole_pipe":
        return lib.skge_hole_pipe_runner_create(a["stream"], 0, a["ent"], a["rel"], D, *tail, 1.0,
                                                a["ntries"], NULL)
    if runner == "pair":
        return lib.skge_pair_runner_create(a["stream"], a["model"], 0, a["ent"], a["rel"], a["d"],
                                           *tail, 1.0, a["ntries"], NULL)
    if runner == "pair_multi":
        return lib.skge_pair_runner_create_multi(a["stream"], a["model"], 0, a["ent"], a["rel"],
                                                 a["d"], *tail, 1.0, a["ntries"], NULL, NULL,
                                                 a["negs"])
    if runner == "triple_multi":
        return lib.skge_triple_runner_create_multi(a["stream"], a["model"], a["ent"], a["rel"],
                                                   a["d"], *tail, a["ntries"], NULL, NULL, a["negs"])
    if runner == "sadv":
        return lib.skge_sadv_runner_create(a["stream"], a["model"], a["ent"], a["rel"], a["d"],
                                           *tail, 6.0, 1.0, a["ntries"], NULL, NULL, a["negs"])
    return lib.skge_triple_runner_create(a["stream"], a["model"], a["ent"], a["rel"], a["d"], *tail,
                                         a["ntries"], NULL)


def refused(runner, **bad):
    a = good(runner)
    a.update(bad)
    h = create(runner, a)
    err = L.load().skge_last_error().decode()
    assert not h, "%s accepted %r" % (runner, bad)
    assert err
    return err


# each runner's own lower bound on the set capacity: the two-launch runner takes
# any power of two, the pipelined ones >= 4, the pair / triple loops >= 2T
CAP_BELOW = {"epoch": 0, "pipe": 2, "pipe_dp": 2, "hole_pipe": 2, "pair": 64, "triple": 64,
             "pair_multi": 64, "triple_multi": 64, "sadv": 64}

CASES = [
    ("ent NULL", lambda r: dict(ent=NULL)),
    ("rel NULL", lambda r: dict(rel=NULL)),
    ("trip NULL", lambda r: dict(trip=NULL)),
    ("set NULL", lambda r: dict(set=NULL)),
    ("key NULL", lambda r: dict(key=NULL)),
    ("T = 0", lambda r: dict(T=0)),
    ("nbatches = 0", lambda r: dict(nbatches=0)),
    ("nbatches = T + 1", lambda r: dict(nbatches=T + 1)),
    ("capacity not a power of two", lambda r: dict(cap=CAP + 4)),
    ("capacity below the bound", lambda r: dict(cap=CAP_BELOW[r])),
    ("ntries = 0", lambda r: dict(ntries=0)),
]


@pytest.mark.parametrize("runner", RUNNERS)
@pytest.mark.parametrize("name,bad", CASES, ids=[c[0] for c in CASES])
def test_bad_argument_is_refused_by_the_argument_check(runner, name, bad):
    err = refused(runner, **bad(runner))
    assert BACKSTOP[runner] not in err, err


@pytest.mark.parametrize("runner", RUNNERS)
def test_null_stream_is_refused(runner):
    err = refused(runner, stream=NULL)
    if runner == "epoch":
        assert "non-default stream" in err
    else:
        assert BACKSTOP[runner] not in err, err


def test_triple_runner_refuses_transe_and_a_large_T():
    err = refused("triple", model=L.SKGE_TRANSE_L1)
    assert BACKSTOP["triple"] not in err, err
    err = refused("triple", T=INT32_MAX // 3 + 1, cap=2 ** 31, nbatches=1)
    assert BACKSTOP["triple"] not in err, err


# each _multi runner's bound on T: its batch's pairs / triples / slots are ints
T_MAX = {"pair_multi": INT32_MAX // (4 * K), "triple_multi": INT32_MAX // (3 * (1 + K)),
         "sadv": INT32_MAX // (2 + K)}

NEG_CASES = [
    ("negs NULL", dict(negs=NULL)),
    ("K = 0", dict(negs=negs(n=0))),
    ("K over the bound", dict(negs=negs(n=33, modes=(0, 1)))),
    ("mode 2 with rel_range 0", dict(negs=negs(rel_range=0))),
    ("mode 3", dict(negs=negs(modes=(0, 3)))),
]


@pytest.mark.parametrize("runner", MULTI)
@pytest.mark.parametrize("name,bad", NEG_CASES, ids=[c[0] for c in NEG_CASES])
def test_bad_negatives_are_refused_by_the_argument_check(runner, name, bad):
    err = refused(runner, **bad)
    assert BACKSTOP[runner] not in err, err


@pytest.mark.parametrize("runner", MULTI)
def test_multi_runners_refuse_a_large_T(runner):
    err = refused(runner, T=T_MAX[runner] + 1, cap=2 ** 31, nbatches=1)
    assert BACKSTOP[runner] not in err, err


@pytest.mark.parametrize("runner,bad", [
    ("pair", dict(model=4)), ("pair_multi", dict(model=4)),
    ("pair", dict(model=L.SKGE_COMPLEX, d=7)), ("pair_multi", dict(model=L.SKGE_COMPLEX, d=7)),
    ("pair", dict(model=L.SKGE_ROTATE, d=7)), ("pair_multi", dict(model=L.SKGE_ROTATE, d=7)),
    ("triple", dict(model=4)), ("triple_multi", dict(model=4)),
    ("triple", dict(model=L.SKGE_ROTATE)), ("triple_multi", dict(model=L.SKGE_ROTATE)),
    ("triple_multi", dict(model=L.SKGE_TRANSE_L1)),
    ("triple", dict(model=L.SKGE_COMPLEX, d=7)), ("triple_multi", dict(model=L.SKGE_COMPLEX, d=7)),
    ("sadv", dict(model=L.SKGE_HOLE)), ("sadv", dict(model=4)),
    ("sadv", dict(model=L.SKGE_ROTATE, d=7)),
], ids=lambda v: v if isinstance(v, str) else ",".join("%s=%s" % kv for kv in v.items()))
def test_model_and_width_refusals(runner, bad):
    err = refused(runner, **bad)
    assert BACKSTOP[runner] not in err, err


@pytest.mark.parametrize("runner", ("triple",) + MULTI)
def test_relation_touched_capacity_is_refused(runner):
    """The backstop on the relation side alone: an entity table without slot
    records, a relation table with them and touched_cap 0.  (The pair runner's
    (1, [0, 1]) create leaves this one to skge_pair_step at capture, after the
    first HIP call, so it has no row here.)"""
    err = refused(runner, ent=ctypes.byref(table(N_ENT, L.SKGE_ACC_F32, False)),
                  rel=ctypes.byref(table(N_REL, L.SKGE_ACC_F32, True)))
    assert "relation accumulator needs" in err and "touched slots, has 0" in err, err


@pytest.mark.parametrize("runner,loose", [
    # a set smaller than 2T: the two-launch and pipelined runners take it
    ("epoch", dict(cap=4)), ("pipe", dict(cap=4)), ("pipe_dp", dict(cap=4)),
    ("hole_pipe", dict(cap=4)),
    # the pair loop takes what the triple loop's 3T positions cannot hold
    ("pair", dict(T=INT32_MAX // 3 + 1, cap=2 ** 31, nbatches=1)),
    ("pair", dict(model=L.SKGE_TRANSE_L1)),
    ("triple", dict(T=INT32_MAX // 3, cap=2 ** 31, nbatches=1)),
    # a set of exactly 2T slots
    ("pair", dict(T=32, cap=64)), ("triple", dict(T=32, cap=64)),
    ("pair_multi", dict(T=32, cap=64)), ("triple_multi", dict(T=32, cap=64)),
    ("sadv", dict(T=32, cap=64)),
    # the largest T each _multi runner's int indices hold
    ("pair_multi", dict(T=T_MAX["pair_multi"], cap=2 ** 31, nbatches=1)),
    ("triple_multi", dict(T=T_MAX["triple_multi"], cap=2 ** 31, nbatches=1)),
    ("sadv", dict(T=T_MAX["sadv"], cap=2 ** 31, nbatches=1)),
    # the widest negatives: K = 64 slots; a complex model with an even d
    ("pair_multi", dict(negs=negs(n=32, modes=(0, 1)))),
    ("triple_multi", dict(negs=negs(n=32, modes=(0, 1)))),
    ("sadv", dict(negs=negs(n=32, modes=(0, 1)))),
    ("pair_multi", dict(model=L.SKGE_ROTATE)), ("triple_multi", dict(model=L.SKGE_COMPLEX)),
    ("sadv", dict(model=L.SKGE_ROTATE)),
], ids=lambda v: v if isinstance(v, str) else ",".join("%s=%s" % kv for kv in v.items()))
def test_loosest_accepted_arguments_pass_the_argument_check(runner, loose):
    err = refused(runner, **loose)
    assert BACKSTOP[runner] in err, err
