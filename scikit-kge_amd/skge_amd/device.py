"""Device-resident training data and the native epoch runners.

DeviceKG holds the training triples on the GPU ([T, 3] int32, (s, o, p)) and
the open-addressing triple set the device sampler rejects against.
EpochRunner wraps the TransE runners (skge_pipe_runner_* / skge_runner_*,
csrc/skge_pipeline.hip, skge_epoch.hip) and PairLoopRunner the any-model pair
loop (skge_pair_runner_*, csrc/skge_pairloop.hip): one epoch of
PairwiseStochasticTrainer batches (nbatches full batches + the remainder,
skge/base.py:1246-1268), captured once into a hipGraph and replayed."""
import math
import os as _os
import timeit
import warnings

import numpy as np
import torch

from . import _lib as L
from .util import to_device_triples


def _next_pow2(n):
    c = 1
    while c < n:
        c <<= 1
    return c


class DeviceKG(object):
    def __init__(self, xs, device=None, stream=None):
        L.require_gpu()
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.trip = to_device_triples(xs, dev)
        self.T = int(self.trip.shape[0])
        self.capacity = _next_pow2(max(2 * self.T, 4))
        nbytes = int(L.lib().skge_triple_set_bytes(self.capacity))
        self.slots = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        L.check(L.lib().skge_triple_set_build(L.stream_ptr(stream), L.ptr(self.trip), self.T,
                                              L.ptr(self.slots), self.capacity), "triple set build")
        self._pools = {}

    def pools(self, n_rel):
        """The type index of the triples as a CSR of 2 * n_rel pools
        (include/skge_hip.h, skge_sampler_t), built on first use: pool
        2p + side holds the ascending unique entity ids seen as subject
        (side 0) or object (side 1) of relation p.  Returns (pool_off int64
        [2 * n_rel + 1], pool_ent int32); a relation that never occurs has two
        empty pools.  The typed and LCWA device samplers draw from it."""
        n_rel = int(n_rel)
        if n_rel not in self._pools:
            t = self.trip.long()
            p = t[:, 2]
            if n_rel < 1 or int(p.min().item()) < 0 or int(p.max().item()) >= n_rel:
                raise ValueError("type index: relation ids must be in [0, %d)" % n_rel)
            if int(t[:, :2].min().item()) < 0:
                raise ValueError("type index: negative entity id")
            n = int(t[:, :2].max().item()) + 1
            keys = torch.unique(torch.cat([(2 * p) * n + t[:, 0], (2 * p + 1) * n + t[:, 1]]))
            bounds = torch.arange(2 * n_rel + 1, dtype=torch.int64, device=t.device) * n
            off = torch.searchsorted(keys, bounds).to(torch.int64).contiguous()
            ent = (keys % n).to(torch.int32).contiguous()
            self._pools[n_rel] = (off, ent)
        return self._pools[n_rel]

    def sampler(self, kind, n_rel=None):
        """skge_sampler_t for `kind` (None: RANDOM, the entry points' NULL);
        the struct holds pointers into pools(n_rel), which this object keeps."""
        if kind == L.SKGE_SAMPLER_RANDOM:
            return None
        if kind not in (L.SKGE_SAMPLER_TYPED, L.SKGE_SAMPLER_LCWA):
            raise ValueError("unknown sampler kind %r" % (kind,))
        if n_rel is None:
            raise ValueError("the typed and LCWA samplers need the model's relation count")
        off, ent = self.pools(n_rel)
        return L.SkgeSampler(int(kind), int(n_rel), off.data_ptr(), ent.data_ptr())


PACKED_MAX = 32767   # a 16-bit packed field's bound (csrc/skge_pipeline.hip PACKED_MAX)


def _row_counts(col, n):
    return torch.bincount(col.long(), minlength=n)


def corruption_load(kind, pool_off, pool_ent, rel_counts, n_ent, batch, T):
    """Expected corruptions per batch of every entity row, float64 [n_ent] on
    the pools' device (pure tensor arithmetic: CPU tensors stay on the CPU).
    kind: SKGE_SAMPLER_*; pool_off [2 * n_rel + 1] / pool_ent: the type index
    (DeviceKG.pools); rel_counts [n_rel]: triples per relation; batch
    positives of the T triples per batch.
      RANDOM  both modes draw an entity uniformly: 2 batch / n_ent per row.
      TYPED   mode m of a positive of relation p draws uniformly from pool
              2p + m: a batch holds cnt_p batch / T positives of p, so a row
              gets cnt_p batch / (T L) from every pool of length L it is in.
      LCWA    mode 0 accepts candidates of pool 2p only, uniform over it (the
              TYPED share of pool 2p); mode 1 is RANDOM's: batch / n_ent.
    An empty pool draws nothing.  Rejected tries are not discounted (an upper
    estimate: a try that hits a training triple is redrawn from the same
    pool)."""
    n_ent, batch, T = int(n_ent), float(batch), float(max(int(T), 1))
    if kind == L.SKGE_SAMPLER_RANDOM:
        dev = pool_off.device if torch.is_tensor(pool_off) else None
        return torch.full((n_ent,), 2.0 * batch / max(n_ent, 1), dtype=torch.float64, device=dev)
    if kind not in (L.SKGE_SAMPLER_TYPED, L.SKGE_SAMPLER_LCWA):
        raise ValueError("unknown sampler kind %r" % (kind,))
    off = torch.as_tensor(pool_off).long()
    ent = torch.as_tensor(pool_ent, device=off.device).long()
    cnt = torch.as_tensor(rel_counts, device=off.device).double()
    lens = off[1:] - off[:-1]
    if lens.numel() != 2 * cnt.numel():
        raise ValueError("pool_off needs 2 * n_rel + 1 entries for %d relations" % cnt.numel())
    share = cnt.repeat_interleave(2) * (batch / T) / lens.clamp(min=1).double()
    if kind == L.SKGE_SAMPLER_LCWA:
        share[1::2] = 0.0
    load = torch.zeros(n_ent, dtype=torch.float64, device=off.device)
    load.index_add_(0, ent[int(off[0]):int(off[-1])], share.repeat_interleave(lens))
    if kind == L.SKGE_SAMPLER_LCWA:
        load += batch / max(n_ent, 1)
    return load


def packed_count_bound(kg, n_ent, batch, tail=None, sampler=L.SKGE_SAMPLER_RANDOM, n_rel=None):
    """Upper bound on an ENTITY row's per-batch occurrence count in the
    TransE-L1 device loops (the count bounds every 16-bit field of its packed
    sums, csrc/skge_pipeline.hip).  A positive adds at most 3 to each of its s
    and o (skge/transe.py:103-136: s is sp of both pairs and sn of the
    tail-corrupted one) and 1 to each accepted corruption.  The first part
    comes from the training triples: a row that is the subject of c_s of the
    T triples is the subject of at most min(c_s, B) positives of a batch, and
    -- the batch being a uniform sample of the triples (the epoch permutation)
    -- of fewer than the binomial tail mu + 12 sqrt(mu) + 40, mu = c_s B / T,
    as relation_replicas() bounds the relation rows (round 4: the whole-KG
    count alone sent skewed KGs to fp32 sums at every batch past ~3k);
    likewise as object.  The corruptions are uniform draws over the entities
    (skge/sample.py:41-46), bounded by their Poisson tail (lambda + 12
    sqrt(lambda) + 40, lambda = 2 batch / n_ent).  The typed and LCWA samplers
    (sampler=, with n_rel= the model's relation count) draw from pools instead:
    a row's corruptions have the mean corruption_load() gives it -- a
    two-entity pool takes every corruption of its relation -- so the bound is
    per row, max over rows of (3 x its occurrences + the tail of its load):
    the row with the most occurrences need not be the one with the largest
    load.  The applies still check every row's count at run time (ERR_PACKED),
    and device_optim reads that flag after every epoch."""
    T = float(max(int(kg.trip.shape[0]), 1))
    B = float(min(int(batch), int(kg.trip.shape[0])))

    def per_batch(col):
        c = _row_counts(col, n_ent).double()
        mu = c * (B / T)
        return torch.minimum(torch.minimum(c, torch.full_like(c, B)), (tail or _tail)(mu))
    occ = per_batch(kg.trip[:, 0]) + per_batch(kg.trip[:, 1])
    if sampler != L.SKGE_SAMPLER_RANDOM:
        if n_rel is None:
            raise ValueError("the typed and LCWA samplers need the model's relation count")
        off, ent = kg.pools(n_rel)
        load = corruption_load(sampler, off, ent, _row_counts(kg.trip[:, 2], int(n_rel)), n_ent,
                               batch, kg.trip.shape[0])
        cap = float(2 * int(batch))
        rows = 3.0 * torch.clamp(torch.ceil(occ), max=cap) + \
            torch.clamp(torch.ceil((tail or _tail)(load)), max=cap)
        return int(rows.max().item())
    det = 3 * min(int(math.ceil(float(occ.max().item()))), 2 * int(batch))
    lam = 2.0 * batch / max(n_ent, 1)
    corr = min(2 * int(batch), int(math.ceil((tail or _tail)(lam))))
    return det + corr


def _tail8(mu):
    """A tighter tail for the int8x4 entity sums' choice (mu + 8 sqrt(mu) +
    20: a Poisson count passes it with probability < 1e-15): the choice only
    trades atomic bytes, and a count past 127 is still caught by the apply
    (the runner raises, use SKGE_PIPE_E8=0)."""
    return mu + 8.0 * mu ** 0.5 + 20.0


def int8_entity_sums(kg, n_ent, batch, sampler=L.SKGE_SAMPLER_RANDOM, n_rel=None):
    """The pipelined runners' entity sums in 8-bit fields (SKGE_ACC_I8X4: half
    the atomic bytes; the apply checks every count): while every entity's
    per-batch count is <= 127 under _tail8's bound, unless SKGE_PIPE_E8=0."""
    return (packed_count_bound(kg, n_ent, batch, _tail8, sampler=sampler, n_rel=n_rel) <= 127 and
            _os.environ.get("SKGE_PIPE_E8", "1") != "0")


def _tail(mu):
    """Poisson/binomial upper tail used for the random parts of the count
    bounds: mu + 12 sqrt(mu) + 40 (never reached in practice; the applies
    still check every count at run time)."""
    return mu + 12.0 * mu ** 0.5 + 40.0


def relation_replicas(kg, n_rel, batch, max_reps=32, ranks=1):
    """Accumulator copies the packed relation sums need (the two-launch
    runner; the pipelined runner switches to int32x2 sums when this is not 1).
    Positive j adds into copy j mod reps, so a copy of a (union, over `ranks`)
    batch holds per = ranks * ceil(batch / reps) positives; relation p's count
    among them is at most min(per, count_p) and, the batch being a uniform
    sample of the triples, below the binomial tail of mu = per * count_p / T.
    Each positive adds <= 4 to its relation's count.  Returns 0 when even
    max_reps copies cannot keep 4 * bound <= PACKED_MAX."""
    cnt = _row_counts(kg.trip[:, 2], n_rel).double()
    T = float(max(int(kg.trip.shape[0]), 1))
    reps = 1
    while True:
        per = float(int(ranks) * -(-int(batch) // reps))
        bound = torch.minimum(torch.minimum(cnt, torch.full_like(cnt, per)), _tail(cnt * (per / T)))
        if 4.0 * float(bound.max().item()) <= PACKED_MAX:
            return reps
        reps *= 2
        if reps > max_reps:
            return 0


def padded_width(d):
    """Row width the quad-layout runners use for a d % 4 != 0 table: the next
    multiple of 32 floats (whole 128-B lines: config 1's d = 50 -> 64, 256-B
    rows; same box, WN18 SGD: 128.4 M vs 122.1 M triples/s at 52) when that
    costs at most 30% more row bytes, else the next multiple of 4.
    SKGE_PIPE_PAD_TO (A/B) forces the rounding (4: the round-3 width)."""
    force = _os.environ.get("SKGE_PIPE_PAD_TO")
    if force:
        k = max(4, int(force) // 4 * 4)
        return (d + k - 1) // k * k
    d32 = (d + 31) // 32 * 32
    return d32 if d32 <= 1.3 * d else (d + 3) // 4 * 4


class _Runner(object):
    """What the device runners share: the stream, the kg / model / nbatches /
    seed / ntries fields, the epoch key, create-or-raise, run() ordered
    against the caller's stream, and the handle's release.  A subclass builds
    its tables, calls _create with its ABI prefix (skge_<prefix>_create / _run
    / _nlaunches / _destroy, include/skge_hip.h) and overrides synchronize."""

    pipelined = False
    counters = False   # keeps the per-row counters (updateCounts, violations)
    _pad = False
    graph = None       # dp.DataParallelRunner: the torch graph of its captured epoch

    def _setup(self, model, kg, nbatches, seed, ntries, stream, sampler=L.SKGE_SAMPLER_RANDOM,
               negatives=None):
        dev = model.device
        # (n, modes[, rel_range]) of the sampler; anything but (1, [0, 1]) runs
        # the _multi entry points (include/skge_hip.h, skge_negatives_t)
        self.n, self.modes, self._neg = 1, [0, 1], None
        if negatives is not None:
            self.n, self.modes = int(negatives[0]), [int(m) for m in negatives[1]]
            if (self.n, self.modes) != (1, [0, 1]):
                self._neg = negatives_struct(self.n, self.modes, model.sz[2],
                                             negatives[2] if len(negatives) > 2 else None)
        self.K = self.n * len(self.modes)
        # the negative sampler's kind (include/skge_hip.h SKGE_SAMPLER_*) and,
        # for the pool kinds, its view of the kg's type index
        self.sampler = int(sampler)
        self._smp = kg.sampler(self.sampler, model.sz[2]) if self.sampler else None
        self.stream = stream if stream is not None else torch.cuda.Stream(device=dev)
        self.kg, self.model, self.nbatches = kg, model, nbatches
        self.seed, self.ntries = int(seed) & (2 ** 64 - 1), int(ntries)
        self.epoch_key = torch.zeros(1, dtype=torch.int64, device=dev)

    def _total(self, given, dtype):
        """The caller's running total (violations / loss), or the runner's own."""
        return given if given is not None else torch.zeros(1, dtype=dtype,
                                                           device=self.model.device)

    def _hold_state(self, updaters):
        """The graph captures raw pointers to the parameters and to the
        updaters' state (AdaGrad's p2): hold the tensors, so a caller that
        drops its updaters while the runner lives cannot free what the graph
        still reads and writes."""
        self._state_held = [(u.param.data, u.state()) for u in updaters.values()]

    def _hold_captured(self, updaters):
        """The graph captures raw pointers to the model's accumulators and
        counters: hold the tensors, so a later per-batch call that grows the
        model's slot arrays cannot free what this runner still writes; and
        the updaters' state (_hold_state)."""
        m = self.model
        self._captured = [(a.sum, a.cnt, a.touched) for a in m._acc.values()] + \
            [p._counters.copy() for p in m.params.values()]
        self._hold_state(updaters)

    def _epoch_args(self):
        kg = self.kg
        return (L.ptr(kg.trip), kg.T, L.ptr(kg.slots), kg.capacity, int(self.nbatches), self.seed,
                L.ptr(self.epoch_key))

    def _create(self, prefix, *args, create=None):
        """The tables' zero-filled accumulators were made on the current
        stream and the runner works on its own (a reused allocation could
        otherwise hold a freed runner's counts when the first launch runs):
        synchronize, then create or raise with the library's error text."""
        lib = L.lib()
        torch.cuda.current_stream(self.model.device).synchronize()
        name = create or prefix + "_create"
        h = getattr(lib, name)(L.stream_ptr(self.stream), *args)
        if not h:
            raise L.SkgeError("%s: %s" % (name, lib.skge_last_error().decode()))
        self._abi, self.handle = prefix, h
        self.nlaunches = getattr(lib, prefix + "_nlaunches")(h)

    def _create_loop(self, prefix, *args):
        """The pair and logistic loops' create: the (1, [0, 1]) entry point or,
        with any other (n, modes), the _multi one, which takes them as one
        more argument."""
        if self._neg is None:
            self._create(prefix, *args, create=prefix + "_create_ex")
        else:
            self._create(prefix, *args, self._neg, create=prefix + "_create_multi")

    def _pad_in(self):
        pass

    def _pad_out(self):
        pass

    def _launch(self, nepochs):
        L.check(getattr(L.lib(), self._abi + "_run")(self.handle, L.stream_ptr(self.stream),
                                                     int(nepochs)), self._abi + "_run")

    last_order = None   # the last run()'s / profile()'s path code (_order_begin)

    def _order_begin(self):
        """The caller's stream's earlier work (parameters it wrote) before the
        runner's launches, without a wait queued on the runner's stream
        (include/skge_hip.h, skge_run_order_begin).  Keeps the path code in
        last_order: 0 = the caller's stream was idle, nothing enqueued (after
        a synchronize: the fit loop); 1 = the host waited for it."""
        rc = L.lib().skge_run_order_begin(L.stream_ptr(self.stream), L.stream_ptr())
        if rc < 0:
            L.check(rc, "skge_run_order_begin")
        self.last_order = rc

    # True: the ordering after a run is an event wait queued on the caller's
    # stream (run() returns at once; the replays run ~10% slower while that
    # wait is pending, profiles/run_ordering); False: the host waits
    queued_after = _os.environ.get("SKGE_RUN_ORDER_AFTER", "host") == "event"
    last_order_end = None   # skge_run_order_end's path code

    def _order_end(self):
        """The caller's stream's later work after the runner's launches."""
        rc = L.lib().skge_run_order_end(L.stream_ptr(self.stream), L.stream_ptr(),
                                        int(self.queued_after))
        if rc < 0:
            L.check(rc, "skge_run_order_end")
        self.last_order_end = rc

    def run(self, nepochs=1):
        """nepochs epochs on the runner's stream, ordered after the caller's
        stream (parameters it wrote) and before its later work.

        Called from another stream than the runner's, both orderings are paid
        for on the host, so that no cross-stream wait is queued on either
        stream.  Before: when the caller's stream still has work in flight,
        run() BLOCKS until that work has drained (last_order == 1); a caller
        that synchronised first pays nothing (last_order == 0).  After: run()
        BLOCKS until its epochs are done (what the synchronize() that follows
        would wait for); queued_after = True (SKGE_RUN_ORDER_AFTER=event)
        queues an event wait on the caller's stream instead and returns at
        once, at ~0.9 us more per replayed launch.  Called on the runner's
        own stream (the fit loops) run() orders nothing and never blocks.
        The caller's stream must not be capturing."""
        self._order_begin()
        self._pad_in()
        self._launch(nepochs)
        self._pad_out()
        self._order_end()

    def synchronize(self):
        self.stream.synchronize()
        L.check_device_error(L.stream_ptr(self.stream), self._who)

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                self.graph = None   # (it names the handle's buffers)
                self.stream.synchronize()
                getattr(L.lib(), self._abi + "_destroy")(h)
            except Exception:
                pass
            self.handle = None


def negatives_struct(n, modes, n_rel, rel_range=None):
    """skge_negatives_t for Sampler(n, modes); rel_range: the TYPED sampler's
    len(type_index) (None: n_rel, what the other kinds draw a relation from)."""
    modes = [int(m) for m in modes]
    if not 1 <= len(modes) <= 8:
        raise ValueError("modes %r: 1 to 8 entries" % (modes,))
    return L.SkgeNegatives(int(n), len(modes), (L.c_i * 8)(*modes),
                           int(n_rel if rel_range is None else rel_range))


class _PaddedTables(object):
    """The TransE-L1 runners' own accumulators and tables, over zero-padded
    copies of the parameters where d % 4 != 0 (EpochRunner, dp.DataParallelRunner)."""

    def _tables(self, model, updaters, packed, rel_replicas, rel_w32=False, ent_i8=False,
                pad=False):
        """The runner's own accumulators (captured by its graph) and tables
        (pad: over zero-padded copies of the parameters and AdaGrad states)."""
        from .param import Accumulator, table_struct, post_code
        from .base import deterministic
        dev = model.device
        E, R = model.params["E"], model.params["R"]
        if pad:
            class _Padded(object):   # what table_struct reads of a Parameter
                def __init__(self, rows, width):
                    self.rows, self.width = rows, width
                    self.data = torch.zeros((rows, width), dtype=torch.float32, device=dev)
            self._padded = []
            tabs = {}
            for pid, P in (("E", E), ("R", R)):
                u = updaters[pid]
                pp = _Padded(P.rows, self.d_pad)
                st = u.state()
                sp = None if st is None else torch.zeros_like(pp.data)
                self._padded.append((P, pp.data, st, sp))
                tabs[pid] = (u, pp, sp)
            E = tabs["E"][1]
            R = tabs["R"][1]
        mode = L.SKGE_ACC_I16X4 if packed else L.SKGE_ACC_F32
        if not packed and deterministic():   # exact fixed-point sums, one copy
            mode, rel_replicas = L.SKGE_ACC_FX64, 1
        bs = self.kg.T // self.nbatches
        self.accE = Accumulator(E.rows, E.width, dev, slots=4 * bs,
                                mode=L.SKGE_ACC_I8X4 if ent_i8 else mode)
        # relation rows are hot (every positive adds to one of |R| rows): the
        # two-launch runner spreads the adds over `rel_replicas` copies, the
        # pipelined one keeps 32-bit fields (rel_w32)
        self.accR = Accumulator(R.rows, R.width, dev, mode=L.SKGE_ACC_I32X2 if rel_w32 else mode,
                                dense=True, replicas=rel_replicas)
        self.rel_w32 = rel_w32
        self.packed = packed
        if pad:
            def tab(pid, acc):
                u, pp, sp = tabs[pid]
                return table_struct(pp, sp, acc, opt=u.opt, post=post_code(u.param.post),
                                    lr=float(u.learning_rate))
            self.te = tab("E", self.accE)
            self.tr = tab("R", self.accR)
            return
        self.te = updaters["E"].table(self.accE, counters=False)
        self.tr = updaters["R"].table(self.accR, counters=False)

    def _pad_in(self):
        """Padded tables: the model's parameters / states into the copies
        (run()'s _order_begin has ordered them after the caller's stream)."""
        if not self._pad:
            return
        d = self.model.d
        with torch.cuda.stream(self.stream):
            for P, Pp, st, sp in self._padded:
                Pp[:, :d].copy_(P.data)
                if st is not None:
                    sp[:, :d].copy_(st)

    def _pad_out(self):
        """The copies back into the model (run()'s _order_end follows)."""
        if not self._pad:
            return
        d = self.model.d
        with torch.cuda.stream(self.stream):
            for P, Pp, st, sp in self._padded:
                P.data.copy_(Pp[:, :d])
                if st is not None:
                    st.copy_(sp[:, :d])


class _PipeRunner(_Runner):
    """The pipelined runners (skge_pipe_runner_*): their error word and profile()."""

    pipelined = True
    _packed_hint = ""

    def synchronize(self):
        """Read the error word; once it is set the runner is invalid (later
        epochs of this run changed nothing and every later run() is refused)."""
        self.stream.synchronize()
        rc = L.lib().skge_pipe_runner_error(self.handle, L.stream_ptr(self.stream))
        left = "; the tables hold that epoch's partial updates and the runner refuses further runs"
        if rc < 0:
            raise L.SkgeError("%s: %s" % (self._who, L.lib().skge_last_error().decode()))
        if rc & 1:
            raise L.SkgeError("%s: a cross-workgroup wait timed out%s" % (self._who, left))
        if rc & 2:
            raise L.SkgeError("%s: a row's per-batch count exceeded 32767 (packed sums may have "
                              "wrapped)%s%s" % (self._who, left, self._packed_hint))

    def profile(self, trace_launch=None):
        """Pipelined runner only: one eager epoch with HIP events around every
        launch (trains like run(1)).  Returns (us, stats): per-launch durations
        and [entity rows applied, relation rows applied, violating pairs];
        with trace_launch (1..nb1+1) also the per-wave timestamp trace of that
        launch (include/skge_hip.h, skge_pipe_runner_profile)."""
        if not self.pipelined:
            raise ValueError("profile() needs the pipelined runner")
        n = self.nlaunches
        us = np.zeros(n, dtype=np.float32)
        stats = np.zeros((n, 3), dtype=np.int32)
        tr = np.zeros(2 + 6 * self.kg.T + 8 * self.kg.T + 64, dtype=np.uint64) \
            if trace_launch else None
        self._order_begin()
        self._pad_in()
        L.check(L.lib().skge_pipe_runner_profile(
            self.handle, L.stream_ptr(self.stream), us.ctypes.data, stats.ctypes.data, n,
            int(trace_launch or 0), None if tr is None else tr.ctypes.data,
            0 if tr is None else len(tr)), "runner profile")
        self._pad_out()
        self._order_end()
        if trace_launch:
            return us, stats, tr
        return us, stats


class EpochRunner(_PaddedTables, _PipeRunner):
    """Native hipGraph epoch of the TransE device batch loop (keeps no per-row
    counters).

    pipelined: None (auto) uses the one-launch-per-batch pipelined runner
    (skge_pipe_runner_*) whenever it applies (TransE-L1, packed accumulators,
    single-copy relation accumulator) and the two-launch runner otherwise;
    True demands it, False forces the two-launch runner.  Both give identical
    parameters.

    Packed (exact int16x4) entity sums are used for TransE-L1 unless
    force_f32, or unless packed_count_bound() says a row's per-batch count
    could pass 32767 (then fp32 sums: packed=None decides, packed=True
    insists).  The pipelined runner keeps relation sums as int32x2; the
    two-launch runner spreads them over relation_replicas() copies.
    """

    _who = "pipelined runner"
    _packed_hint = "; use force_f32=True"

    def __init__(self, model, updaters, kg, nbatches, seed=0, ntries=100, stream=None,
                 nviol_total=None, force_f32=False, replicas=1, pipelined=None, packed=None,
                 sampler=L.SKGE_SAMPLER_RANDOM):
        from .transe import TransE
        if not isinstance(model, TransE):
            raise NotImplementedError("device_loop supports TransE (the north-star path) only")
        self._setup(model, kg, nbatches, seed, ntries, stream, sampler)
        self.nviol_total = self._total(nviol_total, torch.int32)
        self._hold_state(updaters)
        bs = kg.T // nbatches
        self.hot_rows = 0   # pipelined TransE: entity rows with replicated sums (skewed KGs)
        # d % 4 != 0 (e.g. the reference's d = 50): the packed / pipelined
        # runners work on quads, so they run on zero-padded copies of the
        # tables (width rounded up to 4), copied in and out around every run().
        # A zero column stays zero (TransE-L1: sign(0) = 0 contributions, AdaGrad
        # and the projection leave 0 at 0) and adds nothing to a score or norm,
        # so the padded step is the d-wide step.
        self.d_pad = padded_width(model.d)
        self._pad = (bool(model.l1) and model.d % 4 != 0 and not force_f32 and replicas <= 1
                     and pipelined is not False and packed is not False
                     and _os.environ.get("SKGE_PIPE_PAD", "1") != "0")
        # TransE-L1 sign contributions are small integers: exact packed int16x4
        # sums while every row's per-batch count stays <= 32767 (the applies
        # flag a larger count, checked by synchronize())
        can_pack = bool(model.l1) and (model.d % 4 == 0 or self._pad) and not force_f32
        # (the per-batch count bound of this runner's sampler kind)
        self.count_bound = packed_count_bound(kg, model.E.rows, bs, sampler=self.sampler,
                                              n_rel=model.sz[2]) if can_pack else 0
        auto_packed = packed is None
        if packed is None:
            packed = can_pack and self.count_bound <= PACKED_MAX
        elif packed and not can_pack:
            raise ValueError("packed sums need TransE-L1, d % 4 == 0 and no force_f32")
        packed = bool(packed)
        # the two-launch runner's packed relation sums: hot relations spread
        # over accumulator copies (0: not even 32 copies suffice)
        rel_reps = relation_replicas(kg, model.R.rows, bs) if packed else 1
        can_pipe = packed and replicas <= 1 and pipelined is not False
        if pipelined and not can_pipe:
            raise ValueError("pipelined runner needs TransE-L1, d % 4 == 0, packed sums "
                             "and replicas == 1")
        lib = L.lib()
        if can_pipe:
            # relation sums in 16-bit fields while a relation's per-batch count
            # fits them (faster: half the atomics), else int32x2; entity sums in
            # 8-bit fields while every entity's per-batch count is <= 127
            e8 = int8_entity_sums(kg, model.E.rows, bs, self.sampler, model.sz[2])
            self._tables(model, updaters, packed, 1, rel_w32=rel_reps != 1, ent_i8=e8,
                         pad=self._pad)
            self.ent_i8 = e8
            wd = self.d_pad if self._pad else model.d
            try:
                if pipelined or self._pipe_fits(wd):   # (auto mode: only if it fits)
                    self._create("skge_pipe_runner", self.te, self.tr, wd, *self._epoch_args(),
                                 float(model.margin), self.ntries, L.ptr(self.nviol_total), 0,
                                 self._smp, create="skge_pipe_runner_create_smp")
                    self.hot_rows = lib.skge_pipe_runner_hot_rows(self.handle)
                    self.kernel = ("k_pipe_batch",
                                   "k_pipe_fused")[lib.skge_pipe_runner_kernel(self.handle)]
                    return
            except L.SkgeError as e:
                if not (pipelined is None and "allocation" in str(e)):
                    raise
            # auto mode: it does not fit, or ran out of device memory -> two-launch runner
            self.accE = self.accR = self.te = self.tr = None
            torch.cuda.empty_cache()
        self.pipelined = False
        self.kernel = "k_transe_sample_grad"
        if self._pad:   # the two-launch runner takes any d: no padded copies
            self._pad = False
            packed = packed and model.d % 4 == 0
            rel_reps = relation_replicas(kg, model.R.rows, bs) if packed else 1
        if packed and rel_reps == 0:
            if not auto_packed:
                raise ValueError("packed sums: a relation's per-batch count exceeds what 32 "
                                 "accumulator copies hold; use packed=None or force_f32=True")
            packed = False
        self._tables(model, updaters, packed, max(int(replicas), rel_reps) if packed else replicas)
        args = (int(bool(model.l1)), self.te, self.tr, model.d) + self._epoch_args() + \
            (float(model.margin), self.ntries, None, L.ptr(self.nviol_total))
        self._create("skge_runner", *(args + (self._smp,)), create="skge_runner_create_smp")

    def _pipe_fits(self, d):
        """Auto mode: the pipelined runner only if what it allocates beside the
        tables just built (skge_pipe_runner_plan's device_bytes -- the C side's
        own rule and sizes, hot-row buffers at their upper bound) fits in the
        free device memory with room to spare: 64 MB for k_pipe_fused, 256 MB
        for k_pipe_batch, and a tenth of what is free."""
        dev = self.model.device
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        plan = L.SkgePipePlan()
        L.check(L.lib().skge_pipe_runner_plan(self.te, self.tr, int(d), self.kg.T,
                                              int(self.nbatches), 0, 0, plan), "pipelined plan")
        slack = (64 << 20) if plan.kernel == 1 else (256 << 20)
        return plan.device_bytes + slack < torch.cuda.mem_get_info(dev)[0] * 0.9

    def synchronize(self):
        if self.pipelined:
            return _PipeRunner.synchronize(self)
        self.stream.synchronize()
        L.check_device_error(L.stream_ptr(self.stream), "epoch runner")


class HolePipeRunner(_PipeRunner):
    """Pipelined HolE device loop (skge_hole_pipe_runner_create,
    csrc/skge_pipeline.hip k_hole_pipe): the TransE pipelined runner's launch
    structure -- launch g scores batch b (both pairs of a positive per wave,
    k_hole_pos's arithmetic) while batch b-1's rows are applied beside it --
    with fp32 sums.  Same pairs as PairLoopRunner's HolE path (the same
    device draws); parameters equal to fp32 rounding (float atomics add in
    any order).  Needs d % 4 == 0, 4 <= d <= 256.  Keeps no per-row
    counters."""

    _who = "pipelined HolE runner"

    def __init__(self, model, updaters, kg, nbatches, seed=0, ntries=100, stream=None,
                 nviol_total=None, sampler=L.SKGE_SAMPLER_RANDOM):
        from .hole import HolE
        from .param import Accumulator
        if not isinstance(model, HolE):
            raise TypeError("HolePipeRunner trains HolE")
        dev = model.device
        self._setup(model, kg, nbatches, seed, ntries, stream, sampler)
        self.nviol_total = self._total(nviol_total, torch.int32)
        self._hold_state(updaters)
        E, R = model.params["E"], model.params["R"]
        bs = kg.T // nbatches
        self.accE = Accumulator(E.rows, E.width, dev, slots=4 * bs)
        self.accR = Accumulator(R.rows, R.width, dev, dense=True)
        reg = model._reg("pairwise")
        self.te = updaters["E"].table(self.accE, counters=False, rin=reg["E"][0],
                                      rout=reg["E"][1], fixed_div=reg["E"][2])
        self.tr = updaters["R"].table(self.accR, counters=False, rin=reg["R"][0],
                                      rout=reg["R"][1], fixed_div=reg["R"][2])
        args = (model._af_code(), self.te, self.tr, model.d) + self._epoch_args() + \
            (float(model.margin), self.ntries, L.ptr(self.nviol_total))
        self._create("skge_pipe_runner", *(args + (self._smp,)),
                     create="skge_hole_pipe_runner_create_smp")
        # hub rows (pair form, skewed KGs)
        self.hot_rows = L.lib().skge_pipe_runner_hot_rows(self.handle)

    @staticmethod
    def eligible(model):
        from .hole import HolE
        d = model.d
        return isinstance(model, HolE) and d % 4 == 0 and 4 <= d <= 256


def batch_sizes(T, nbatches):
    """Batch sizes of StochasticTrainer._optim's np.split (skge/base.py:1246-1268)."""
    bs = T // nbatches
    return [min(bs, T - s0) for s0 in range(0, T, bs)]


class PairLoopRunner(_Runner):
    """Native hipGraph epoch of the device pair loop for any model
    (skge_pair_runner_*, csrc/skge_pairloop.hip): the epoch's permutation and
    negatives drawn on the device (the same keyed draws as EpochRunner), every
    batch's explicit pairs built once per epoch, then per batch one
    skge_pair_step -- the kernels of the explicit-pair path, so a device epoch
    trains like feeding those pairs to model._pairwise_step.  HolE and RESCAL
    (MFMA) run both pairs of a positive together instead (k_hole_pos,
    k_rescal_pos_scatter: the same pairs, contributions and counts; the env
    switches SKGE_HOLE_PAIRS=1 / SKGE_RESCAL_PAIRS=1 select the explicit
    pairs).  The per-row counters (updateCounts, TransE violations) are kept
    as on that path."""

    counters = True    # updateCounts / TransE violations, as on the per-batch path
    _who = "pair-loop runner"

    def __init__(self, model, updaters, kg, nbatches, seed=0, ntries=100, stream=None,
                 nviol_total=None, sampler=L.SKGE_SAMPLER_RANDOM, negatives=None):
        self._setup(model, kg, nbatches, seed, ntries, stream, sampler, negatives)
        self.nviol_total = self._total(nviol_total, torch.int32)
        P = self.K * max(batch_sizes(kg.T, nbatches))
        self.te, self.tr = model._tables("pairwise", updaters, slots=model._pair_slots(P))
        self._hold_captured(updaters)
        self._create_loop("skge_pair_runner", model._kernel_model(), model._af_code(), self.te,
                          self.tr, model.d, *self._epoch_args(), float(model.margin), self.ntries,
                          L.ptr(self.nviol_total), self._smp)
        # how the captured batches update the entity rows: "scatter" (sums by
        # the gradient launch, then an apply launch) or "rows" (RESCAL's
        # row-grouped apply, k_rescal_fold)
        self.entity_apply = ("scatter", "rows")[L.lib().skge_pair_runner_entity_apply(self.handle)]


def _require_logistic_model(model):
    if model._kernel_model() == L.SKGE_ROTATE:
        raise ValueError("RotatE has no logistic trainer: its scores are <= 0, so the loss needs "
                         "a gamma offset; train it with PairwiseStochasticTrainer")
    if model._kernel_model() not in (L.SKGE_HOLE, L.SKGE_RESCAL, L.SKGE_DISTMULT,
                                     L.SKGE_COMPLEX):
        raise NotImplementedError("%s has no logistic loss in the reference"
                                  % type(model).__name__)


class LogisticLoopRunner(_Runner):
    """Native hipGraph epoch of the device logistic loop for HolE and RESCAL
    (skge_triple_runner_*, csrc/skge_tripleloop.hip): one epoch of
    StochasticTrainer with RandomModeSampler(1, [0, 1]) (skge/base.py:
    1242-1316) -- the epoch's permutation and negatives drawn on the device
    (the same keyed draws as the other runners), every batch's labelled
    triples built once per epoch in the order ``xys += samplef(xys)`` gives
    (positives, then each positive's s- and o-corruption; a negative not
    found in ntries draws is a skipped triple), then per batch one
    skge_triple_step -- the kernels of the per-batch path, so a device epoch
    trains like feeding those triples to model._logistic_step.  HolE in the
    wave FFT's range scores a positive and both corruptions in one wave
    instead (k_hole_logistic_pos: the same triples, contributions and counts;
    SKGE_HOLE_TRIPLES=1 selects the explicit triples).  The epoch's loss is
    added into ``loss_total``; the per-row counters (updateCounts) are kept
    as on the per-batch path."""

    counters = True
    _who = "logistic-loop runner"

    def __init__(self, model, updaters, kg, nbatches, seed=0, ntries=100, stream=None,
                 loss_total=None, sampler=L.SKGE_SAMPLER_RANDOM, negatives=None):
        _require_logistic_model(model)
        self._setup(model, kg, nbatches, seed, ntries, stream, sampler, negatives)
        self.loss_total = self._total(loss_total, torch.float32)
        T3 = (1 + self.K) * max(batch_sizes(kg.T, nbatches))
        self.te, self.tr = model._tables("logistic", updaters, slots=model._triple_slots(T3))
        self._hold_captured(updaters)
        self._create_loop("skge_triple_runner", model._kernel_model(), self.te, self.tr, model.d,
                          *self._epoch_args(), self.ntries, L.ptr(self.loss_total), self._smp)


class SadvLoopRunner(_Runner):
    """Native hipGraph epoch of the self-adversarial loss for TransE and RotatE
    (skge_sadv_runner_create, csrc/skge_pairloop.hip): the epoch's permutation
    and its K = n * len(modes) negatives per positive drawn on the device (the
    _multi draw of the other loops, so (n, modes) may be anything with K <= 64,
    (1, [0, 1]) included as K = 2), then per batch one k_sadv_pos launch
    straight on the records -- scores, softmax weights, coefficients,
    contributions -- and one apply of both tables.  A device epoch trains like
    feeding epoch_records_multi's records batch by batch to model._sadv_step.
    The epoch's loss is added into ``loss_total``; updateCounts are kept as on
    the per-batch path."""

    counters = True
    _who = "sadv-loop runner"

    def __init__(self, model, updaters, kg, nbatches, seed=0, ntries=100, stream=None,
                 loss_total=None, sampler=L.SKGE_SAMPLER_RANDOM, negatives=None):
        model._require_sadv()
        self._setup(model, kg, nbatches, seed, ntries, stream, sampler, negatives)
        if self._neg is None:
            self._neg = negatives_struct(1, [0, 1], model.sz[2])
        self.loss_total = self._total(loss_total, torch.float32)
        B = max(batch_sizes(kg.T, nbatches))
        self.te, self.tr = model._tables("sadv", updaters,
                                         slots=((2 + self.K) * B, (1 + self.K) * B))
        self._hold_captured(updaters)
        self._create("skge_pair_runner", model._kernel_model(), self.te, self.tr, model.d,
                     *self._epoch_args(), float(model.gamma), float(model.alpha), self.ntries,
                     L.ptr(self.loss_total), self._smp, self._neg,
                     create="skge_sadv_runner_create")


def _loss_loop_optim(runner_cls, trainer, xs, ntries, sampler, negatives):
    """The fit of a trainer whose device loop adds the epoch's loss into
    trainer._loss_dev: the runner, then _fit_epochs."""
    model = trainer.model
    dev = model.device
    if trainer._loss_dev is None:
        trainer._loss_dev = torch.zeros(1, dtype=torch.float32, device=dev)
    kg = DeviceKG(xs, dev)
    runner = runner_cls(model, trainer._updaters, kg, trainer.nbatches, seed=trainer.seed,
                        ntries=trainer.ntries if ntries is None else ntries,
                        loss_total=trainer._loss_dev, sampler=sampler, negatives=negatives)
    trainer.batch_size = kg.T // trainer.nbatches
    _fit_epochs(trainer, runner)


def sadv_device_optim(trainer, xs, ntries=None, sampler=L.SKGE_SAMPLER_RANDOM, negatives=None):
    """SelfAdversarialTrainer.fit with device_loop=True: per epoch _pre_epoch,
    one graph replay, the runner's error word, then the post_epoch callbacks
    (which read the epoch's loss through trainer.loss)."""
    _loss_loop_optim(SadvLoopRunner, trainer, xs, ntries, sampler, negatives)


def _fit_epochs(trainer, runner):
    """The device fits' epoch loop: per epoch _pre_epoch, one graph replay, the
    runner's error word (read before the post_epoch callbacks, so no callback
    ever sees parameters from a failed epoch), then the callbacks."""
    trainer._runner = runner
    with torch.cuda.stream(runner.stream):
        for trainer.epoch in range(1, trainer.max_epochs + 1):
            trainer._pre_epoch()
            trainer.epoch_start = timeit.default_timer()
            runner.run(1)
            runner.synchronize()   # raises on the epoch's error bits
            for f in trainer.post_epoch:
                if not f(trainer):
                    break


def logistic_device_optim(trainer, xs, ntries=None, sampler=L.SKGE_SAMPLER_RANDOM,
                          negatives=None):
    """StochasticTrainer.fit with device_loop=True: per epoch _pre_epoch, one
    graph replay, the runner's error word, then the post_epoch callbacks (which
    read the epoch's loss through trainer.loss as on the per-batch path).
    sampler: the kind device_sampler_args reported; negatives: its (n, modes,
    rel_range) (None: (1, [0, 1]))."""
    _loss_loop_optim(LogisticLoopRunner, trainer, xs, ntries, sampler, negatives)


def epoch_records(kg, n_ent, seed, epoch_key, ntries=100, stream=None,
                  sampler=L.SKGE_SAMPLER_RANDOM, n_rel=None):
    """The epoch's positives and draws as the device loops make them:
    (rec [T, 4] = (s, o, p, s' or -1), rec_n1 [T] = o' or -1) on the device.
    sampler: the kind (the typed and LCWA kinds need n_rel, the model's
    relation count)."""
    dev = kg.trip.device
    rec = torch.empty((kg.T, 4), dtype=torch.int32, device=dev)
    rec_n1 = torch.empty(kg.T, dtype=torch.int32, device=dev)
    ek = torch.tensor([int(epoch_key)], dtype=torch.int64, device=dev)
    L.check(L.lib().skge_epoch_sample_ex(L.stream_ptr(stream), L.ptr(kg.trip), kg.T,
                                         L.ptr(kg.slots), kg.capacity, int(n_ent),
                                         int(seed) & (2 ** 64 - 1), L.ptr(ek), int(ntries),
                                         L.ptr(rec), L.ptr(rec_n1), kg.sampler(sampler, n_rel)),
            "epoch sample")
    return rec, rec_n1


def epoch_records_multi(kg, n_ent, n_rel, seed, epoch_key, n, modes, ntries=100, stream=None,
                        sampler=L.SKGE_SAMPLER_RANDOM, rel_range=None):
    """The epoch's positives and draws as the _multi device loops make them,
    for Sampler(n, modes): (pos [T, 3] = (s, o, p), neg [T, K]) on the device,
    K = n * len(modes), slot k = rep * len(modes) + mi holding the id that
    replaces position modes[mi] (a relation for mode 2), or -1.  rel_range: the
    TYPED sampler's len(type_index) (None: n_rel)."""
    dev = kg.trip.device
    negs = negatives_struct(n, modes, n_rel, rel_range)
    K = max(int(n) * len(modes), 1)
    pos = torch.empty((kg.T, 3), dtype=torch.int32, device=dev)
    neg = torch.empty((kg.T, K), dtype=torch.int32, device=dev)
    ek = torch.tensor([int(epoch_key)], dtype=torch.int64, device=dev)
    L.check(L.lib().skge_epoch_sample_multi(L.stream_ptr(stream), L.ptr(kg.trip), kg.T,
                                            L.ptr(kg.slots), kg.capacity, int(n_ent), int(n_rel),
                                            int(seed) & (2 ** 64 - 1), L.ptr(ek), int(ntries),
                                            L.ptr(pos), L.ptr(neg), kg.sampler(sampler, n_rel),
                                            negs), "epoch sample (multi)")
    return pos, neg


def make_runner(model, updaters, kg, nbatches, seed=0, ntries=100, nviol_total=None,
                runner="auto", sampler=L.SKGE_SAMPLER_RANDOM, negatives=None):
    """runner: 'auto' (TransE -> EpochRunner, the fused sampler/score runners;
    HolE -> HolePipeRunner where it applies, RESCAL -> PairLoopRunner),
    'epoch', 'hole_pipe', 'pairs' or 'pipe'.  sampler: the kind of negatives
    (SKGE_SAMPLER_*); under 'auto' (and by the names 'epoch' / 'hole_pipe')
    the fused and pipelined runners draw RANDOM only, so the typed and LCWA
    kinds run the pair loop for every model.  'pipe' is the model's throughput
    runner with whatever kind the sampler is: TransE -> EpochRunner(sampler=),
    an eligible HolE -> HolePipeRunner(sampler=); anything else (RESCAL, a
    HolE outside the runner's widths, n or modes other than (1, [0, 1])) is
    refused and needs 'pairs'.  negatives: the
    sampler's (n, modes, rel_range) (None: (1, [0, 1])); the fused and
    pipelined runners draw (1, [0, 1]) only, so any other runs the pair loop."""
    from .transe import TransE
    from .base import deterministic
    from .distmult import DistMult
    from .rotate import RotatE
    if isinstance(model, (DistMult, RotatE)) and runner in ("pipe", "epoch", "hole_pipe"):
        # DistMult / ComplEx / RotatE train on the pair loop only (k_diag_pos,
        # k_rot_pos)
        raise ValueError("device runner %r is TransE's or HolE's; %s needs 'pairs' (or 'auto')"
                         % (runner, type(model).__name__))
    if runner == "pipe":
        if negatives is not None and (int(negatives[0]), list(negatives[1])) != (1, [0, 1]):
            raise ValueError("device runner 'pipe' draws one negative per mode of [0, 1] only; "
                             "n = %r, modes = %r need 'pairs' (or 'auto')"
                             % (negatives[0], list(negatives[1])))
        if isinstance(model, TransE):
            return EpochRunner(model, updaters, kg, nbatches, seed=seed, ntries=ntries,
                               nviol_total=nviol_total, sampler=sampler)
        if HolePipeRunner.eligible(model) and not deterministic():
            return HolePipeRunner(model, updaters, kg, nbatches, seed=seed, ntries=ntries,
                                  nviol_total=nviol_total, sampler=sampler)
        raise ValueError("device runner 'pipe' is TransE's or HolE's (d %% 4 == 0, 4 <= d <= 256, "
                         "not deterministic) pipelined runner; %s needs 'pairs' (or 'auto')"
                         % type(model).__name__)
    if sampler != L.SKGE_SAMPLER_RANDOM:
        if runner not in ("auto", "pairs"):
            raise ValueError("device runner %r draws RandomModeSampler negatives only; the typed "
                             "and LCWA samplers need 'pairs' (or 'auto')" % (runner,))
        runner = "pairs"
    if negatives is not None and (int(negatives[0]), list(negatives[1])) != (1, [0, 1]):
        if runner not in ("auto", "pairs"):
            raise ValueError("device runner %r draws one negative per mode of [0, 1] only; "
                             "n = %r, modes = %r need 'pairs' (or 'auto')"
                             % (runner, negatives[0], list(negatives[1])))
        runner = "pairs"
    if runner == "auto":
        runner = "epoch" if isinstance(model, TransE) else \
            ("hole_pipe" if HolePipeRunner.eligible(model) and not deterministic() else "pairs")
    if runner == "hole_pipe":
        return HolePipeRunner(model, updaters, kg, nbatches, seed=seed, ntries=ntries,
                              nviol_total=nviol_total)
    if runner == "epoch":
        return EpochRunner(model, updaters, kg, nbatches, seed=seed, ntries=ntries,
                           nviol_total=nviol_total)
    if runner == "pairs":
        return PairLoopRunner(model, updaters, kg, nbatches, seed=seed, ntries=ntries,
                              nviol_total=nviol_total, sampler=sampler, negatives=negatives)
    raise ValueError("unknown device runner %r" % (runner,))


class SamplerArgs(tuple):
    """device_sampler_args' result: unpacks as (eligible, ntries, reason), as
    it always has; ``kind`` is the device sampler's kind (SKGE_SAMPLER_*),
    ``n`` and ``modes`` the sampler's, ``rel_range`` the range a mode 2 draws
    its relation from (None: the model's relation count), and ``negatives``
    the three as the runners take them."""

    def __new__(cls, eligible, ntries, reason, kind=L.SKGE_SAMPLER_RANDOM, n=1, modes=(0, 1),
                rel_range=None):
        self = super(SamplerArgs, cls).__new__(cls, (eligible, ntries, reason))
        self.kind, self.n, self.modes, self.rel_range = kind, n, list(modes), rel_range
        return self

    @property
    def negatives(self):
        return (self.n, self.modes, self.rel_range)


MAX_SLOTS = 64   # K = n * len(modes) slots per positive (skge_negatives_t)


def _negatives_reason(name, n, modes):
    """Why Sampler(n, modes) is outside what the device loops draw ('': it is
    inside): n >= 1, 1 to 8 modes from {0, 1, 2}, n * len(modes) <= 64."""
    try:
        modes = list(modes)
        ok = isinstance(n, (int, np.integer)) and n >= 1 and 1 <= len(modes) <= 8 and \
            all(isinstance(m, (int, np.integer)) and 0 <= m <= 2 for m in modes)
    except TypeError:
        ok = False
    if not ok:
        return ("%s(n=%r, modes=%r): the device loops draw n >= 1 negatives over 1 to 8 modes "
                "from {0, 1, 2}" % (name, n, modes))
    if n * len(modes) > MAX_SLOTS:
        return ("%s(n=%r, modes=%r): %d negatives per positive, the device loops draw at most %d"
                % (name, n, modes, n * len(modes), MAX_SLOTS))
    return ""


def _pools_match(index, xs3):
    """Whether a CorruptedSampler's type_index lists, per relation and side,
    exactly the entities type_index(xs) does, each once (a repeated entry
    would be drawn more often than the device's unique pools draw it)."""
    from .sample import type_index
    want = type_index(xs3)
    try:
        if set(index.keys()) != set(want.keys()):
            return False
        for k, sides in want.items():
            for side in (0, 1):
                got = [int(v) for v in index[k][side]]
                if len(got) != len(sides[side]) or set(got) != set(sides[side]):
                    return False
    except (AttributeError, KeyError, TypeError, ValueError):
        return False
    return True


def device_sampler_args(trainer, xs, ys):
    """(eligible, ntries, reason), with the device sampler's kind as the
    result's ``kind``: whether a trainer's fit with device_loop=True may run
    the device loop, whose samplers draw what
      RandomModeSampler(1, [0, 1], xs, sz)               (kind RANDOM),
      CorruptedSampler(1, xs, type_index(xs), modes=[0, 1])  (kind TYPED) or
      LCWASampler(1, [0, 1], xs, sz)                     (kind LCWA)
    would (skge/sample.py:28-120, skge/base.py:422-428) -- or, for a trainer
    built with device_negatives=True, what the three classes draw with any
    n >= 1 over 1 to 8 modes from {0, 1, 2} (mode 2 corrupts the relation),
    n * len(modes) <= 64, reported as the result's ``n``, ``modes`` and
    ``rel_range``.  Needed: every y is +1, samplef is such a sampler's own
    sample method, n == 1 and modes == [0, 1] (without device_negatives),
    sizes equal to the model's, and a sampler that rejects against the
    same training triples the device loop does (its xs == the fit's xs); the
    typed sampler's type_index must be the one of xs and the LCWA sampler's
    counts those of xs.  samplef None is the reference's labelled-negatives
    branch (skge/base.py:1350-1357: positives paired with the given y != 1
    rows; with none it builds no pairs), which the device loop does not
    mirror."""
    if ys is not None and not np.all(np.asarray(ys) == 1):
        return SamplerArgs(False, trainer.ntries, "labelled negatives (y != 1)")
    f = trainer.samplef
    if f is None:
        return SamplerArgs(False, trainer.ntries,
                           "samplef is None (the labelled-negatives branch, "
                           "skge/base.py:1350-1357); pass samplef="
                           "RandomModeSampler(1, [0, 1], xs, sz).sample")
    from .sample import CorruptedSampler, LCWASampler, RandomModeSampler, Sampler
    smp = getattr(f, "__self__", None)
    cls = next((c for c in (LCWASampler, CorruptedSampler, RandomModeSampler)
                if isinstance(smp, c)), None)   # LCWASampler is a RandomModeSampler: first
    if cls is None or getattr(f, "__func__", None) is not Sampler.sample:
        return SamplerArgs(False, trainer.ntries, "samplef is not RandomModeSampler.sample (nor "
                           "CorruptedSampler's or LCWASampler's)")
    name = cls.__name__
    kind = {RandomModeSampler: L.SKGE_SAMPLER_RANDOM, CorruptedSampler: L.SKGE_SAMPLER_TYPED,
            LCWASampler: L.SKGE_SAMPLER_LCWA}[cls]
    if type(smp)._sample is not cls._sample:
        return SamplerArgs(False, trainer.ntries, "%s._sample is overridden" % name)
    if not getattr(trainer, "device_negatives", False):
        # as it always was: one negative per mode of [0, 1], or the per-batch path
        if smp.n != 1 or list(smp.modes) != [0, 1]:
            return SamplerArgs(False, trainer.ntries, "%s(n=%r, modes=%r) is not (1, [0, 1]) "
                               "(device_negatives=True draws n negatives over modes from "
                               "{0, 1, 2} on the device)" % (name, smp.n, smp.modes))
    why = _negatives_reason(name, smp.n, smp.modes)
    if why:
        return SamplerArgs(False, trainer.ntries, why)
    n, modes = int(smp.n), [int(m) for m in smp.modes]
    n_ent, n_rel = trainer.model.E.rows, int(trainer.model.sz[2])
    if cls is not CorruptedSampler and (
            tuple(smp.sz[:2]) != (n_ent, n_ent) or (2 in modes and smp.sz[2] != n_rel)):
        return SamplerArgs(False, trainer.ntries,
                           "sampler sizes %r differ from the model's" % (smp.sz,))
    xs3 = np.asarray(xs, dtype=np.int64).reshape(-1, 3).tolist()
    fit_set = set(tuple(int(v) for v in x) for x in xs3)
    if fit_set != smp.xs:
        return SamplerArgs(False, trainer.ntries,
                           "the sampler's rejection set differs from the fit's "
                           "triples (the device sampler rejects against xs)")
    if cls is CorruptedSampler and not _pools_match(smp.type_index, xs3):
        return SamplerArgs(False, trainer.ntries,
                           "CorruptedSampler.type_index differs from type_index(xs) (the device "
                           "sampler draws from the fit's triples' type index)")
    if cls is LCWASampler and set(k for k, c in smp.counts.items() if c > 0) != \
            set((s, p) for s, _, p in fit_set):
        return SamplerArgs(False, trainer.ntries,
                           "LCWASampler.counts differ from the fit's triples' (s, p) counts")
    # a typed mode 2 draws randint(len(type_index)) as a relation id
    # (skge/sample.py:80); type_index is the one of xs, so it is <= n_rel
    rel_range = len(smp.type_index) if cls is CorruptedSampler and 2 in modes else None
    return SamplerArgs(True, smp.ntries, "", kind, n, modes, rel_range)


def device_optim(trainer, xs, ntries=None, sampler=L.SKGE_SAMPLER_RANDOM, negatives=None):
    """PairwiseStochasticTrainer.fit with device_loop=True (sampler: the kind
    device_sampler_args reported; negatives: its (n, modes, rel_range), None:
    (1, [0, 1])).  The runner's
    error word (packed-sum overflow, cross-workgroup wait timeout) is read
    after every epoch, before the post_epoch callbacks, so no callback ever
    sees parameters from a failed epoch."""
    model = trainer.model
    dev = model.device
    if trainer._nviol_dev is None:
        trainer._nviol_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    kg = DeviceKG(xs, dev)
    which = trainer.device_runner
    if which == "auto" and trainer.file_gradients is not None:
        # file_grad's #(violations) / #(updates) columns need the per-row
        # counters, which only the pair loop keeps (file_grad=None: the
        # fused / pipelined runners)
        which = "pairs"
    runner = make_runner(model, trainer._updaters, kg, trainer.nbatches, seed=trainer.seed,
                         ntries=trainer.ntries if ntries is None else ntries,
                         nviol_total=trainer._nviol_dev, runner=which, sampler=sampler,
                         negatives=negatives)
    _fit_epochs(trainer, runner)
