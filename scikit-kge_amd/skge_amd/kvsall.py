"""KvsAll (1-N) training of DistMult and ComplEx.

Every distinct (s, p, ?) and (?, p, o) of the training set is a *query*; a
batch of queries is scored against every entity and takes binary
cross-entropy against the multi-hot vector of its known answers
(skge_kvsall_grad / skge_kvsall_step, csrc/skge_kvsall.hip).  There is no
sampler: `KvsAllQueries` builds the queries and their answers once, on the
host, and `KvsAllTrainer` walks them in StochasticTrainer's shuffled batches.

`OneNQueries` and `OneNTrainer` are what this regime shares with 1vsAll
(onevsall.py): a regime is a queries class, two model methods and a few words.
"""
import numpy as np
import torch

from .base import StochasticTrainer, deterministic

MAX_BATCH = 4096          # skge_kvsall_* / skge_onevsall_*: queries per batch
_DIRECTIONS = {"tail": 0, "head": 1}


class OneNQueries(object):
    """Queries (anchor[i], rel[i], dir[i], ...) of a set of triples (s, o, p):
    dir 0 is (anchor, rel, ?), dir 1 is (?, rel, anchor).  `_FIELDS` names the
    arrays a class holds: its constructor's arguments, in that order, before
    n_ent and n_rel.  Arrays are int32 NumPy on the host; `.to` returns a copy
    holding device tensors."""

    _FIELDS = ()

    def __init__(self, arrays, n_ent, n_rel):
        for name, a in zip(self._FIELDS, arrays):
            setattr(self, name, a)
        self.n_ent, self.n_rel = int(n_ent), int(n_rel)

    @classmethod
    def _parse(cls, xs, sz, directions):
        """The triples [T, 3] int64, n_ent, n_rel and the direction codes in
        the order given (each once), checked."""
        x = np.asarray(xs, dtype=np.int64).reshape(-1, 3)
        n_ent, n_rel = int(sz[0]), int(sz[2])
        dirs = []
        for name in directions:
            if name not in _DIRECTIONS:
                raise ValueError("%s: direction %r; 'tail' and 'head' are served"
                                 % (cls.__name__, name))
            if _DIRECTIONS[name] not in dirs:
                dirs.append(_DIRECTIONS[name])
        if not dirs:
            raise ValueError("%s: no direction given; 'tail' and 'head' are served" % cls.__name__)
        if len(x) and (x.min() < 0 or x[:, :2].max() >= n_ent or x[:, 2].max() >= n_rel):
            raise ValueError("%s: a triple names a row outside sz = %r" % (cls.__name__, tuple(sz)))
        return x, n_ent, n_rel, dirs

    def _arrays(self):
        return tuple(getattr(self, name) for name in self._FIELDS)

    def __len__(self):
        return int(self.anchor.shape[0])

    @property
    def device(self):
        return self.anchor.device if torch.is_tensor(self.anchor) else None

    def to(self, device):
        """A copy with the arrays on `device`."""
        host = self.numpy()
        return type(self)(*[torch.as_tensor(a, device=device) for a in host._arrays()],
                          self.n_ent, self.n_rel)

    def numpy(self):
        if self.device is None:
            return self
        return type(self)(*[a.cpu().numpy() for a in self._arrays()], self.n_ent, self.n_rel)

    def batch(self, ids):
        """The queries `ids`, in that order, on the same device.  On a device
        it is an index gather: no device-to-host read."""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if self.device is None:
            return type(self)(*[a[ids] for a in self._arrays()], self.n_ent, self.n_rel)
        i = torch.as_tensor(ids, device=self.device)
        return type(self)(*[a[i].contiguous() for a in self._arrays()], self.n_ent, self.n_rel)


class KvsAllQueries(OneNQueries):
    """The distinct queries of a set of triples (s, o, p) and their answers, as
    a CSR: query i is (anchor[i], rel[i], dir[i]) -- dir 0 asks for the tails
    of (anchor, rel, ?), dir 1 for the heads of (?, rel, anchor) -- and its
    answers are ans[off[i]:off[i + 1]], sorted and distinct.  The queries are
    sorted by (dir, rel, anchor).  Arrays are int32 NumPy on the host; `.to`
    returns a copy holding device tensors."""

    _FIELDS = ("anchor", "rel", "dir", "off", "ans")

    def __init__(self, anchor, rel, dir, off, ans, n_ent, n_rel):
        super(KvsAllQueries, self).__init__((anchor, rel, dir, off, ans), n_ent, n_rel)
        self._off_host = off if isinstance(off, np.ndarray) else None

    @classmethod
    def from_triples(cls, xs, sz, directions=("tail", "head")):
        x, n_ent, n_rel, dirs = cls._parse(xs, sz, directions)
        rows = []
        for t in sorted(dirs):   # (dir, rel, anchor, answer)
            a, e = (x[:, 0], x[:, 1]) if t == 0 else (x[:, 1], x[:, 0])
            rows.append(np.stack([np.full(len(x), t, dtype=np.int64), x[:, 2], a, e], axis=1))
        rows = np.unique(np.concatenate(rows, axis=0), axis=0)   # sorted rows, duplicates dropped
        if len(rows) == 0:
            z = np.zeros(0, dtype=np.int32)
            return cls(z, z.copy(), z.copy(), np.zeros(1, dtype=np.int32), z.copy(), n_ent, n_rel)
        first = np.ones(len(rows), dtype=bool)
        first[1:] = np.any(rows[1:, :3] != rows[:-1, :3], axis=1)
        start = np.flatnonzero(first)
        off = np.append(start, len(rows)).astype(np.int32)
        q = rows[start]
        return cls(q[:, 2].astype(np.int32), q[:, 1].astype(np.int32), q[:, 0].astype(np.int32),
                   off, rows[:, 3].astype(np.int32), n_ent, n_rel)

    def to(self, device):
        """A copy with the five arrays on `device` (the offsets stay on the host
        too: a batch's answer count is known without a device read)."""
        host = self.numpy()
        out = super(KvsAllQueries, host).to(device)
        out._off_host = host.off
        return out

    def batch(self, ids):
        """The queries `ids`, in that order, with their answers: a KvsAllQueries
        on the same device.  On a device it is index arithmetic only: no
        device-to-host read."""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        oh = self._off_host.astype(np.int64)
        lens = oh[ids + 1] - oh[ids]
        boff = np.zeros(len(ids) + 1, dtype=np.int32)
        np.cumsum(lens, out=boff[1:])
        total = int(boff[-1])
        if self.device is None:
            src = np.repeat(oh[ids] - boff[:-1], lens) + np.arange(total)
            return KvsAllQueries(self.anchor[ids], self.rel[ids], self.dir[ids], boff,
                                 self.ans[src], self.n_ent, self.n_rel)
        dev = self.device
        i = torch.as_tensor(ids, device=dev)
        shift = torch.as_tensor(oh[ids] - boff[:-1], device=dev)
        src = torch.repeat_interleave(shift, torch.as_tensor(lens, device=dev),
                                      output_size=total) + torch.arange(total, device=dev)
        out = KvsAllQueries(self.anchor[i].contiguous(), self.rel[i].contiguous(),
                            self.dir[i].contiguous(), torch.as_tensor(boff, device=dev),
                            self.ans[src].contiguous(), self.n_ent, self.n_rel)
        out._off_host = boff
        return out


class OneNTrainer(StochasticTrainer):
    """What KvsAllTrainer and OneVsAllTrainer share: the kwargs and their
    refusals, the queries built once per fit and walked in StochasticTrainer's
    shuffled batches, the fused and the unfused route of a batch.  A regime
    names itself (`_REGIME`), its queries class, the model's two methods, what
    its negatives are (for the refusal of labelled ones), and pops its own
    kwargs in `_regime_hyperparams`."""

    _REGIME = None
    _QUERIES = None
    _GRADIENTS = _STEP = None
    _NEGATIVES = None

    def __init__(self, *args, **kwargs):
        model = args[0]
        model._require_kvsall(self._REGIME)
        who, name = type(self).__name__, type(model).__name__
        eps = float(kwargs.pop("label_smoothing", 0.0))
        if not 0.0 <= eps < 1.0:
            raise ValueError("%s on %s: label_smoothing %r outside [0, 1)" % (who, name, eps))
        hyper = [("label_smoothing", eps)] + self._regime_hyperparams(name, kwargs)
        self.directions = tuple(kwargs.pop("directions", ("tail", "head")))
        runner = kwargs.pop("device_runner", "auto")
        if runner != "auto":
            raise ValueError("%s on %s: device_runner %r; %s has no device runner (only 'auto' is "
                             "accepted): the named runners are PairwiseStochasticTrainer's"
                             % (who, name, runner, self._REGIME))
        if kwargs.get("samplef") is not None:
            raise ValueError("%s on %s: samplef given; %s scores every entity and draws no "
                             "negatives (sampled negatives train with StochasticTrainer or "
                             "PairwiseStochasticTrainer)" % (who, name, self._REGIME))
        if kwargs.get("device_loop"):
            raise ValueError("%s on %s: device_loop=True; there is no sampler to move to the "
                             "device, and every batch is already a handful of launches"
                             % (who, name))
        self._refuse_deterministic(name)
        super(OneNTrainer, self).__init__(*args, **kwargs)
        for key, value in hyper:
            self.model.add_hyperparam(key, value)
        self.queries = None

    def _regime_hyperparams(self, name, kwargs):
        """The regime's own kwargs, popped and checked: [(hyperparameter, value)]."""
        return []

    @classmethod
    def _refuse_deterministic(cls, name):
        if deterministic():
            raise ValueError("%s on %s: set_deterministic(True); %s adds the chain rule with float "
                             "atomics and sums its fp32 products in tile order, so it has no "
                             "deterministic mode" % (cls.__name__, name, cls._REGIME))

    def fit(self, xs, ys=None):
        who, name = type(self).__name__, type(self.model).__name__
        self._refuse_deterministic(name)
        if ys is not None and not np.all(np.asarray(ys) == 1):
            raise ValueError("%s on %s: labelled negatives (y != 1); %s"
                             % (who, name, self._NEGATIVES))
        q = self._QUERIES.from_triples(xs, self.model.sz, self.directions)
        nq, nb = len(q), int(self.nbatches)
        if nq == 0:
            raise ValueError("%s on %s: no triples to train on" % (who, name))
        if nb < 1 or nq // nb < 1:
            raise ValueError("%s on %s: nbatches = %d for %d queries; 1 <= nbatches <= %d"
                             % (who, name, nb, nq, nq))
        if nq // nb > MAX_BATCH:
            raise ValueError("%s on %s: nbatches = %d makes batches of %d queries (of %d); a batch "
                             "holds at most %d: use nbatches >= %d"
                             % (who, name, nb, nq // nb, nq, MAX_BATCH, nq // (MAX_BATCH + 1) + 1))
        self.queries = q.to(self.model.device)   # uploaded once
        self._optim(list(range(nq)))

    def _process_batch(self, ids):
        if len(ids) == 0:
            return
        batch = self.queries.batch(ids)
        if self.fused and self._fusable:
            if self._loss_dev is None:
                self._loss_dev = torch.zeros(1, dtype=torch.float32, device=self.model.device)
            getattr(self.model, self._STEP)(batch, self._updaters, self._loss_dev)
            return
        grads = getattr(self.model, self._GRADIENTS)(batch)
        self.loss += self.model.loss
        self._batch_step(grads)


class KvsAllTrainer(OneNTrainer):
    """KvsAll / 1-N training of DistMult and ComplEx.  For a batch of B queries
    over N entities, with eps = label_smoothing,

        y'_be = (1 - eps) [e answers b] + eps / N
        L     = (1 / B) sum_b sum_e BCE(sigma(q_b . E_e), y'_be)

    and the gradient is the plain gradient of L plus rparam * param (the
    model's logistic regulariser) -- not the library's mean over a row's
    occurrences: every entity row occurs in every query, so that mean would be
    the 1 / B already in L.  E is updated (and projected) on every row every
    batch; R on the rows some query of the batch names.  ``loss`` is the
    epoch's sum of the batches' L.

    kwargs: ``label_smoothing`` (default 0), ``directions`` (default ('tail',
    'head')), and StochasticTrainer's ``nbatches``, ``max_epochs``,
    ``learning_rate``, ``param_update``, ``post_epoch``, ``fused``.  There are
    no negatives to draw, so ``samplef``, ``device_loop=True`` and a named
    ``device_runner`` are refused, as is the deterministic mode (the chain
    rule adds with float atomics and the products are fp32 MFMA sums)."""

    _REGIME = "KvsAll"
    _QUERIES = KvsAllQueries
    _GRADIENTS, _STEP = "_kvsall_gradients", "_kvsall_step"
    _NEGATIVES = "every entity that does not answer a query is its negative"
