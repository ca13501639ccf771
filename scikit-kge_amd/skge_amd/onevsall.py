"""1vsAll training of DistMult and ComplEx with N3 (Lacroix et
al. 2018, "Canonical Tensor Decomposition for Knowledge Base Completion").

Every training triple is a *query* per direction -- (s, p, ?) with target o,
(?, p, o) with target s -- scored against every entity, with softmax
cross-entropy against its one target and the nuclear 3-norm regulariser
(skge_onevsall_grad / skge_onevsall_step, csrc/skge_kvsall.hip).  Queries are
not deduplicated: a triple that occurs twice is two queries.  There is no
sampler: `OneVsAllQueries` builds the queries once, on the host, and
`OneVsAllTrainer` walks them in StochasticTrainer's shuffled batches.
"""
import math

import numpy as np
import torch

from .base import StochasticTrainer, deterministic

MAX_BATCH = 4096          # skge_onevsall_*: queries per batch
_DIRECTIONS = {"tail": 0, "head": 1}


class OneVsAllQueries(object):
    """One query per triple (s, o, p) and direction: query i is (anchor[i],
    rel[i], dir[i], target[i]) -- dir 0 is (anchor, rel, ?) with the triple's
    object for target, dir 1 is (?, rel, anchor) with its subject.  The
    directions follow each other in the order given, the triples keep their
    input order within a direction, duplicates stay.  Arrays are int32 NumPy on
    the host; `.to` returns a copy holding device tensors."""

    def __init__(self, anchor, rel, dir, target, n_ent, n_rel):
        self.anchor, self.rel, self.dir, self.target = anchor, rel, dir, target
        self.n_ent, self.n_rel = int(n_ent), int(n_rel)

    @classmethod
    def from_triples(cls, xs, sz, directions=("tail", "head")):
        x = np.asarray(xs, dtype=np.int64).reshape(-1, 3)
        n_ent, n_rel = int(sz[0]), int(sz[2])
        dirs = []
        for name in directions:
            if name not in _DIRECTIONS:
                raise ValueError("OneVsAllQueries: direction %r; 'tail' and 'head' are served"
                                 % (name,))
            if _DIRECTIONS[name] not in dirs:
                dirs.append(_DIRECTIONS[name])
        if not dirs:
            raise ValueError("OneVsAllQueries: no direction given; 'tail' and 'head' are served")
        if len(x) and (x.min() < 0 or x[:, :2].max() >= n_ent or x[:, 2].max() >= n_rel):
            raise ValueError("OneVsAllQueries: a triple names a row outside sz = %r" % (tuple(sz),))
        cols = [[], [], [], []]
        for t in dirs:
            a, g = (x[:, 0], x[:, 1]) if t == 0 else (x[:, 1], x[:, 0])
            for c, v in zip(cols, (a, x[:, 2], np.full(len(x), t, dtype=np.int64), g)):
                c.append(v)
        return cls(*[np.concatenate(c).astype(np.int32) for c in cols], n_ent, n_rel)

    def __len__(self):
        return int(self.anchor.shape[0])

    def _arrays(self):
        return (self.anchor, self.rel, self.dir, self.target)

    @property
    def device(self):
        return self.anchor.device if torch.is_tensor(self.anchor) else None

    def to(self, device):
        """A copy with the four arrays on `device`."""
        host = self.numpy()
        return OneVsAllQueries(*[torch.as_tensor(a, device=device) for a in host._arrays()],
                               self.n_ent, self.n_rel)

    def numpy(self):
        if self.device is None:
            return self
        return OneVsAllQueries(*[a.cpu().numpy() for a in self._arrays()], self.n_ent, self.n_rel)

    def batch(self, ids):
        """The queries `ids`, in that order: a OneVsAllQueries on the same
        device.  On a device it is an index gather: no device-to-host read."""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if self.device is None:
            return OneVsAllQueries(*[a[ids] for a in self._arrays()], self.n_ent, self.n_rel)
        i = torch.as_tensor(ids, device=self.device)
        return OneVsAllQueries(*[a[i].contiguous() for a in self._arrays()], self.n_ent,
                               self.n_rel)


class OneVsAllTrainer(StochasticTrainer):
    """1vsAll training of DistMult and ComplEx.  For a batch of B queries over N
    entities, with eps = label_smoothing and z_be = q_b . E_e,

        y'_be = (1 - eps) [e == g_b] + eps / N
        L_ce  = (1 / B) sum_b ( log sum_e exp(z_be) - sum_e y'_be z_be )
        L_n3  = (n3 / B) sum_b ( |E_a|_3^3 + |R_p|_3^3 + |E_g|_3^3 )

    and the gradient is the plain gradient of L = L_ce + L_n3 plus rparam *
    param, summed and never averaged over a row's occurrences, as KvsAllTrainer
    takes it.  E is updated (and projected) on every row every batch; R on the
    rows some query of the batch names.  ``loss`` is the epoch's sum of the
    batches' L.

    kwargs: ``label_smoothing`` (default 0), ``n3`` (default 0), ``directions``
    (default ('tail', 'head')), and StochasticTrainer's ``nbatches``,
    ``max_epochs``, ``learning_rate``, ``param_update``, ``post_epoch``,
    ``fused``.  There are no negatives to draw, so ``samplef``,
    ``device_loop=True`` and a named ``device_runner`` are refused, as is the
    deterministic mode (the chain rule adds with float atomics and the products
    are fp32 MFMA sums)."""

    def __init__(self, *args, **kwargs):
        model = args[0]
        model._require_kvsall("1vsAll")
        name = type(model).__name__
        eps = float(kwargs.pop("label_smoothing", 0.0))
        if not 0.0 <= eps < 1.0:
            raise ValueError("OneVsAllTrainer on %s: label_smoothing %r outside [0, 1)"
                             % (name, eps))
        n3 = float(kwargs.pop("n3", 0.0))
        if not (n3 >= 0.0 and math.isfinite(n3)):
            raise ValueError("OneVsAllTrainer on %s: n3 %r; the N3 weight is a finite number "
                             ">= 0" % (name, n3))
        self.directions = tuple(kwargs.pop("directions", ("tail", "head")))
        runner = kwargs.pop("device_runner", "auto")
        if runner != "auto":
            raise ValueError("OneVsAllTrainer on %s: device_runner %r; 1vsAll has no device "
                             "runner (only 'auto' is accepted): the named runners are "
                             "PairwiseStochasticTrainer's" % (name, runner))
        if kwargs.get("samplef") is not None:
            raise ValueError("OneVsAllTrainer on %s: samplef given; 1vsAll scores every entity "
                             "and draws no negatives (sampled negatives train with "
                             "StochasticTrainer or PairwiseStochasticTrainer)" % name)
        if kwargs.get("device_loop"):
            raise ValueError("OneVsAllTrainer on %s: device_loop=True; there is no sampler to "
                             "move to the device, and every batch is already a handful of "
                             "launches" % name)
        self._refuse_deterministic(name)
        super(OneVsAllTrainer, self).__init__(*args, **kwargs)
        self.model.add_hyperparam("label_smoothing", eps)
        self.model.add_hyperparam("n3", n3)
        self.queries = None

    @staticmethod
    def _refuse_deterministic(name):
        if deterministic():
            raise ValueError("OneVsAllTrainer on %s: set_deterministic(True); 1vsAll adds the "
                             "chain rule with float atomics and sums its fp32 products in tile "
                             "order, so it has no deterministic mode" % name)

    def fit(self, xs, ys=None):
        name = type(self.model).__name__
        self._refuse_deterministic(name)
        if ys is not None and not np.all(np.asarray(ys) == 1):
            raise ValueError("OneVsAllTrainer on %s: labelled negatives (y != 1); every entity "
                             "but a query's target is its negative" % name)
        q = OneVsAllQueries.from_triples(xs, self.model.sz, self.directions)
        nq, nb = len(q), int(self.nbatches)
        if nq == 0:
            raise ValueError("OneVsAllTrainer on %s: no triples to train on" % name)
        if nb < 1 or nq // nb < 1:
            raise ValueError("OneVsAllTrainer on %s: nbatches = %d for %d queries; 1 <= nbatches "
                             "<= %d" % (name, nb, nq, nq))
        if nq // nb > MAX_BATCH:
            raise ValueError("OneVsAllTrainer on %s: nbatches = %d makes batches of %d queries "
                             "(of %d); a batch holds at most %d: use nbatches >= %d"
                             % (name, nb, nq // nb, nq, MAX_BATCH, nq // (MAX_BATCH + 1) + 1))
        self.queries = q.to(self.model.device)   # uploaded once
        self._optim(list(range(nq)))

    def _process_batch(self, ids):
        if len(ids) == 0:
            return
        batch = self.queries.batch(ids)
        if self.fused and self._fusable:
            if self._loss_dev is None:
                self._loss_dev = torch.zeros(1, dtype=torch.float32, device=self.model.device)
            self.model._onevsall_step(batch, self._updaters, self._loss_dev)
            return
        grads = self.model._onevsall_gradients(batch)
        self.loss += self.model.loss
        self._batch_step(grads)
