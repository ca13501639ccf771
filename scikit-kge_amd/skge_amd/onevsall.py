"""1vsAll training of DistMult and ComplEx with N3 (Lacroix et
al. 2018, "Canonical Tensor Decomposition for Knowledge Base Completion").

Every training triple is a *query* per direction -- (s, p, ?) with target o,
(?, p, o) with target s -- scored against every entity, with softmax
cross-entropy against its one target and the nuclear 3-norm regulariser
(skge_onevsall_grad / skge_onevsall_step, csrc/skge_kvsall.hip).  Queries are
not deduplicated: a triple that occurs twice is two queries.  There is no
sampler: `OneVsAllQueries` builds the queries once, on the host, and
`OneVsAllTrainer` walks them in StochasticTrainer's shuffled batches (both on
kvsall.py's shared bases).
"""
import math

import numpy as np

from .kvsall import MAX_BATCH, OneNQueries, OneNTrainer  # noqa: F401 (MAX_BATCH: skge_onevsall_*)


class OneVsAllQueries(OneNQueries):
    """One query per triple (s, o, p) and direction: query i is (anchor[i],
    rel[i], dir[i], target[i]) -- dir 0 is (anchor, rel, ?) with the triple's
    object for target, dir 1 is (?, rel, anchor) with its subject.  The
    directions follow each other in the order given, the triples keep their
    input order within a direction, duplicates stay.  Arrays are int32 NumPy on
    the host; `.to` returns a copy holding device tensors."""

    _FIELDS = ("anchor", "rel", "dir", "target")

    def __init__(self, anchor, rel, dir, target, n_ent, n_rel):
        super(OneVsAllQueries, self).__init__((anchor, rel, dir, target), n_ent, n_rel)

    @classmethod
    def from_triples(cls, xs, sz, directions=("tail", "head")):
        x, n_ent, n_rel, dirs = cls._parse(xs, sz, directions)
        cols = [[], [], [], []]
        for t in dirs:
            a, g = (x[:, 0], x[:, 1]) if t == 0 else (x[:, 1], x[:, 0])
            for c, v in zip(cols, (a, x[:, 2], np.full(len(x), t, dtype=np.int64), g)):
                c.append(v)
        return cls(*[np.concatenate(c).astype(np.int32) for c in cols], n_ent, n_rel)


class OneVsAllTrainer(OneNTrainer):
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

    _REGIME = "1vsAll"
    _QUERIES = OneVsAllQueries
    _GRADIENTS, _STEP = "_onevsall_gradients", "_onevsall_step"
    _NEGATIVES = "every entity but a query's target is its negative"

    def _regime_hyperparams(self, name, kwargs):
        n3 = float(kwargs.pop("n3", 0.0))
        if not (n3 >= 0.0 and math.isfinite(n3)):
            raise ValueError("OneVsAllTrainer on %s: n3 %r; the N3 weight is a finite number "
                             ">= 0" % (name, n3))
        return [("n3", n3)]
