"""Nearest neighbours in embedding space: which rows of a table are most
similar to a given row or vector.

``Neighbours(model).topk(k)`` scores every row of the table against every
other row and returns the k best per row in one ``skge_neighbours`` call
(csrc/skge_neighbours.hip): ids int64 [n, k] and similarities float32 [n, k],
ordered by descending similarity, then ascending id among exactly equal
values; when fewer than k rows are eligible the remaining slots hold id -1
and -inf.  ``topk(k, rows=...)`` asks for some rows only; in both a row is
never its own neighbour.  ``query(vectors, k)`` takes external vectors and
excludes nothing.

The similarity is the cosine (default) or the dot product, in the fixed fp32
arithmetic of include/skge_hip.h; a zero row has cosine 0 with everything.

This is what the reference's eval-embeddings.py computes with ``cosTheta``
over all pairs followed by a sort per entity (``cosineMatrix``, which
truncates every cosine to an integer, and ``similarity``); ``shared_role``
is its TRAIN / TEST tag.
"""
import numpy as np
import torch

from . import _lib as L
from .predict import K_MAX
from .util import triples_array

METRICS = {"cosine": 0, "dot": 1}


class Neighbours(object):
    """model: a TransE, HolE or RESCAL; table: "E" (default), "R" (RESCAL's W
    [M, d, d] is viewed as [M, d * d]) or an [n, d] array or tensor, e.g. SA
    of ``Subgraphs.embed``.  A model's table is read at each call."""

    def __init__(self, model, table="E", metric="cosine"):
        if metric not in METRICS:
            raise ValueError("metric must be 'cosine' or 'dot', not %r" % (metric,))
        self.model = model
        self.metric = metric
        self._name = self._fixed = None
        if isinstance(table, str):
            if table not in ("E", "R"):
                raise ValueError("table must be 'E', 'R' or an [n, d] array, not %r" % (table,))
            self._name = table
        else:
            t = table if torch.is_tensor(table) else torch.as_tensor(np.asarray(table))
            if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
                raise ValueError("table must be 'E', 'R' or an [n, d] array, not shape %s"
                                 % (tuple(t.shape),))
            self._fixed = t

    def _table(self):
        """The table as a contiguous float32 [n, width] tensor on the model's device."""
        if self._fixed is not None:
            t = self._fixed
        else:
            params = self.model.params
            name = self._name if self._name in params else "W"     # RESCAL's relations
            t = params[name].data
            t = t.reshape(t.shape[0], -1)
        return t.to(device=self.model.device, dtype=torch.float32).contiguous()

    def topk(self, k=10, rows=None):
        """The k most similar other rows of every row (rows=None) or of the
        rows ``rows`` (ids, repeats allowed), the row itself excluded."""
        k = _check_k(k)
        T = self._table()
        if rows is None:
            return self._run(T, None, None, T.shape[0], k)
        r = np.asarray(rows, dtype=np.int64).reshape(-1)
        bad = (r < 0) | (r >= T.shape[0])
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError("topk: query %d is row %d, out of range for %d rows"
                             % (i, int(r[i]), T.shape[0]))
        return self._run(T, None, torch.as_tensor(r.astype(np.int32), device=T.device), len(r), k)

    def query(self, vectors, k=10):
        """The k rows most similar to each of ``vectors`` [n, width] (or one
        vector [width]); nothing is excluded."""
        k = _check_k(k)
        T = self._table()
        q = vectors if torch.is_tensor(vectors) else torch.as_tensor(np.asarray(vectors))
        if q.dim() == 1 and q.shape[0] == T.shape[1]:
            q = q.reshape(1, -1)
        if q.dim() != 2 or q.shape[1] != T.shape[1]:
            raise ValueError("query: vectors of shape %s for a table of width %d"
                             % (tuple(q.shape), T.shape[1]))
        q = q.to(device=T.device, dtype=torch.float32).contiguous()
        return self._run(T, q, None, q.shape[0], k)

    def _run(self, T, Q, rows, n, k):
        if n == 0:
            return np.zeros((0, k), dtype=np.int64), np.zeros((0, k), dtype=np.float32)
        L.require_gpu()
        N, d = T.shape
        lib = L.lib()
        ids = torch.empty((n, k), dtype=torch.int32, device=T.device)
        sims = torch.empty((n, k), dtype=torch.float32, device=T.device)
        nbytes = lib.skge_neighbours_workspace_bytes(n, N, d, k)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=T.device)
        L.check(lib.skge_neighbours(L.stream_ptr(), L.ptr(T), N, d, L.ptr(Q), L.ptr(rows), n,
                                    METRICS[self.metric], k, L.ptr(ws), nbytes, L.ptr(ids),
                                    L.ptr(sims)), "neighbours")
        return ids.cpu().numpy().astype(np.int64), sims.cpu().numpy()


def _check_k(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= K_MAX:
        raise ValueError("k must be an integer in 1 .. %d, not %r" % (K_MAX, k))
    return int(k)


def shared_role(ids, triples, rows=None):
    """bool [n, k]: is neighbour ids[i, c] *connected* to entity i (rows=None)
    or rows[i] in ``triples`` (s, o, p), as eval-embeddings.py means it --
    both are objects of some common relation (its ``incoming_neighbours``) or
    both are subjects of some common relation (``outgoing_neighbours``).

    The ENTITY ID ids[i, c] is tested.  The reference's tagging loop tests the
    rank index (``k in incoming_train``), which says nothing about the
    neighbour; that is not reproduced.  Padding ids (-1) give False.  Host
    NumPy."""
    ids = np.asarray(ids, dtype=np.int64)
    if ids.ndim != 2:
        raise ValueError("ids must be [n, k], not shape %s" % (ids.shape,))
    ent = np.arange(len(ids), dtype=np.int64) if rows is None else \
        np.asarray(rows, dtype=np.int64).reshape(-1)
    if len(ent) != len(ids):
        raise ValueError("shared_role: %d rows for %d rows of ids" % (len(ent), len(ids)))
    t = triples_array(triples).astype(np.int64).reshape(-1, 3)
    n_ent = int(max(ids.max(initial=-1), ent.max(initial=-1), t[:, :2].max(initial=-1))) + 1
    n_rel = int(t[:, 2].max(initial=-1)) + 1
    heads = np.zeros((n_ent, max(n_rel, 1)), dtype=bool)   # entity x relation: is a subject of
    tails = np.zeros((n_ent, max(n_rel, 1)), dtype=bool)   # is an object of
    heads[t[:, 0], t[:, 2]] = True
    tails[t[:, 1], t[:, 2]] = True
    out = np.zeros(ids.shape, dtype=bool)
    if ids.size == 0:
        return out
    ok = ids >= 0
    j = np.where(ok, ids, 0)
    for c in range(ids.shape[1]):
        both = (heads[ent] & heads[j[:, c]]).any(axis=1) | (tails[ent] & tails[j[:, c]]).any(axis=1)
        out[:, c] = both & ok[:, c]
    return out
