"""Top-k link prediction on the device: which entities complete (s, p, ?) or
(?, p, o).

``LinkPredictor(model, known_triples).tails(s, p, k)`` / ``.heads(o, p, k)``
score every entity against each query and return the k best in one
``skge_topk`` call (csrc/skge_topk.hip): entity ids int64 [n, k] and scores
float32 [n, k], ordered by descending score, then ascending id among exactly
equal scores; when fewer than k entities are eligible the remaining slots
hold id -1 and score -inf.  ``.relations(s, o, k)`` asks for the relation slot
of (s, ?, o) the same way (``skge_reltopk``, csrc/skge_relation.hip).

scoring="eval" scores as FilteredRankingEval ranks (any TransE by the L1
distance); scoring="model" uses the model's own score (the squared L2
distance for ``TransE(l1=False)``).
"""
from collections import defaultdict

import numpy as np
import torch

from . import _lib as L
from .eval import _model_code, refuse_rotate, check_pool_ids, check_triple_ids, pool_csr, type_pools
from .util import triples_array

K_MAX = 128
_CACHE_ENTRIES = 8


def _check_ids(ids, n, what, kind):
    """Raise ValueError naming the first of ``ids`` outside 0 .. n - 1."""
    bad = (ids < 0) | (ids >= n)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError("%s: query %d has %s %d, out of range for %d"
                         % (what, i, kind, int(ids[i]), n))


class LinkPredictor(object):
    """model: a TransE, HolE or RESCAL; known_triples: every known (s, o, p),
    the filter of ``filtered=True``."""

    def __init__(self, model, known_triples=None, scoring="eval"):
        if scoring not in ("eval", "model"):
            raise ValueError("scoring must be 'eval' or 'model', not %r" % (scoring,))
        self.model = model
        self.scoring = scoring
        self._known = None if known_triples is None else triples_array(known_triples)
        self._answers = None   # ({(s, p): tails}, {(o, p): heads}, {(s, o): relations})
        self._csr = {}         # per device and query set: the exclusion CSR
        self._types = None     # candidates="typed": the type index's pools as a CSR

    def tails(self, s, p, k=10, filtered=True, exclude=None, candidates=None):
        """The k best objects of (s, p, ?).  candidates: None scores every
        entity; "typed" only the range of p in ``known_triples`` (the objects
        seen with p); a list of id arrays, one per query, or one array for
        all queries, is an explicit candidate pool; a tuple ``(pools,
        pool_ids)`` gives shared pools (pool_csr's forms) and each query's
        pool id, -1 being every entity (``skge_topk_pools``,
        csrc/skge_pools.hip).  Returned entities are pool members that are
        not excluded; ids are checked on the host."""
        return self._topk(s, p, k, filtered, exclude, 0, candidates)

    def heads(self, o, p, k=10, filtered=True, exclude=None, candidates=None):
        """The k best subjects of (?, p, o); candidates as tails(), "typed"
        being the domain of p."""
        return self._topk(o, p, k, filtered, exclude, 1, candidates)

    def relations(self, s, o, k=10, filtered=True, exclude=None):
        """The k best relations of (s, ?, o): relation ids int64 [n, k] and
        scores float32 [n, k] in one ``skge_reltopk`` call
        (csrc/skge_relation.hip), ordered and padded as tails().
        filtered=True excludes every known relation of (s, o); exclude: per
        query an iterable of further relation ids."""
        model = self.model
        refuse_rotate(model, "LinkPredictor.relations (relation prediction)")
        code, rel = _model_code(model)
        if self.scoring == "model":
            code = model._kernel_model()
        E = model.params["E"]
        n_ent, n_rel = E.rows, rel.rows
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= K_MAX:
            raise ValueError("k must be an integer in 1 .. %d, not %r" % (K_MAX, k))
        k = int(k)
        if filtered and self._known is None:
            raise ValueError("filtered=True needs known_triples (or pass filtered=False)")
        a = np.asarray(s, dtype=np.int64).reshape(-1)
        b = np.asarray(o, dtype=np.int64).reshape(-1)
        if len(a) != len(b):
            raise ValueError("relations: %d subjects for %d objects" % (len(a), len(b)))
        _check_ids(a, n_ent, "relations", "subject")
        _check_ids(b, n_ent, "relations", "object")
        if filtered:
            check_triple_ids(self._known, n_ent, n_rel, "known triples")
        n = len(a)
        if n == 0:
            return np.zeros((0, k), dtype=np.int64), np.zeros((0, k), dtype=np.float32)
        dev = model.device
        q = np.stack([a, b], axis=1).astype(np.int32)
        xkey = None if exclude is None else repr([None if e is None else np.asarray(e).tolist()
                                                  for e in (exclude if n > 1 else [exclude])])
        key = (str(torch.device(dev)), "rel", bool(filtered), q.tobytes(), xkey)
        csr = self._device_csr(
            key, lambda: self._exclusions(a, b, 2, filtered, exclude, n_rel), dev)
        pairs = torch.as_tensor(q, device=dev)
        lib = L.lib()
        rels = torch.empty((n, k), dtype=torch.int32, device=dev)
        scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        nbytes = lib.skge_reltopk_workspace_bytes(n, model.d, k, n_rel, code)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        L.check(lib.skge_reltopk(L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), n_ent, n_rel,
                                 model.d, L.ptr(pairs), n, k,
                                 L.ptr(csr[0]) if csr else None, L.ptr(csr[1]) if csr else None,
                                 L.ptr(ws), nbytes, L.ptr(rels), L.ptr(scores)), "reltopk")
        return rels.cpu().numpy().astype(np.int64), scores.cpu().numpy()

    # ---- host side: ids, the exclusion lists ----

    def _known_answers(self):
        if self._answers is None:
            tails, heads, rels = defaultdict(set), defaultdict(set), defaultdict(set)
            for s, o, p in self._known.tolist():
                tails[(s, p)].add(o)
                heads[(o, p)].add(s)
                rels[(s, o)].add(p)
            self._answers = (tails, heads, rels)
        return self._answers

    def _exclusions(self, anchors, rels, direction, filtered, exclude, n_ent):
        """Per query the sorted, de-duplicated union of its known answers
        (filtered) and its ``exclude`` ids, as (offsets [n + 1], ids) int32;
        None when every list is empty.  direction 2: the queries are (s, o)
        pairs and the ids relations, n_ent their range."""
        n = len(anchors)
        extra = [()] * n
        if exclude is not None:
            ex = list(exclude)
            if n == 1 and (len(ex) != 1 or np.ndim(ex[0]) == 0):
                ex = [ex]     # one query: a flat list of ids
            if len(ex) != n:
                raise ValueError("exclude: %d lists for %d queries" % (len(ex), n))
            extra = [np.asarray(() if e is None else e, dtype=np.int64).reshape(-1) for e in ex]
            for i, e in enumerate(extra):
                bad = (e < 0) | (e >= n_ent)
                if bad.any():
                    raise ValueError("exclude: query %d has %s %d, out of range for %d"
                                     % (i, "relation" if direction == 2 else "entity",
                                        int(e[np.argmax(bad)]), n_ent))
        known = self._known_answers()[direction] if filtered else {}
        off, ent = [0], []
        for i, (a, p) in enumerate(zip(anchors.tolist(), rels.tolist())):
            ids = set(known.get((a, p), ()))
            ids.update(int(x) for x in extra[i])
            ent.extend(sorted(ids))
            off.append(len(ent))
        if not ent:
            return None
        return np.asarray(off, dtype=np.int32), np.asarray(ent, dtype=np.int32)

    def _device_csr(self, key, build, device):
        if key not in self._csr:
            if len(self._csr) >= _CACHE_ENTRIES:
                self._csr.clear()
            csr = build()
            self._csr[key] = None if csr is None else tuple(
                torch.as_tensor(x, device=device) for x in csr)
        return self._csr[key]

    def _candidate_pools(self, candidates, rels, direction, n_ent, n_rel):
        """(off, ent, query_pool) of ``candidates`` (tails()): the pools' CSR
        (pool_csr: ids checked, Python lists sorted) and each query's pool."""
        n = len(rels)
        if isinstance(candidates, str):
            if candidates != "typed":
                raise ValueError("candidates must be None, 'typed' or id arrays, not %r"
                                 % (candidates,))
            if self._known is None:
                raise ValueError("candidates='typed' needs known_triples")
            check_triple_ids(self._known, n_ent, n_rel, "known triples")
            if self._types is None:
                self._types = pool_csr(type_pools(self._known, n_rel), n_ent, "candidates")
            off, ent = self._types
            return off, ent, check_pool_ids(2 * rels + (1 - direction), 2 * n_rel, "candidates")
        if isinstance(candidates, tuple) and len(candidates) == 2:     # shared pools
            off, ent = pool_csr(candidates[0], n_ent, "candidates")
            ids = check_pool_ids(candidates[1], len(off) - 1, "candidates")
            if len(ids) != n:
                raise ValueError("candidates: %d pool ids for %d queries" % (len(ids), n))
            return off, ent, ids
        if torch.is_tensor(candidates):
            candidates = candidates.cpu().numpy()
        if isinstance(candidates, np.ndarray):
            one = candidates.ndim == 1
        else:
            candidates = list(candidates)
            one = len(candidates) > 0 and all(np.ndim(c) == 0 for c in candidates)
        if one:     # one pool for every query
            off, ent = pool_csr([candidates], n_ent, "candidates")
            return off, ent, np.zeros(n, dtype=np.int32)
        if len(candidates) != n:
            raise ValueError("candidates: %d pools for %d queries" % (len(candidates), n))
        off, ent = pool_csr(list(candidates), n_ent, "candidates")
        return off, ent, np.arange(n, dtype=np.int32)

    # ---- the call ----

    def _topk(self, anchor, p, k, filtered, exclude, direction, candidates=None):
        model = self.model
        code, rel = _model_code(model)
        if self.scoring == "model":
            code = model._kernel_model()
        E = model.params["E"]
        n_ent, n_rel = E.rows, rel.rows
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= K_MAX:
            raise ValueError("k must be an integer in 1 .. %d, not %r" % (K_MAX, k))
        k = int(k)
        if filtered and self._known is None:
            raise ValueError("filtered=True needs known_triples (or pass filtered=False)")
        what = "heads" if direction else "tails"
        a = np.asarray(anchor, dtype=np.int64).reshape(-1)
        r = np.asarray(p, dtype=np.int64).reshape(-1)
        if len(r) == 1 and len(a) > 1:
            r = np.repeat(r, len(a))
        if len(a) != len(r):
            raise ValueError("%s: %d entities for %d relations" % (what, len(a), len(r)))
        _check_ids(a, n_ent, what, "object" if direction else "subject")
        _check_ids(r, n_rel, what, "relation")
        if filtered:
            check_triple_ids(self._known, n_ent, n_rel, "known triples")
        n = len(a)
        pools = None if candidates is None else self._candidate_pools(candidates, r, direction,
                                                                      n_ent, n_rel)
        if n == 0:
            return np.zeros((0, k), dtype=np.int64), np.zeros((0, k), dtype=np.float32)
        dev = model.device
        q = np.stack([a, r], axis=1).astype(np.int32)
        xkey = None if exclude is None else repr([None if e is None else np.asarray(e).tolist()
                                                  for e in (exclude if n > 1 else [exclude])])
        key = (str(torch.device(dev)), direction, bool(filtered), q.tobytes(), xkey)
        csr = self._device_csr(
            key, lambda: self._exclusions(a, r, direction, filtered, exclude, n_ent), dev)
        queries = torch.as_tensor(q, device=dev)
        lib = L.lib()
        ents = torch.empty((n, k), dtype=torch.int32, device=dev)
        scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        if pools is not None:
            off, ent, qpool = pools
            n_pools = len(off) - 1
            d_off = torch.as_tensor(off, device=dev)
            d_ent = torch.as_tensor(ent if len(ent) else np.zeros(1, dtype=np.int32), device=dev)
            d_qpool = torch.as_tensor(qpool, device=dev)
            nbytes = lib.skge_topk_pools_workspace_bytes(n, model.d, k, n_ent, n_pools)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            L.check(lib.skge_topk_pools(L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), n_ent,
                                        model.d, L.ptr(queries), n, direction, k, L.ptr(d_off),
                                        L.ptr(d_ent), n_pools, L.ptr(d_qpool),
                                        L.ptr(csr[0]) if csr else None,
                                        L.ptr(csr[1]) if csr else None,
                                        L.ptr(ws), nbytes, L.ptr(ents), L.ptr(scores)),
                    "topk (pools)")
            return ents.cpu().numpy().astype(np.int64), scores.cpu().numpy()
        nbytes = lib.skge_topk_workspace_bytes(n, model.d, k, n_ent)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        L.check(lib.skge_topk(L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), n_ent, model.d,
                              L.ptr(queries), n, direction, k,
                              L.ptr(csr[0]) if csr else None, L.ptr(csr[1]) if csr else None,
                              L.ptr(ws), nbytes, L.ptr(ents), L.ptr(scores)), "topk")
        return ents.cpu().numpy().astype(np.int64), scores.cpu().numpy()
