"""Filtered link-prediction ranking on the device (mirrors FilteredRankingEval,
skge/base.py:737-1031, with the TransEEval / HolEEval scorers of
skge/run_transe.py:15-29 and skge/run_hole.py:12-19).

``positions(model)`` returns the reference's structures
``(pos, fpos)`` = ``{p: {'head': [...], 'tail': [...]}}`` (raw, filtered),
computed for every test triple in one ``skge_rank`` call
(csrc/skge_eval.hip).  A position is 1 + #entities scoring strictly higher
than the true one: the reference's descending-argsort position whenever no
other entity ties the true score exactly (among exact ties the reference
follows numpy's unstable argsort order).
"""
import os
from collections import defaultdict

import numpy as np
import torch

from . import _lib as L
from .device import DeviceKG
from .util import triples_array


def _model_code(model):
    from .transe import TransE
    from .hole import HolE
    from .rescal import RESCAL
    from .distmult import DistMult
    from .rotate import RotatE
    if isinstance(model, (DistMult, RotatE)):   # ComplEx too: its own code
        return model.model_code, model.params["R"]
    if isinstance(model, TransE):
        return L.SKGE_TRANSE_L1, model.params["R"]
    if isinstance(model, HolE):
        return L.SKGE_HOLE, model.params["R"]
    if isinstance(model, RESCAL):
        return L.SKGE_RESCAL, model.params["W"]
    raise NotImplementedError("no evaluator for %s" % type(model).__name__)


def refuse_rotate(model, what):
    """ValueError for the questions RotatE is not served with: |s * r_j - o|
    has no single query vector against the relation table, and the subgraph
    ranks take the reference's three models."""
    from .rotate import RotatE
    if isinstance(model, RotatE):
        raise ValueError("%s is not served for RotatE" % what)


def check_triple_ids(triples, n_ent, n_rel, what="triples"):
    """Raise ValueError, naming the first offender, unless every (s, o, p) row
    of ``triples`` has 0 <= s, o < n_ent and 0 <= p < n_rel.  The ranking
    kernels index the tables with these ids unchecked, so this is the bounds
    check: it runs on the host, before anything is allocated or launched."""
    if torch.is_tensor(triples):
        triples = triples.cpu().numpy()
    a = np.asarray(triples).reshape(-1, 3)
    if a.shape[0] == 0:
        return
    bad = ((a[:, 0] < 0) | (a[:, 0] >= n_ent) | (a[:, 1] < 0) | (a[:, 1] >= n_ent) |
           (a[:, 2] < 0) | (a[:, 2] >= n_rel))
    if bad.any():
        i = int(np.argmax(bad))
        s, o, p = (int(x) for x in a[i])
        raise ValueError("%s: triple %d (s=%d, o=%d, p=%d) is out of range for %d entities and "
                         "%d relations" % (what, i, s, o, p, n_ent, n_rel))


def pool_csr(pools, n_ent, what="pools"):
    """Candidate pools as the CSR the pool entry points read
    (include/skge_hip.h, skge_rank_pools): (off int64 [n_pools + 1], ent
    int32), every pool's ids ascending and unique.  ``pools`` is a list of id
    collections, or a tuple ``(off, ent)`` that already is the CSR.  A pool
    given as a Python list, tuple or set is sorted and de-duplicated; an
    array (numpy or torch) must already be ascending and unique.  Raises
    ValueError, naming the first offender, for an id outside 0 .. n_ent - 1,
    for an array out of order and for offsets that are not a CSR's.  This is
    the bounds check: the kernels index the entity table with these ids."""
    if isinstance(pools, tuple) and len(pools) == 2:
        off, ent = (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in pools)
        off = off.astype(np.int64).reshape(-1)
        ent = ent.astype(np.int64).reshape(-1)
        if len(off) < 1 or off[0] != 0 or off[-1] != len(ent) or (np.diff(off) < 0).any():
            raise ValueError("%s: offsets are not a CSR over %d ids" % (what, len(ent)))
    else:
        rows = []
        for g in pools:
            if torch.is_tensor(g):
                g = g.cpu().numpy()
            if isinstance(g, np.ndarray):
                rows.append(g.astype(np.int64).reshape(-1))
            else:
                rows.append(np.unique(np.asarray(list(g), dtype=np.int64)))
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(r) for r in rows])
        ent = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    which = np.searchsorted(off, np.arange(len(ent)), side="right") - 1   # each id's pool
    bad = (ent < 0) | (ent >= n_ent)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError("%s: pool %d holds id %d, out of range for %d entities"
                         % (what, int(which[i]), int(ent[i]), n_ent))
    if len(ent) > 1:
        bad = (ent[1:] <= ent[:-1]) & (which[1:] == which[:-1])
        if bad.any():
            i = int(np.argmax(bad)) + 1
            raise ValueError("%s: pool %d is not ascending and unique (id %d after %d)"
                             % (what, int(which[i]), int(ent[i]), int(ent[i - 1])))
    return off, ent.astype(np.int32)


def check_pool_ids(ids, n_pools, what):
    """int32 array of ``ids``; ValueError naming the first one outside
    -1 .. n_pools - 1 (-1: every entity)."""
    a = np.asarray(ids, dtype=np.int64).reshape(-1)
    bad = (a < -1) | (a >= n_pools)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError("%s: entry %d names pool %d, outside -1 .. %d"
                         % (what, i, int(a[i]), n_pools - 1))
    return a.astype(np.int32)


def type_pools(types, n_rel):
    """The type index as a list of 2 * n_rel sorted id arrays, DeviceKG.pools'
    layout: pool 2p holds the subjects (the domain) of relation p, pool 2p + 1
    its objects (the range); a relation without triples has two empty pools.
    ``types``: a ``type_index(xs)`` dict, or an array of triples (s, o, p)."""
    sets = [set() for _ in range(2 * n_rel)]
    if isinstance(types, dict):
        for p, sides in types.items():
            if not 0 <= int(p) < n_rel:
                raise ValueError("type index: relation %d is out of range for %d relations"
                                 % (int(p), n_rel))
            sets[2 * int(p)].update(int(x) for x in sides[0])
            sets[2 * int(p) + 1].update(int(x) for x in sides[1])
    else:
        for s, o, p in triples_array(types).tolist():
            if not 0 <= p < n_rel:
                raise ValueError("type index: relation %d is out of range for %d relations"
                                 % (p, n_rel))
            sets[2 * p].add(s)
            sets[2 * p + 1].add(o)
    return [np.array(sorted(g), dtype=np.int64) for g in sets]


class FilteredRankingEval(object):
    """xs: test triples (s, o, p); true_triples: every known triple (the
    filter).  neval is accepted for signature compatibility (the reference
    computes it but evaluates every triple, base.py:955)."""

    def __init__(self, xs, true_triples, neval=-1):
        self.sz = len(xs)
        self.neval = neval
        idx = defaultdict(list)
        for s, o, p in triples_array(xs).tolist():
            idx[p].append((s, o))
        self.idx = dict(idx)
        self._true = triples_array(true_triples)
        self._kg = {}        # per device: the known-triple set
        self._answers = {}   # per device: the known-answer CSR
        self._relations = {}   # per device: the known-relation CSR
        self.last_ranks = None
        self.last_relation_ranks = None
        self.last_typed_candidates = None

    def _known_set(self, device):
        key = str(torch.device(device))
        if key not in self._kg:
            self._kg[key] = DeviceKG(self._true, device)
        return self._kg[key]

    def _known_answers(self, q, device):
        """Per query (s, o, p) its other known tails {o' != o: (s, o', p) known}
        and heads {s' != s: (s', o, p) known}, as int32 CSR on the device (the
        filter of skge/base.py:913-1031 as lists: a handful per query)."""
        key = str(torch.device(device))
        if key not in self._answers:
            tails, heads = defaultdict(set), defaultdict(set)
            for s, o, p in self._true.tolist():
                tails[(s, p)].add(o)
                heads[(o, p)].add(s)
            toff, tent, hoff, hent = [0], [], [0], []
            for s, o, p in q:
                tent.extend(sorted(x for x in tails.get((s, p), ()) if x != o))
                toff.append(len(tent))
                hent.extend(sorted(x for x in heads.get((o, p), ()) if x != s))
                hoff.append(len(hent))
            as_dev = lambda v: torch.as_tensor(np.asarray(v if v else [0], dtype=np.int32),
                                               device=device)
            self._answers[key] = (as_dev(toff), as_dev(tent), as_dev(hoff), as_dev(hent))
        return self._answers[key]

    def ranks(self, model):
        """[n, 4] int array: tail raw, tail filtered, head raw, head filtered,
        for the test triples in the evaluator's order (by relation, then
        insertion order, as positions() iterates)."""
        code, rel = _model_code(model)
        dev = model.device
        q = [(s, o, p) for p, sos in self.idx.items() for (s, o) in sos]
        E = model.params["E"]
        check_triple_ids(q, E.rows, rel.rows, "test triples")
        check_triple_ids(self._true, E.rows, rel.rows, "known triples")
        if not q:
            return np.zeros((0, 4), dtype=np.int64)
        queries = torch.as_tensor(np.asarray(q, dtype=np.int32), device=dev)
        lib = L.lib()
        out = torch.empty((len(q), 4), dtype=torch.int32, device=dev)
        if os.environ.get("SKGE_RANK_SET") == "1":   # A/B: the triple-set form (round 1)
            # no known triples: no set (skge_rank then filters nothing); an
            # empty triple array has no device pointer to build one from
            kg = self._known_set(dev) if len(self._true) else None
            nbytes = lib.skge_rank_workspace_bytes(len(q), model.d)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            L.check(lib.skge_rank(L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), E.rows,
                                  model.d, L.ptr(queries), len(q),
                                  L.ptr(kg.slots) if kg else None, kg.capacity if kg else 0,
                                  L.ptr(ws), nbytes, L.ptr(out)), "rank")
        else:
            toff, tent, hoff, hent = self._known_answers(q, dev)
            nbytes = lib.skge_rank_known_workspace_bytes(len(q), model.d)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            L.check(lib.skge_rank_known(L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data),
                                        E.rows, model.d, L.ptr(queries), len(q), L.ptr(toff),
                                        L.ptr(tent), L.ptr(hoff), L.ptr(hent), L.ptr(ws), nbytes,
                                        L.ptr(out)), "rank")
        self.last_ranks = out.cpu().numpy().astype(np.int64)
        return self.last_ranks

    def positions(self, mdl, plot=False, pagerankMap=None):
        return self._positions_of(self.ranks(mdl))

    def _positions_of(self, r):
        pos, fpos = {}, {}
        k = 0
        for p, sos in self.idx.items():
            n = len(sos)
            pos[p] = {"tail": r[k:k + n, 0].tolist(), "head": r[k:k + n, 2].tolist()}
            fpos[p] = {"tail": r[k:k + n, 1].tolist(), "head": r[k:k + n, 3].tolist()}
            k += n
        return pos, fpos

    # ---- candidate pools: ranks over a restricted candidate set ----

    def candidate_ranks(self, model, pools, tail_pool, head_pool):
        """ranks() over candidate pools: [n, 4] int64 laid out as ranks(), each
        rank counted over the members of the query's pool (and the true
        entity, whether the pool holds it or not) instead of all entities.
        ``pools``: a list of id collections or a tuple ``(off, ent)``
        (pool_csr); ``tail_pool`` / ``head_pool``: per test triple, in the
        evaluator's order, the pool id of its tail / head query, or -1 for
        every entity.  The filtered rank skips the known answers that are in
        the pool.  One ``skge_rank_pools`` call (csrc/skge_pools.hip); pool
        and member ids are checked here, on the host."""
        code, rel = _model_code(model)
        dev = model.device
        q = [(s, o, p) for p, sos in self.idx.items() for (s, o) in sos]
        E = model.params["E"]
        check_triple_ids(q, E.rows, rel.rows, "test triples")
        check_triple_ids(self._true, E.rows, rel.rows, "known triples")
        off, ent = pool_csr(pools, E.rows)
        n_pools = len(off) - 1
        tp = check_pool_ids(tail_pool, n_pools, "tail_pool")
        hp = check_pool_ids(head_pool, n_pools, "head_pool")
        if len(tp) != len(q) or len(hp) != len(q):
            raise ValueError("candidate_ranks: %d tail and %d head pool ids for %d test triples"
                             % (len(tp), len(hp), len(q)))
        if not q:
            return np.zeros((0, 4), dtype=np.int64)
        queries = torch.as_tensor(np.asarray(q, dtype=np.int32), device=dev)
        vec_pool = torch.as_tensor(np.stack([tp, hp], axis=1).reshape(-1), device=dev)
        d_off = torch.as_tensor(off, device=dev)
        d_ent = torch.as_tensor(ent if len(ent) else np.zeros(1, dtype=np.int32), device=dev)
        toff, tent, hoff, hent = self._known_answers(q, dev)
        lib = L.lib()
        out = torch.empty((len(q), 4), dtype=torch.int32, device=dev)
        nbytes = lib.skge_rank_pools_workspace_bytes(len(q), model.d, n_pools)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        L.check(lib.skge_rank_pools(L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), E.rows,
                                    model.d, L.ptr(queries), len(q), L.ptr(d_off), L.ptr(d_ent),
                                    n_pools, L.ptr(vec_pool), L.ptr(toff), L.ptr(tent),
                                    L.ptr(hoff), L.ptr(hent), L.ptr(ws), nbytes, L.ptr(out)),
                "rank (pools)")
        return out.cpu().numpy().astype(np.int64)

    def typed_pools(self, n_rel, types=None):
        """(pools, tail_pool, head_pool) of the type-constrained protocol:
        the tail query of test triple (s, o, p) ranks over the range of p
        (pool 2p + 1), its head query over the domain (pool 2p).  types=None
        takes the type index of ``true_triples``; a ``type_index(xs)`` dict or
        an array of triples (the training triples, say) gives another."""
        pools = type_pools(self._true if types is None else types, n_rel)
        p = np.asarray([p for p, sos in self.idx.items() for _ in sos], dtype=np.int64)
        return pools, 2 * p + 1, 2 * p

    def typed_ranks(self, model, types=None):
        """Type-constrained ranks, [n, 4] int64 laid out as ranks():
        candidate_ranks over typed_pools.  ``last_typed_candidates`` [n, 2]
        then holds the number of candidates each tail / head rank was taken
        over, |pool + the true entity|."""
        pools, tp, hp = self.typed_pools(_model_code(model)[1].rows, types)
        r = self.candidate_ranks(model, pools, tp, hp)
        q = [(s, o, p) for p, sos in self.idx.items() for (s, o) in sos]
        cand = np.zeros((len(q), 2), dtype=np.int64)
        for i, (s, o, p) in enumerate(q):
            for col, pool, true in ((0, pools[tp[i]], o), (1, pools[hp[i]], s)):
                j = int(np.searchsorted(pool, true))
                cand[i, col] = len(pool) + (0 if j < len(pool) and pool[j] == true else 1)
        self.last_typed_candidates = cand
        return r

    def typed_positions(self, model, types=None):
        """positions()'s structures (pos, fpos) from typed_ranks;
        ranking_scores works on them unchanged."""
        return self._positions_of(self.typed_ranks(model, types))

    # ---- the relation slot: the position of p among all relations of (s, ?, o) ----

    def _known_relations(self, q, device):
        """Per query (s, o, p) its other known relations {p' != p: (s, o, p')
        known}, ascending, as int32 CSR on the device."""
        key = str(torch.device(device))
        if key not in self._relations:
            rels = defaultdict(set)
            for s, o, p in self._true.tolist():
                rels[(s, o)].add(p)
            off, rel = [0], []
            for s, o, p in q:
                rel.extend(sorted(x for x in rels.get((s, o), ()) if x != p))
                off.append(len(rel))
            as_dev = lambda v: torch.as_tensor(np.asarray(v if v else [0], dtype=np.int32),
                                               device=device)
            self._relations[key] = (as_dev(off), as_dev(rel))
        return self._relations[key]

    def relation_ranks(self, model):
        """[n, 2] int64 array: raw and filtered rank of the true relation p
        among all relations of (s, ?, o), for the test triples in the
        evaluator's order (as ranks()).  A rank is 1 + #relations scoring
        strictly higher; the filtered rank skips every other p' with
        (s, o, p') known.  One ``skge_relrank`` call (csrc/skge_relation.hip)."""
        refuse_rotate(model, "relation_ranks (relation prediction)")
        code, rel = _model_code(model)
        dev = model.device
        q = [(s, o, p) for p, sos in self.idx.items() for (s, o) in sos]
        E = model.params["E"]
        check_triple_ids(q, E.rows, rel.rows, "test triples")
        check_triple_ids(self._true, E.rows, rel.rows, "known triples")
        if not q:
            self.last_relation_ranks = np.zeros((0, 2), dtype=np.int64)
            return self.last_relation_ranks
        queries = torch.as_tensor(np.asarray(q, dtype=np.int32), device=dev)
        off, known = self._known_relations(q, dev)
        lib = L.lib()
        out = torch.empty((len(q), 2), dtype=torch.int32, device=dev)
        nbytes = lib.skge_relrank_workspace_bytes(len(q), model.d, rel.rows, code)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        L.check(lib.skge_relrank(L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), E.rows,
                                 rel.rows, model.d, L.ptr(queries), len(q), L.ptr(off),
                                 L.ptr(known), L.ptr(ws), nbytes, L.ptr(out)), "relrank")
        self.last_relation_ranks = out.cpu().numpy().astype(np.int64)
        return self.last_relation_ranks

    def relation_positions(self, model):
        """(pos, fpos) = {p: {'rel': [...]}} (raw, filtered): positions()'s
        structure for the relation slot."""
        r = self.relation_ranks(model)
        pos, fpos = {}, {}
        k = 0
        for p, sos in self.idx.items():
            n = len(sos)
            pos[p] = {"rel": r[k:k + n, 0].tolist()}
            fpos[p] = {"rel": r[k:k + n, 1].tolist()}
            k += n
        return pos, fpos


class TransEEval(FilteredRankingEval):
    """skge/run_transe.py:13-29 (scores -sum|E[s] + R[p] - E|, either norm)."""


class HolEEval(FilteredRankingEval):
    """skge/run_hole.py:10-19 (scores ccorr(R[p], E) . E[s])."""


def compute_scores(pos, hits=10):
    """(MRR, mean position, hits@k in percent), skge/base.py:1099-1103."""
    pos = np.asarray(pos, dtype=np.float64)
    return float(np.mean(1.0 / pos)), float(np.mean(pos)), float(np.mean(pos <= hits) * 100)


def ranking_scores(pos, fpos):
    """Raw and filtered (MRR, mean position, hits@10) over heads and tails of
    every relation, as ranking_scores (skge/base.py:1050-1058) aggregates."""
    raw = [x for k in pos for x in pos[k]["head"] + pos[k]["tail"]]
    filt = [x for k in fpos for x in fpos[k]["head"] + fpos[k]["tail"]]
    return compute_scores(raw), compute_scores(filt)


def relation_ranking_scores(pos, fpos, hits=1):
    """Raw and filtered (MRR, mean position, hits@``hits`` in percent) over the
    relation positions of every relation (relation_positions' structures)."""
    raw = [x for k in pos for x in pos[k]["rel"]]
    filt = [x for k in fpos for x in fpos[k]["rel"]]
    return compute_scores(raw, hits), compute_scores(filt, hits)
