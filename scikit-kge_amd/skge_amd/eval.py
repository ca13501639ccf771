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
    if isinstance(model, TransE):
        return L.SKGE_TRANSE_L1, model.params["R"]
    if isinstance(model, HolE):
        return L.SKGE_HOLE, model.params["R"]
    if isinstance(model, RESCAL):
        return L.SKGE_RESCAL, model.params["W"]
    raise NotImplementedError("no evaluator for %s" % type(model).__name__)


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
        r = self.ranks(mdl)
        pos, fpos = {}, {}
        k = 0
        for p, sos in self.idx.items():
            n = len(sos)
            pos[p] = {"tail": r[k:k + n, 0].tolist(), "head": r[k:k + n, 2].tolist()}
            fpos[p] = {"tail": r[k:k + n, 1].tolist(), "head": r[k:k + n, 3].tolist()}
            k += n
        return pos, fpos

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
