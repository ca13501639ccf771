"""Subgraph embeddings and subgraph ranking on the device.

The reference groups the triples by (relation, subject) and by (relation,
object), embeds every group with more than ``mincard`` members as the mean
(and the variance) of its members' entity vectors
(``Experiment.make_subgraphs``, skge/base.py:122-202; skge/subgraphs.py) and
ranks the groups for each test query (``FilteredRankingEval.
subgraph_positions``, skge/base.py:828-911).  Here:

``Subgraphs.from_triples(xs, mincard)``   the grouping (numpy; off the hot path)
``Subgraphs.embed(model, variance)``      SA, SV by ``skge_subgraph_embed``
``SubgraphRankingEval(xs, subgraphs)``    ranks by ``skge_subgraph_rank``

Both kernels are in csrc/skge_subgraph.hip; there is no CPU fallback.
"""
from collections import defaultdict
from enum import Enum

import numpy as np
import torch

from . import _lib as L
from .eval import _model_code, check_triple_ids, compute_scores, refuse_rotate
from .util import triples_array

SUBTYPE = Enum("SUBTYPE", "SPO POS")   # skge/subgraphs.py:4
_KINDS = (SUBTYPE.SPO, SUBTYPE.POS)


class Metadata(object):
    """One subgraph, with the reference's field names (skge/subgraphs.py:6-13):
    ``ent`` is the anchor, ``rel`` the relation, ``entities`` the members."""

    def __init__(self, sid, st, sent, srel, ssize, entities):
        self.subType = st
        self.subId = sid
        self.ent = sent
        self.rel = srel
        self.size = ssize
        self.entities = list(entities)


def _as_numpy_triples(xs):
    a = triples_array(xs)
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    return np.asarray(a, dtype=np.int64).reshape(-1, 3)


def _group(xs, kind, mincard):
    """The groups of one kind with count > mincard, in (p, anchor) order:
    (anchor, rel, count, members); the members keep the triples' order (a
    stable sort on (p, anchor), as the reference's ``sorted``)."""
    key, other = (0, 1) if kind == 0 else (1, 0)
    order = np.lexsort((xs[:, key], xs[:, 2]))
    p, a, m = xs[order, 2], xs[order, key], xs[order, other]
    if len(p) == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z
    first = np.ones(len(p), dtype=bool)
    first[1:] = (p[1:] != p[:-1]) | (a[1:] != a[:-1])
    start = np.flatnonzero(first)
    count = np.diff(np.append(start, len(p)))
    keep = count > mincard
    return a[start][keep], p[start][keep], count[keep], m[np.repeat(keep, count)]


class Subgraphs(object):
    """The subgraphs of a triple list: every SPO subgraph in (p, s) order, then
    every POS subgraph in (p, o) order.  Arrays, one entry per subgraph:
    ``kind`` (0 SPO, 1 POS), ``anchor``, ``rel``, ``size``; the members as a
    CSR, ``mem_off`` int64 [S + 1] and ``mem_ent`` int32."""

    def __init__(self, kind, anchor, rel, mem_off, mem_ent, mincard=None):
        self.kind = np.asarray(kind, dtype=np.int8)
        self.anchor = np.asarray(anchor, dtype=np.int32)
        self.rel = np.asarray(rel, dtype=np.int32)
        self.mem_off = np.asarray(mem_off, dtype=np.int64)
        self.mem_ent = np.asarray(mem_ent, dtype=np.int32)
        self.size = np.diff(self.mem_off)
        self.mincard = mincard
        self._meta = None
        self._dev = {}     # per device: mem_off, mem_ent, ans_off, ans_sub
        self._ids = None   # (kind, anchor, rel) -> subgraph id

    @classmethod
    def from_triples(cls, xs, mincard):
        xs = _as_numpy_triples(xs)
        parts = [_group(xs, kind, mincard) for kind in (0, 1)]
        kind = np.concatenate([np.full(len(g[0]), k, dtype=np.int8) for k, g in enumerate(parts)])
        count = np.concatenate([g[2] for g in parts])
        return cls(kind, np.concatenate([g[0] for g in parts]),
                   np.concatenate([g[1] for g in parts]),
                   np.concatenate([[0], np.cumsum(count)]),
                   np.concatenate([g[3] for g in parts]), mincard)

    def get_Nsubgraphs(self):
        return len(self.kind)

    def __len__(self):
        return len(self.kind)

    @property
    def subgraphs(self):
        """The reference's list of Metadata objects."""
        if self._meta is None:
            off, ent = self.mem_off.tolist(), self.mem_ent.tolist()
            self._meta = [Metadata(i, _KINDS[k], a, r, off[i + 1] - off[i], ent[off[i]:off[i + 1]])
                          for i, (k, a, r) in enumerate(zip(self.kind.tolist(),
                                                            self.anchor.tolist(),
                                                            self.rel.tolist()))]
        return self._meta

    def subgraph_id(self, kind, anchor, rel):
        """The id of the subgraph of ``kind`` anchored at (anchor, rel), or -1
        (the reference's get_skip_subgraphs, skge/base.py:775-781)."""
        if self._ids is None:
            self._ids = {}
            for i, key in enumerate(zip(self.kind.tolist(), self.anchor.tolist(),
                                        self.rel.tolist())):
                self._ids.setdefault(key, i)
        k = kind.value - 1 if isinstance(kind, SUBTYPE) else int(kind)
        return self._ids.get((k, int(anchor), int(rel)), -1)

    def _check_members(self, n_ent):
        if len(self.mem_ent) and (self.mem_ent.min() < 0 or self.mem_ent.max() >= n_ent):
            bad = int(np.argmax((self.mem_ent < 0) | (self.mem_ent >= n_ent)))
            raise ValueError("subgraphs: member %d is entity %d, out of range for %d entities"
                             % (bad, int(self.mem_ent[bad]), n_ent))

    def device_arrays(self, device, n_ent):
        """(mem_off, mem_ent, ans_off, ans_sub) on ``device``: the members' CSR
        and its inverse, entity -> the ascending ids of the subgraphs whose
        members contain it (int64 [n_ent + 1], int32), built once."""
        key = (str(torch.device(device)), int(n_ent))
        if key not in self._dev:
            self._check_members(n_ent)
            S = len(self)
            off = torch.as_tensor(self.mem_off, device=device)
            ent = torch.as_tensor(self.mem_ent, device=device)
            sub = torch.repeat_interleave(torch.arange(S, dtype=torch.int64, device=device),
                                          off[1:] - off[:-1])
            pairs = torch.unique(ent.long() * max(S, 1) + sub)    # sorted: (entity, subgraph)
            bounds = torch.arange(n_ent + 1, dtype=torch.int64, device=device) * max(S, 1)
            ans_off = torch.searchsorted(pairs, bounds).to(torch.int64).contiguous()
            ans_sub = (pairs % max(S, 1)).to(torch.int32).contiguous()
            if ans_sub.numel() == 0:
                ans_sub = torch.zeros(1, dtype=torch.int32, device=device)
            self._dev[key] = (off, ent, ans_off, ans_sub)
        return self._dev[key]

    def embed(self, model, variance=False, attach=False, sub_algo="transe"):
        """(SA, SV): float32 device tensors [S, d], the mean and (variance=True,
        else None) the variance of every subgraph's member rows of model.E --
        the reference's sub_algo == "transe" embeddings.  attach=True also sets
        model.SA / model.SV, as subgraphs_create does (skge/base.py:401-408)."""
        if sub_algo != "transe":
            raise NotImplementedError(
                "sub_algo %r: the reference's 'hole' branch (skge/base.py:174-184) folds the "
                "members with np.dot of two vectors, which is a scalar after the second member "
                "and not an embedding; only 'transe' is defined" % (sub_algo,))
        L.require_gpu()
        E = model.params["E"]
        S, d, dev = len(self), model.d, model.device
        if S == 0:
            raise ValueError("no subgraphs to embed (every group has count <= mincard)")
        off, ent, _, _ = self.device_arrays(dev, E.rows)
        SA = torch.empty((S, d), dtype=torch.float32, device=dev)
        SV = torch.empty((S, d), dtype=torch.float32, device=dev) if variance else None
        lib = L.lib()
        nbytes = lib.skge_subgraph_embed_workspace_bytes(S, d, len(self.mem_ent))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        L.check(lib.skge_subgraph_embed(L.stream_ptr(), L.ptr(E.data), E.rows, d, L.ptr(off),
                                        L.ptr(ent), S, L.ptr(SA), L.ptr(SV), L.ptr(ws), nbytes),
                "subgraph embed")
        if attach:
            model.SA = SA
            model.SV = SV
        return SA, SV


class SubgraphRankingEval(object):
    """xs: test triples (s, o, p); subgraphs: a Subgraphs.  Ranks the
    subgraphs' embeddings for every test triple: as tails of (s, p, ?) and as
    heads of (?, p, o), by the model's score with the embedding in the entity's
    place.  The tail query skips the SPO subgraph anchored at (s, p), the head
    query the POS subgraph anchored at (o, p)."""

    def __init__(self, xs, subgraphs):
        idx = defaultdict(list)
        for s, o, p in _as_numpy_triples(xs).tolist():
            idx[p].append((s, o))
        self.idx = dict(idx)
        self.sz = sum(len(v) for v in self.idx.values())
        self.subgraphs = subgraphs
        self._emb = None   # the last (model, variance) embedded here
        self.last_ranks = None

    def _queries(self):
        return [(s, o, p) for p, sos in self.idx.items() for (s, o) in sos]

    def _table(self, model, sub_dist, table):
        """SA or SV: ``table`` when given (a float32 [S, d] tensor on the
        model's device, e.g. embed()'s), else embedded here from the model's
        current E."""
        if table is not None:
            S = len(self.subgraphs)
            if not (torch.is_tensor(table) and tuple(table.shape) == (S, model.d)
                    and table.dtype == torch.float32 and table.device == model.device):
                raise ValueError("table must be a float32 [%d, %d] tensor on %s"
                                 % (S, model.d, model.device))
            return table.contiguous()
        SA, SV = self.subgraphs.embed(model, variance=sub_dist == "var")
        return SV if sub_dist == "var" else SA

    def ranks(self, model, sub_dist="avg", table=None):
        """(tail, head, found_tail, found_head): int arrays over the test
        triples in the evaluator's order (by relation, then insertion order).
        A rank is 1 + the number of eligible subgraphs scoring strictly above
        the best eligible subgraph that contains the answer; with no such
        subgraph found = 0 and the rank is the number of eligible subgraphs
        + 1."""
        if sub_dist == "kl":
            raise NotImplementedError(
                "sub_dist 'kl': the reference's get_kl_divergence_scores (skge/base.py:790) "
                "hard-codes the width 50 and takes its 'true' distribution from the first ten "
                "entities of a scan over all triples per query; it is not carried over")
        if sub_dist not in ("avg", "var"):
            raise ValueError("sub_dist must be 'avg' or 'var', not %r" % (sub_dist,))
        refuse_rotate(model, "subgraph ranking")
        L.require_gpu()
        code, rel = _model_code(model)
        E = model.params["E"]
        q = self._queries()
        check_triple_ids(q, E.rows, rel.rows, "test triples")
        n = len(q)
        zero = np.zeros(0, dtype=np.int64)
        if n == 0:
            return zero, zero, zero, zero
        sg, dev = self.subgraphs, model.device
        S = len(sg)
        if S == 0:
            raise ValueError("no subgraphs to rank (every group has count <= mincard)")
        X = self._table(model, sub_dist, table)
        _, _, ans_off, ans_sub = sg.device_arrays(dev, E.rows)
        skip_t = np.array([sg.subgraph_id(0, s, p) for s, o, p in q], dtype=np.int32)
        skip_h = np.array([sg.subgraph_id(1, o, p) for s, o, p in q], dtype=np.int32)
        queries = torch.as_tensor(np.asarray(q, dtype=np.int32), device=dev)
        skip_t, skip_h = torch.as_tensor(skip_t, device=dev), torch.as_tensor(skip_h, device=dev)
        out = torch.empty((n, 2), dtype=torch.int32, device=dev)
        found = torch.empty((n, 2), dtype=torch.int32, device=dev)
        lib = L.lib()
        nbytes = lib.skge_subgraph_rank_workspace_bytes(n, model.d)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        L.check(lib.skge_subgraph_rank(L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data),
                                       E.rows, model.d, L.ptr(X), S, L.ptr(queries), n,
                                       L.ptr(skip_t), L.ptr(skip_h), L.ptr(ans_off),
                                       L.ptr(ans_sub), L.ptr(ws), nbytes, L.ptr(out),
                                       L.ptr(found)), "subgraph rank")
        r = out.cpu().numpy().astype(np.int64)
        f = found.cpu().numpy().astype(np.int64)
        self.last_ranks = (r[:, 0], r[:, 1], f[:, 0], f[:, 1])
        return self.last_ranks

    def positions(self, model, sub_dist="avg", table=None):
        """The reference's ``{p: {'head': [...], 'tail': [...]}}``
        (subgraph_positions, skge/base.py:828-911)."""
        tail, head, _, _ = self.ranks(model, sub_dist, table)
        pos, k = {}, 0
        for p, sos in self.idx.items():
            n = len(sos)
            pos[p] = {"head": head[k:k + n].tolist(), "tail": tail[k:k + n].tolist()}
            k += n
        return pos


def subgraph_ranking_scores(pos, topk=10):
    """((MRR, mean rank, Hits@topk) of the heads, the same of the tails) over
    every relation of a positions() dictionary, through compute_scores."""
    head = [x for p in pos for x in pos[p]["head"]]
    tail = [x for p in pos for x in pos[p]["tail"]]
    return compute_scores(head, topk), compute_scores(tail, topk)
