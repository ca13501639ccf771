"""Link-prediction AUC and triple classification on the device (mirrors
LinkPredictionEval, skge/base.py:1034-1047, and lp_callback, base.py:291-321).

``score_triples(model, xs)`` (``Model.score``) scores explicit triples through
``skge_score`` (csrc/skge_score.hip); ``curve_stats`` turns a labelled score
array into per-segment P, Nneg, the ROC numerator 2U, the PR trapezoid, the
average precision and the accuracy-maximising threshold in one sort
(``skge_curve_stats``, csrc/skge_curve.hip).  Nothing here falls back to the
host: the scores never leave the device before the statistics are formed.

PR-AUC is ``auc(recall, precision)`` of sklearn's ``precision_recall_curve``
(every threshold kept; sklearn >= 1.3 may drop intermediate ROC points, which
does not change the ROC area); ROC-AUC is ``roc_auc_score``.
"""
import numpy as np
import torch

from . import _lib as L
from .eval import check_triple_ids


def _tables(model):
    rel = model.params[model.rel_id]
    return model._kernel_model(), model.params["E"], rel


def host_triples(xs):
    """Triples in any accepted form (an int array or tensor [n, 3], a list of
    (s, o, p), the reference's list of ((s, o, p), y)) as int64 numpy [n, 3]:
    nothing is narrowed before the range check has seen it."""
    if torch.is_tensor(xs):
        a = xs.detach().cpu().numpy()
    elif isinstance(xs, np.ndarray):
        a = xs
    else:
        xs = list(xs)
        if len(xs) and len(xs[0]) == 2 and not np.isscalar(xs[0][0]):
            xs = [x for x, _ in xs]
        a = np.array(xs, dtype=np.int64)
    # row-major whatever the caller's strides (a[:, [1, 0, 2]] is column-major)
    return np.ascontiguousarray(np.asarray(a).reshape(-1, 3), dtype=np.int64)


def score_triples(model, triples):
    """Raw training scores of ``triples`` (array or list of (s, o, p)) as a
    device fp32 tensor [n] -- no activation applied.  Ids are range-checked on
    the host first (ValueError)."""
    L.require_gpu()
    code, E, rel = _tables(model)
    dev = model.device
    if torch.is_tensor(triples):
        check_triple_ids(triples, E.rows, rel.rows, "score")   # before narrowing to int32
        trip = triples.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
    else:
        a = host_triples(triples)
        check_triple_ids(a, E.rows, rel.rows, "score")
        trip = torch.as_tensor(a.astype(np.int32), device=dev)
    n = int(trip.shape[0])
    out = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    lib = L.lib()
    nbytes = int(lib.skge_score_workspace_bytes(code, n, rel.rows, model.d))
    if nbytes == 0:
        raise L.SkgeError("skge_score: sizes refused (n = %d, d = %d)" % (n, model.d))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.check(lib.skge_score(L.stream_ptr(), code, L.ptr(E.data), L.ptr(rel.data), E.rows, rel.rows,
                           model.d, L.ptr(trip), n, L.ptr(ws), nbytes, L.ptr(out)), "score")
    return out


def labels_array(ys):
    """+-1 or 0/1 labels -> int8 numpy, > 0 = true."""
    y = np.asarray(ys)
    return (y > 0).astype(np.int8)


class CurveStats(object):
    """Per-segment results of one ``skge_curve_stats`` call, as numpy arrays:
    P, Nneg, twoU, best_correct (int64), pr_auc, average_precision (float64,
    NaN where P or Nneg is 0), thresh (float32); roc_auc derived."""

    def __init__(self, counts, areas, thresh):
        self.P, self.Nneg = counts[:, 0].copy(), counts[:, 1].copy()
        self.twoU, self.best_correct = counts[:, 2].copy(), counts[:, 3].copy()
        self.pr_auc, self.average_precision = areas[:, 0].copy(), areas[:, 1].copy()
        self.thresh = thresh
        den = 2.0 * self.P.astype(np.float64) * self.Nneg.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.roc_auc = np.where(den > 0, self.twoU.astype(np.float64) / den, np.nan)


def curve_stats(scores, labels, seg=None, nseg=1):
    """Curve statistics of device scores [n] with labels (> 0 = true) and,
    optionally, segment ids in 0 .. nseg - 1.  Raises ValueError for
    mismatched lengths, segment ids out of range and NaN scores."""
    L.require_gpu()
    if not torch.is_tensor(scores) or scores.dtype != torch.float32 or not scores.is_cuda:
        raise TypeError("curve_stats: scores must be a device fp32 tensor")
    scores = scores.reshape(-1).contiguous()
    dev = scores.device
    n = int(scores.numel())
    lab = labels if torch.is_tensor(labels) else torch.as_tensor(labels_array(labels))
    lab = (lab > 0).to(device=dev, dtype=torch.int8).reshape(-1).contiguous()
    if int(lab.numel()) != n:
        raise ValueError("curve_stats: %d scores but %d labels" % (n, int(lab.numel())))
    nseg = int(nseg)
    if nseg < 1:
        raise ValueError("curve_stats: nseg = %d" % nseg)
    sg = None
    if seg is not None:
        sg = torch.as_tensor(seg).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if int(sg.numel()) != n:
            raise ValueError("curve_stats: %d scores but %d segment ids" % (n, int(sg.numel())))
        if n and (int(sg.min()) < 0 or int(sg.max()) >= nseg):
            raise ValueError("curve_stats: segment id outside 0 .. %d" % (nseg - 1))
    lib = L.lib()
    nbytes = int(lib.skge_curve_stats_workspace_bytes(n, nseg))
    if nbytes == 0:
        raise L.SkgeError("skge_curve_stats: sizes refused (n = %d, nseg = %d)" % (n, nseg))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.zeros((nseg, 4), dtype=torch.int64, device=dev)
    areas = torch.zeros((nseg, 2), dtype=torch.float64, device=dev)
    thresh = torch.zeros(nseg, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(lib.skge_curve_stats(L.stream_ptr(), L.ptr(scores), L.ptr(lab), L.ptr(sg), n, nseg,
                                 L.ptr(ws), nbytes, L.ptr(counts), L.ptr(areas), L.ptr(thresh),
                                 L.ptr(status)), "curve_stats")
    check_curve_status(int(status.item()))
    return CurveStats(counts.cpu().numpy(), areas.cpu().numpy(), thresh.cpu().numpy())


def check_curve_status(st):
    """Raise ValueError on skge_curve_stats's status bits."""
    if st & 1:
        raise ValueError("curve_stats: a score is NaN")
    if st & 2:
        raise ValueError("curve_stats: a segment id is out of range")


def require_both_classes(P, Nneg, what):
    """sklearn's rule for ROC: one class only -> the area is undefined."""
    if P == 0 or Nneg == 0:
        raise ValueError("%s is undefined: %d true and %d false triples" % (what, P, Nneg))


def _check_xy(xs, ys):
    a = host_triples(xs)          # int64: score_triples checks the ids before narrowing
    y = labels_array(ys)
    if len(y) != len(a):
        raise ValueError("%d triples but %d labels" % (len(a), len(y)))
    return a, y


class LinkPredictionEval(object):
    """The reference's LinkPredictionEval: a labelled set of triples (s, o, p),
    ys +-1 or 0/1; ``scores(model)`` -> (PR-AUC, ROC-AUC)."""

    def __init__(self, xs, ys):
        self.xs, self.ys = _check_xy(xs, ys)

    def _global(self, model):
        st = curve_stats(score_triples(model, self.xs), self.ys)
        require_both_classes(int(st.P[0]), int(st.Nneg[0]), "AUC")
        return st

    def scores(self, model):
        st = self._global(model)
        return float(st.pr_auc[0]), float(st.roc_auc[0])

    def average_precision(self, model):
        return float(self._global(model).average_precision[0])

    def per_relation(self, model):
        """dict of arrays [n_rel]: P, Nneg, roc_auc, pr_auc, average_precision
        (NaN where a relation lacks a class)."""
        n_rel = model.params[model.rel_id].rows
        st = curve_stats(score_triples(model, self.xs), self.ys, seg=self.xs[:, 2], nseg=n_rel)
        return {"P": st.P, "Nneg": st.Nneg, "roc_auc": st.roc_auc, "pr_auc": st.pr_auc,
                "average_precision": st.average_precision}


class TripleClassifier(object):
    """Triple classification (the NTN / TransE protocol): thresholds fitted on
    validation scores to maximise accuracy, per relation or one for all; a
    triple is predicted true when score >= threshold."""

    def __init__(self, model):
        self.model = model
        self.thresh = None          # float32 [n_rel]
        self.global_thresh = None

    def fit(self, valid_xs, valid_ys, per_relation=True):
        xs, ys = _check_xy(valid_xs, valid_ys)
        n_rel = self.model.params[self.model.rel_id].rows
        sc = score_triples(self.model, xs)
        g = curve_stats(sc, ys)
        self.global_thresh = np.float32(g.thresh[0])
        th = np.full(n_rel, self.global_thresh, dtype=np.float32)
        if per_relation:
            st = curve_stats(sc, ys, seg=xs[:, 2], nseg=n_rel)
            seen = (st.P + st.Nneg) > 0     # absent relations keep the global threshold
            th[seen] = st.thresh[seen]
        self.thresh = th
        return self

    def _predict(self, xs):
        if self.thresh is None:
            raise RuntimeError("TripleClassifier: fit() first")
        sc = score_triples(self.model, xs)
        th = torch.as_tensor(self.thresh, device=sc.device)
        rel = torch.as_tensor(np.ascontiguousarray(xs[:, 2]), device=sc.device).long()
        return sc >= th[rel]

    def predict(self, xs):
        return self._predict(host_triples(xs))

    def accuracy(self, xs, ys):
        """(overall accuracy, per-relation accuracies [n_rel], NaN for a
        relation without test triples)."""
        xs, ys = _check_xy(xs, ys)
        if len(xs) == 0:
            raise ValueError("accuracy of no triples is undefined")
        n_rel = len(self.thresh) if self.thresh is not None else 0
        ok = (self._predict(xs).cpu().numpy() == (ys > 0))
        tot = np.bincount(xs[:, 2], minlength=n_rel).astype(np.float64)
        hit = np.bincount(xs[:, 2], weights=ok.astype(np.float64), minlength=n_rel)
        with np.errstate(divide="ignore", invalid="ignore"):
            per = np.where(tot > 0, hit / tot, np.nan)
        return float(ok.mean()), per


def link_prediction_callback(ev_valid, ev_test, every=1):
    """A ``post_epoch`` function shaped like the reference's lp_callback:
    every ``every`` epochs it evaluates on validation, and when the PR-AUC
    improves it remembers the test scores of that epoch.  Writes no files; the
    record is the returned function's ``best`` dict."""
    best = {"epoch": None, "auc pr valid": -1.0, "auc roc valid": None, "auc pr test": None,
            "auc roc test": None}

    def post_epoch(trainer):
        if trainer.epoch % every == 0:
            pr_v, roc_v = ev_valid.scores(trainer.model)
            if pr_v > best["auc pr valid"]:
                pr_t, roc_t = ev_test.scores(trainer.model)
                best.update({"epoch": trainer.epoch, "auc pr valid": pr_v, "auc roc valid": roc_v,
                             "auc pr test": pr_t, "auc roc test": roc_t})
        return True

    post_epoch.best = best
    return post_epoch
