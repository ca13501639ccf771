#!/usr/bin/env python3
"""Link-prediction fixture made by the reference's own LinkPredictionEval
(skge/base.py:1034-1047): for a few labelled score arrays, the (PR-AUC,
ROC-AUC) pair its ``scores`` returns.

Runs ONLY where the reference is: it is imported as tools/gen_golden.py does
(import_reference).  The evaluator is handed a stand-in model whose
``_scores`` returns the recorded fp32 scores, so the fixture pins the
reference's curve arithmetic (sklearn's precision_recall_curve / auc /
roc_auc_score as the reference calls them) and nothing of its models.

Writes tests/golden/linkpred/linkpred_ref.npz: per case k the arrays
xs_k (s, o, p) int64 [n, 3], ys_k (+-1) int64, scores_k float32 and
expect_k = (pr_auc, roc_auc) float64.  Data only.
Usage:  python tools/gen_golden_linkpred.py [--out tests/golden/linkpred]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

from gen_golden import import_reference  # noqa: E402

# (kind, n, seed): tests/linkpred_ref.curve_case (no +-inf scores: sklearn, and
# with it the reference, refuses them)
CASES = (("informative", 257, 1), ("levels8", 4097, 2), ("distinct", 255, 3), ("zeros", 256, 4),
         ("equal", 64, 6), ("informative", 2, 8))


class _Stub(object):
    def __init__(self, scores):
        self.scores = scores

    def _scores(self, ss, ps, os):
        return self.scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "tests", "golden", "linkpred"))
    args = ap.parse_args()
    out = os.path.abspath(args.out)
    ref = import_reference()
    import linkpred_ref as LR
    data = {"n_cases": np.int64(len(CASES))}
    for k, (kind, n, seed) in enumerate(CASES):
        s, y = LR.curve_case(kind, n, seed)
        if n == 2:
            y[:] = (1, 0)
        assert 0 < y.sum() < n
        rs = np.random.RandomState(100 + seed)
        xs = np.stack([rs.randint(0, 50, n), rs.randint(0, 50, n), rs.randint(0, 4, n)], axis=1)
        ys = np.where(y > 0, 1, -1).astype(np.int64)
        ev = ref.base.LinkPredictionEval([tuple(int(v) for v in r) for r in xs], ys)
        pr, roc = ev.scores(_Stub(s))
        data["xs_%d" % k] = xs.astype(np.int64)
        data["ys_%d" % k] = ys
        data["scores_%d" % k] = s
        data["expect_%d" % k] = np.array([pr, roc], dtype=np.float64)
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "linkpred_ref.npz")
    np.savez_compressed(path, **data)
    print("wrote %s (%d bytes), %d cases" % (path, os.path.getsize(path), len(CASES)))


if __name__ == "__main__":
    main()
