"""RotatE: score -sum_j |E[s]_j * R[p]_j - E[o]_j| over d/2 complex components,
a distance model like TransE whose relations are rotations.

``ncomp = d`` counts floats and must be even: a row holds d/2 complex
components INTERLEAVED, component j is (re, im) = (x[2j], x[2j + 1]), ComplEx's
layout (complex.py).  R is stored at width d like E -- not as d/2 phases -- and
every one of its components is put back on the unit circle after each update
(param.unitmod, SKGE_POST_UNITMOD).  E is TransE's: init_nunif, then unit rows
(normalize), and so is the loss: the raw pairwise margin with a strict >,
contribution lists (sp, op, sn, on) and (pp, pn), mean over occurrences, no
rparam.  The arithmetic is csrc/skge_rot.h; _pairwise_gradients ->
skge_pair_grad, the device pair loop -> k_rot_pos.

Not served (each raises ValueError): the logistic trainer, relation
prediction, subgraph ranking, the pipelined / two-launch / data-parallel
runners."""
import numpy as np

from . import _lib as L
from .base import Model
from .param import normalize, unitmod


def init_phases(rows, d):
    """R [rows][d] from numpy's global RNG: theta ~ U(-pi, pi) per component,
    (cos theta, sin theta) interleaved, in float64."""
    theta = np.random.uniform(-np.pi, np.pi, (rows, d // 2))
    R = np.empty((rows, d), dtype=np.float64)
    R[:, 0::2] = np.cos(theta)
    R[:, 1::2] = np.sin(theta)
    return R


class RotatE(Model):
    default_posts = {"E": normalize, "R": unitmod}   # posts restored when a model file has none
    model_code = L.SKGE_ROTATE
    rel_id = "R"

    def __init__(self, *args, **kwargs):
        super(RotatE, self).__init__(*args, **kwargs)
        self.add_hyperparam("sz", args[0])
        self.add_hyperparam("ncomp", args[1])
        if int(self.ncomp) % 2:
            raise ValueError("RotatE needs an even ncomp (d/2 interleaved complex components), "
                             "not %d" % int(self.ncomp))
        self.add_param("E", (self.sz[0], self.ncomp), post=normalize)
        # drawn after E: phases, not init's distribution
        self.add_param("R", None, post=unitmod, value=init_phases(self.sz[2], int(self.ncomp)))

    def _gradients(self, xys):
        raise ValueError("RotatE has no logistic loss (its scores are <= 0: the loss needs a "
                         "gamma offset)")

    def _logistic_step(self, trip, ys, updaters, loss):
        raise ValueError("RotatE has no logistic loss (its scores are <= 0: the loss needs a "
                         "gamma offset)")
