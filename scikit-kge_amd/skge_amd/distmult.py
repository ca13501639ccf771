"""DistMult: score sum_k E[s]_k R[p]_k E[o]_k, with HolE's conventions
(hole.py) wherever a choice exists -- E projected by normless1, the pairwise
violation f(n) + margin > f(p), contribution lists (pp, pn) and (sp, sn, op,
on), mean over occurrences, rparam on R (pairwise) or on both (logistic).

_gradients -> skge_triple_grad; _pairwise_gradients -> skge_pair_grad.  The
products are taken on rows held in registers (csrc/skge_diag.h)."""
from . import _lib as L
from . import actfun as af
from .base import Model
from .param import normless1


class DistMult(Model):
    default_posts = {"E": normless1}   # posts restored when loading a model file without them
    model_code = L.SKGE_DISTMULT
    rel_id = "R"

    def __init__(self, *args, **kwargs):
        super(DistMult, self).__init__(*args, **kwargs)
        self.add_hyperparam("sz", args[0])
        self.add_hyperparam("ncomp", args[1])
        self.add_hyperparam("rparam", kwargs.pop("rparam", 0.0))
        self.add_hyperparam("af", kwargs.pop("af", af.Sigmoid))
        self._check_width()
        self.add_param("E", (self.sz[0], self.ncomp), post=normless1)
        self.add_param("R", (self.sz[2], self.ncomp))

    def _check_width(self):
        pass

    def _af_code(self):
        return af.af_code(self.af)

    def _reg(self, mode):
        # as HolE: pairwise dR += rparam * R only; logistic both, outside the mean
        r = float(self.rparam)
        if mode == "pairwise":
            return {"E": (0.0, 0.0, 0.0), "R": (0.0, r, 0.0)}
        return {"E": (0.0, r, 0.0), "R": (0.0, r, 0.0)}
