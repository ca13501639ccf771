"""ComplEx: score Re sum_j R[p]_j E[s]_j conj(E[o]_j), DistMult's conventions
(distmult.py) with complex components.

``ncomp = d`` counts floats and must be even: a row holds d/2 complex
components INTERLEAVED, component j is (re, im) = (x[2j], x[2j + 1]).  The
layout is public -- ``model.params`` and model files show it.  It is what
keeps both halves of a component in neighbouring lanes of one register on the
device (csrc/skge_diag.h)."""
from . import _lib as L
from .distmult import DistMult


class ComplEx(DistMult):
    model_code = L.SKGE_COMPLEX

    def _check_width(self):
        if int(self.ncomp) % 2:
            raise ValueError("ComplEx needs an even ncomp (d/2 interleaved complex components), "
                             "not %d" % int(self.ncomp))
