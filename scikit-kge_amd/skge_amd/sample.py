"""Negative samplers (mirrors skge/sample.py).

RandomModeSampler, CorruptedSampler and LCWASampler here are the reference's
host samplers, statement for statement (same numpy global RNG stream, so a
seeded run draws the same negatives as the reference).  The throughput path
samples on the device instead (k_epoch_sample, csrc/skge_pipeline.hip; the
trainers' device_loop=True): RandomModeSampler(1, [0, 1]) on every device
runner, CorruptedSampler(1, xs, type_index(xs)) and LCWASampler(1, [0, 1])
on the pair loop and the logistic loop (skge_amd/device.py
device_sampler_args)."""
from collections import defaultdict as ddict
from copy import deepcopy

from numpy.random import randint


class Sampler(object):
    """skge/sample.py:11-25"""

    def __init__(self, n, modes, ntries=100):
        self.n = n
        self.modes = modes
        self.ntries = ntries

    def sample(self, xys):
        res = []
        for x, _ in xys:
            for _ in range(self.n):
                for mode in self.modes:
                    t = self._sample(x, mode)
                    if t is not None:
                        res.append(t)
        return res


class RandomModeSampler(Sampler):
    """Corrupt s (mode 0) or o (mode 1) with up to ntries rejection draws
    against the training set (skge/sample.py:28-46)."""

    def __init__(self, n, modes, xs, sz):
        super(RandomModeSampler, self).__init__(n, modes)
        self.xs = set(tuple(int(v) for v in x) for x in xs)
        self.sz = sz

    def _sample(self, x, mode):
        nex = list(x)
        res = None
        for _ in range(self.ntries):
            nex[mode] = randint(self.sz[mode])
            if tuple(nex) not in self.xs:
                res = (tuple(nex), -1.0)
                break
        return res


class CorruptedSampler(Sampler):
    """Type-constrained corruption (skge/sample.py:68-88): s (mode 0) is
    replaced by an entity seen as a subject of the triple's relation, o (mode
    1) by one seen as its object, mode 2 draws a relation; up to ntries
    rejection draws against the training set.

    The reference's constructor calls ``Sampler.__init__(n)`` without
    ``modes`` and so cannot be constructed; this one keeps its positional
    signature ``(n, xs, type_index)`` and adds the keyword ``modes`` ([0, 1],
    what the reference's driver passes its other samplers)."""

    def __init__(self, n, xs, type_index, modes=[0, 1]):
        super(CorruptedSampler, self).__init__(n, modes)
        self.xs = set(tuple(int(v) for v in x) for x in xs)
        self.type_index = type_index

    def _sample(self, x, mode):
        nex = list(deepcopy(x))
        res = None
        for _ in range(self.ntries):
            if mode == 2:
                nex[2] = randint(len(self.type_index))
            else:
                k = x[2]
                n = len(self.type_index[k][mode])
                nex[mode] = self.type_index[k][mode][randint(n)]
            if tuple(nex) not in self.xs:
                res = (tuple(nex), -1.0)
                break
        return res


class LCWASampler(RandomModeSampler):
    """Negatives under the local closed world assumption (skge/sample.py:
    91-110): a draw is kept only if its (subject, relation) occurs in the
    training set and the triple itself does not."""

    def __init__(self, n, modes, xs, sz):
        super(LCWASampler, self).__init__(n, modes, xs, sz)
        self.counts = ddict(int)
        for s, o, p in xs:
            self.counts[(s, p)] += 1

    def _sample(self, x, mode):
        nex = list(deepcopy(x))
        res = None
        for _ in range(self.ntries):
            nex[mode] = randint(self.sz[mode])
            if self.counts[(nex[0], nex[2])] > 0 and tuple(nex) not in self.xs:
                res = (tuple(nex), -1.0)
                break
        return res


def type_index(xs):
    """relation -> {0: its subjects, 1: its objects} (skge/sample.py:113-120)."""
    index = ddict(lambda: {0: set(), 1: set()})
    for i, j, k in xs:
        index[k][0].add(i)
        index[k][1].add(j)
    return {k: {0: list(v[0]), 1: list(v[1])} for k, v in index.items()}
