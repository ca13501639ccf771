"""Host restatement of the device draw of n negatives per positive over any
modes (include/skge_hip.h skge_negatives_t, csrc/skge_sampler.h sample_slot),
and the small KG the multi-negative tests share.

draw and epoch_sample_key come from tests/sampler_ref.py; the replay takes
the epoch's permutation as an input, a Python set as the rejection set and the
type index as plain CSR arrays, so it shares no code with the library.  The
keyed permutation is restated too (epoch_permutation), so that the CPU tests
can state properties of the very records the device draws; the GPU tests hold
it equal to skge_epoch_permutation.
"""
import functools

import numpy as np

from sampler_ref import LCWA, M64, RANDOM, TYPED, draw, epoch_sample_key, fmix32, mix64

KINDS = {"random": RANDOM, "typed": TYPED, "lcwa": LCWA}


# ---- the keyed permutation (csrc/skge_sampler.h: 4-round Feistel + cycle walking) ----

def epoch_perm_key(seed, epoch_key):
    return mix64((seed ^ mix64((epoch_key * 0xD6E8FEB86659FD93 + 1) & M64)) & M64)


def epoch_permutation(T, seed, epoch_key):
    bits = 1
    while (1 << bits) < T:
        bits += 1
    half = (bits + 1) // 2
    mask = (1 << half) - 1
    key = epoch_perm_key(int(seed) & M64, int(epoch_key))

    def feistel(x):
        Lh, Rh = x >> half, x & mask
        for r in range(4):
            kr = ((key >> (16 * r)) & 0xFFFFFFFF) ^ ((0x9E3779B9 * (r + 1)) & 0xFFFFFFFF)
            F = int(fmix32(np.uint32((Rh & 0xFFFFFFFF) ^ kr))) & mask
            Lh, Rh = Rh, Lh ^ F
        return (Lh << half) | Rh

    out = np.empty(T, dtype=np.int64)
    for j in range(T):
        x = feistel(j)
        while x >= T:
            x = feistel(x)
        out[j] = x
    return out


# ---- the replay ----

def pools_numpy(xs, n_rel):
    """The type index as a CSR over 2 * n_rel pools: pool 2p + side holds the
    ascending unique entities seen as subject (0) or object (1) of relation p."""
    off, ent = [0], []
    for p in range(n_rel):
        for side in (0, 1):
            ent += sorted(set(x[side] for x in xs if x[2] == p))
            off.append(len(ent))
    return np.asarray(off, dtype=np.int64), np.asarray(ent, dtype=np.int64)


def candidates(kind, skey, j, k, mode, x, pools, ntries, n_ent, n_rel, rel_range):
    """Slot k's ntries candidate ids in try order (None: the slot draws
    nothing, an empty pool)."""
    tries = np.arange(ntries)
    if mode == 2:
        return draw(skey, j, k, tries, rel_range if kind == TYPED else n_rel)
    if kind == TYPED:
        off, ent = pools
        pool = ent[off[2 * x[2] + mode]:off[2 * x[2] + mode + 1]]
        return pool[draw(skey, j, k, tries, len(pool))] if len(pool) else None
    return draw(skey, j, k, tries, n_ent)


def accepts(kind, known, subj_of, x, mode, c):
    """The kind's acceptance rule for candidate c of positive x = (s, o, p)
    (skge/sample.py:41-46, 75-88, 102-110); subj_of[p] is the set of subjects
    of relation p (LCWA's counts[(s, p)] > 0)."""
    t = list(x)
    t[mode] = int(c)
    if tuple(t) in known:
        return False
    return kind != LCWA or t[0] in subj_of.get(t[2], ())


def replay(kind, trip, perm, seed, epoch_key, pools, ntries, n_ent, n_rel, n, modes,
           rel_range=None):
    """(pos [T, 3], neg [T, K]) of the epoch whose key is epoch_key for
    Sampler(n, modes): slot k = rep * len(modes) + mi corrupts position
    modes[mi] with the first accepted of its ntries candidates, else -1."""
    trip = [tuple(int(v) for v in x) for x in np.asarray(trip).tolist()]
    known = set(trip)
    subj_of = {}
    for s, _, p in trip:
        subj_of.setdefault(p, set()).add(s)
    skey = epoch_sample_key(int(seed), int(epoch_key))
    modes = list(modes)
    K = n * len(modes)
    T = len(trip)
    pos = np.empty((T, 3), dtype=np.int64)
    neg = np.full((T, K), -1, dtype=np.int64)
    for j in range(T):
        x = trip[int(perm[j])]
        pos[j] = x
        for k in range(K):
            mode = modes[k % len(modes)]
            cands = candidates(kind, skey, j, k, mode, x, pools, ntries, n_ent, n_rel,
                               n_rel if rel_range is None else rel_range)
            for c in ([] if cands is None else cands):
                if accepts(kind, known, subj_of, x, mode, c):
                    neg[j, k] = int(c)
                    break
    return pos, neg


def negative_triple(x, mode, c):
    t = list(int(v) for v in x)
    t[mode] = int(c)
    return tuple(t)


def batch_pairs(pos, neg, modes, start, count):
    """The batch's pairs as PairwiseStochasticTrainer._process_batch appends
    them (skge/base.py:1394-1427): per positive, its kept negatives in slot order."""
    pp, nn = [], []
    for j in range(start, start + count):
        for k, c in enumerate(neg[j].tolist()):
            if c >= 0:
                pp.append(tuple(int(v) for v in pos[j]))
                nn.append(negative_triple(pos[j], modes[k % len(modes)], c))
    return pp, nn


def batch_triples(pos, neg, modes, start, count):
    """The batch's labelled triples as `xys += samplef(xys)` gives them: the
    positives, then every positive's kept negatives in slot order."""
    trip = [tuple(int(v) for v in pos[j]) for j in range(start, start + count)]
    trip += batch_pairs(pos, neg, modes, start, count)[1]
    ys = np.concatenate([np.ones(count), -np.ones(len(trip) - count)])
    return np.array(trip, dtype=np.int64), ys


# ---- the KG of the multi-negative tests ----
#
# 60 entities, 5 relations, 299 unique triples (299 % 3 == 2: nbatches = 3 has
# a remainder batch).  Relation 0 is the complete block {0..5} x {0..5} (36
# triples, self-loops included): an s- or o-corruption of one of its positives
# lands in the block with probability 1/10, so one try leaves some slots at
# -1.  Relations 1-3 hold random triples; relation 4 never occurs, so the
# typed sampler's rel_range is 4 < M.

N, M, T = 60, 5, 299
SEED = 21


def _make_kg():
    xs = [(s, o, 0) for s in range(6) for o in range(6)]
    rs = np.random.RandomState(7)
    seen = set(xs)
    while len(xs) < T:
        t = (int(rs.randint(N)), int(rs.randint(N)), 1 + int(rs.randint(3)))
        if t not in seen:
            seen.add(t)
            xs.append(t)
    return xs


XS = _make_kg()
KNOWN = set(XS)
OFF, ENT = pools_numpy(XS, M)
REL_RANGE = len(set(x[2] for x in XS))    # len(type_index(XS))

# the (n, modes) the tests draw
CASES = [(3, [0, 1]), (2, [0, 1, 2]), (1, [2]), (4, [1, 0, 0])]


@functools.lru_cache(maxsize=None)
def perm_of(key, seed=SEED):
    return epoch_permutation(T, seed, key)


@functools.lru_cache(maxsize=None)
def _replay_cached(kind, n, modes, ntries, key, seed):
    return replay(kind, XS, perm_of(key, seed), seed, key, (OFF, ENT), ntries, N, M, n, list(modes),
                  REL_RANGE if kind == TYPED else None)


def kg_replay(kind, n, modes, ntries, key, seed=SEED):
    """The shared KG's records, computed once per case (read-only)."""
    pos, neg = _replay_cached(kind, n, tuple(modes), ntries, key, seed)
    pos.setflags(write=False)
    neg.setflags(write=False)
    return pos, neg
