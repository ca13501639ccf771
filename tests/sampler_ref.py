"""Host restatement of the device samplers' counter-based draws
(csrc/skge_sampler.h, csrc/skge_device.h) and a replay of a whole epoch's
records for each sampler kind, for the GPU tests to compare against.

fmix32 and draw are written over numpy uint32 (wrapping 32-bit arithmetic, as
the device's); the 64-bit epoch keys over Python ints reduced mod 2^64.  The
replay takes the epoch's permutation as an input (the device's own, from
skge_epoch_permutation), a Python set as the rejection set and the type
index as plain CSR arrays, so it shares no code with the library.
"""
import numpy as np

RANDOM, TYPED, LCWA = 0, 1, 2
M64 = (1 << 64) - 1


def _u32(x):
    return np.asarray(x, dtype=np.uint64).astype(np.uint32)


def fmix32(h):
    """murmur3's 32-bit finaliser over uint32 (array or scalar)."""
    h = np.asarray(h, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return h


def mix64(z):
    """splitmix64's finaliser (Python int, mod 2^64)."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def epoch_sample_key(seed, epoch_key):
    return mix64(mix64((seed + 0xA0761D6478BD642F) & M64) ^ ((epoch_key * 0xE7037ED1A0B428DB) & M64))


def draw(skey, j, mode, tr, n):
    """draw(skey, j, mode, tr, n) in [0, n): tr may be an array of tries."""
    skey, j = int(skey) & M64, int(j) & M64
    tr = np.asarray(tr, dtype=np.uint32)
    with np.errstate(over="ignore"):
        h = fmix32((_u32(j & 0xFFFFFFFF) * np.uint32(0x9E3779B1)) ^ _u32(skey & 0xFFFFFFFF))
        x = (_u32(skey >> 32) ^ (_u32(j >> 32) * np.uint32(0x85EBCA77)) ^
             (np.uint32(mode) * np.uint32(0x27D4EB2F) + tr * np.uint32(0x165667B1)))
        h = fmix32(h ^ x)
    return ((h.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def _first(cands, ok):
    """The first candidate that passes, else -1 (skge/sample.py:41-46)."""
    for c in cands:
        c = int(c)
        if ok(c):
            return c
    return -1


def replay_records(kind, trip, perm, seed, epoch_key, pools, ntries, n_ent):
    """(rec [T, 4], rec_n1 [T]) of the epoch whose key is epoch_key, as
    include/skge_hip.h defines the kinds.  trip: [T, 3] (s, o, p); perm:
    perm[j] = index of the epoch's j-th positive; pools: (pool_off, pool_ent)
    or None for RANDOM."""
    trip = np.asarray(trip, dtype=np.int64)
    known = set(map(tuple, trip.tolist()))
    skey = epoch_sample_key(int(seed), int(epoch_key))
    tries = np.arange(ntries)
    T = len(trip)
    rec = np.empty((T, 4), dtype=np.int64)
    rec_n1 = np.empty(T, dtype=np.int64)
    if pools is not None:
        off, ent = (np.asarray(a, dtype=np.int64) for a in pools)
    for j in range(T):
        s, o, p = (int(v) for v in trip[int(perm[j])])
        pool = [None, None]
        if kind != RANDOM:
            pool = [ent[off[2 * p + m]:off[2 * p + m + 1]] for m in (0, 1)]
        free0 = lambda c: (c, o, p) not in known
        free1 = lambda c: (s, c, p) not in known
        if kind == TYPED:
            n0 = _first(pool[0][draw(skey, j, 0, tries, len(pool[0]))], free0) if len(pool[0]) else -1
            n1 = _first(pool[1][draw(skey, j, 1, tries, len(pool[1]))], free1) if len(pool[1]) else -1
        else:
            subj = set(pool[0].tolist()) if kind == LCWA else None
            n0 = _first(draw(skey, j, 0, tries, n_ent),
                        free0 if kind == RANDOM else (lambda c: c in subj and free0(c)))
            n1 = _first(draw(skey, j, 1, tries, n_ent), free1)
        rec[j] = (s, o, p, n0)
        rec_n1[j] = n1
    return rec, rec_n1
