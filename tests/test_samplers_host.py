"""Host side of the typed and LCWA samplers (CPU): the facade's
CorruptedSampler / LCWASampler / type_index against what the reference
returned for the same seeded numpy stream (tests/golden/samplers/sampler_*.npz,
tools/gen_golden_samplers.py), which samplers the device loops accept
(skge_amd.device.device_sampler_args, on a stub trainer), and the host
restatement of the device draws the GPU tests replay with
(tests/sampler_ref.py)."""
import os
import types

import numpy as np
import pytest

import sampler_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samplers")


def _fixture(name):
    z = np.load(os.path.join(GOLDEN, "sampler_%s.npz" % name))
    xs = [tuple(int(v) for v in x) for x in z["xs"].tolist()]
    sz = tuple(int(v) for v in z["sz"])
    want = [(tuple(int(v) for v in t), float(y)) for t, y in zip(z["neg"].tolist(), z["ys"])]
    return z, xs, sz, want


def _sample(smp, xs, seed):
    np.random.seed(seed)
    return smp.sample(list(zip(xs, [1.0] * len(xs))))


def test_lcwa_sampler_draws_what_the_reference_drew():
    from skge_amd.sample import LCWASampler
    z, xs, sz, want = _fixture("lcwa")
    got = _sample(LCWASampler(1, [0, 1], xs, sz), xs, int(z["seed"]))
    assert got == want
    assert 0 < len(want) < 2 * len(xs)   # some negatives not found: the None branch ran


def test_corrupted_sampler_draws_what_the_reference_drew():
    from skge_amd.sample import CorruptedSampler, type_index
    z, xs, sz, want = _fixture("corrupted")
    off, ent = z["index_off"], z["index_ent"]
    index = {p: {m: [int(v) for v in ent[off[2 * p + m]:off[2 * p + m + 1]]] for m in (0, 1)}
             for p in range(sz[2])}
    mine = type_index(xs)
    assert {k: {m: set(v[m]) for m in v} for k, v in mine.items()} == \
        {k: {m: set(v[m]) for m in v} for k, v in index.items()}
    smp = CorruptedSampler(1, xs, index)
    assert smp.modes == [0, 1] and smp.n == 1 and smp.ntries == 100
    got = _sample(smp, xs, int(z["seed"]))
    assert got == want
    assert 0 < len(want) < 2 * len(xs)
    # mode 2 draws a relation id (skge/sample.py:79-80)
    np.random.seed(1)
    t, y = CorruptedSampler(1, xs, index, modes=[2])._sample(xs[0], 2)
    assert y == -1.0 and t[:2] == xs[0][:2] and 0 <= t[2] < sz[2] and t not in set(xs)


# ---- which samplers the device loops take ----

N, M = 12, 3
XS = [(0, 1, 0), (2, 3, 0), (4, 1, 0), (5, 6, 1), (5, 7, 1), (8, 9, 2), (10, 9, 2), (8, 11, 2)]


def _trainer(samplef):
    model = types.SimpleNamespace(E=types.SimpleNamespace(rows=N), sz=(N, N, M))
    return types.SimpleNamespace(samplef=samplef, ntries=100, model=model)


def _args(samplef, xs=XS):
    from skge_amd.device import device_sampler_args
    return device_sampler_args(_trainer(samplef), xs, [1] * len(xs))


def test_new_samplers_are_eligible_with_their_kind():
    from skge_amd import _lib as L
    from skge_amd.sample import CorruptedSampler, LCWASampler, RandomModeSampler, type_index
    sz = (N, N, M)
    for smp, kind in ((RandomModeSampler(1, [0, 1], XS, sz), L.SKGE_SAMPLER_RANDOM),
                      (CorruptedSampler(1, XS, type_index(XS)), L.SKGE_SAMPLER_TYPED),
                      (CorruptedSampler(1, XS, type_index(XS), modes=[0, 1]), L.SKGE_SAMPLER_TYPED),
                      (LCWASampler(1, [0, 1], XS, sz), L.SKGE_SAMPLER_LCWA)):
        smp.ntries = 37
        a = _args(smp.sample)
        ok, ntries, why = a   # unpacks as it always has
        assert ok and ntries == 37 and why == "", (type(smp).__name__, why)
        assert a.kind == kind
    assert (L.SKGE_SAMPLER_RANDOM, L.SKGE_SAMPLER_TYPED, L.SKGE_SAMPLER_LCWA) == (0, 1, 2)


def test_non_matching_samplers_are_ineligible_with_a_reason():
    from skge_amd.sample import CorruptedSampler, LCWASampler, type_index
    sz = (N, N, M)
    foreign = type_index(XS)
    foreign[0][0] = foreign[0][0] + [7]           # an entity never a subject of relation 0
    repeated = type_index(XS)
    repeated[1][1] = repeated[1][1] + repeated[1][1][:1]

    class Mine(LCWASampler):
        def _sample(self, x, mode):
            return None

    cases = [
        (LCWASampler(1, [0, 1, 2], XS, sz), "modes=[0, 1, 2]"),
        (LCWASampler(2, [0, 1], XS, sz), "n=2"),
        (CorruptedSampler(2, XS, type_index(XS)), "n=2"),
        (CorruptedSampler(1, XS, type_index(XS), modes=[0, 1, 2]), "modes=[0, 1, 2]"),
        (CorruptedSampler(1, XS, foreign), "type_index"),
        (CorruptedSampler(1, XS, repeated), "type_index"),
        (CorruptedSampler(1, XS[:-1], type_index(XS)), "rejection set"),
        (LCWASampler(1, [0, 1], XS[:-1], sz), "rejection set"),
        (LCWASampler(1, [0, 1], XS, (N + 1, N + 1, M)), "sizes"),
        (Mine(1, [0, 1], XS, sz), "overridden"),
    ]
    for smp, what in cases:
        a = _args(smp.sample)
        assert not a[0] and what in a[2], (type(smp).__name__, what, a[2])
        assert a.kind == 0
    lc = LCWASampler(1, [0, 1], XS, sz)
    lc.counts[(11, 0)] += 1                       # counts no longer those of xs
    a = _args(lc.sample)
    assert not a[0] and "counts" in a[2]
    # the fit's triples differ from the sampler's
    a = _args(LCWASampler(1, [0, 1], XS, sz).sample, xs=XS[:-1])
    assert not a[0] and "rejection set" in a[2]
    assert not _args(lambda xys: [])[0]


# ---- the host restatement of the device draws ----

def test_draw_restatement_hand_values():
    """draw() against values worked out with plain Python integers from
    csrc/skge_sampler.h's definition (two fmix32 rounds over key, position,
    mode and try, then the multiply-shift into [0, n))."""
    assert [int(v) for v in R.fmix32([0, 1, 0xDEADBEEF])] == [0, 0x514E28B7, 0x0DE5C6A9]
    assert R.mix64(0) == 0xE220A8397B1DCDAF
    assert R.epoch_sample_key(11, 5) == 0x52C43796617DD83F
    k = 0x52C43796617DD83F
    assert int(R.draw(k, 5, 0, 0, 64)) == 60
    assert int(R.draw(0x0123456789ABCDEF, 299, 1, 99, 40943)) == 18425
    assert int(R.draw(0xFFFFFFFFFFFFFFFF, (1 << 32) + 5, 0, 7, 3)) == 2
    # tries as an array: element tr is the scalar draw of try tr
    assert R.draw(k, 5, 0, np.arange(2), 64).tolist() == [60, 33]
    assert int(R.draw(k, 5, 1, 0, 64)) == 1


def test_draw_restatement_range_and_determinism():
    k = R.epoch_sample_key(3, 9)
    for n in (1, 2, 7, 64, 40943, 2 ** 31 - 1):
        a = R.draw(k, 123, 0, np.arange(1000), n)
        assert a.min() >= 0 and a.max() < n
        assert np.array_equal(a, R.draw(k, 123, 0, np.arange(1000), n))
    a = R.draw(k, 123, 0, np.arange(4000), 8)
    assert np.bincount(a, minlength=8).min() > 400          # every bucket near 500
    assert not np.array_equal(a, R.draw(k, 124, 0, np.arange(4000), 8))
    assert not np.array_equal(a, R.draw(k, 123, 1, np.arange(4000), 8))
    assert not np.array_equal(a, R.draw(k + 1, 123, 0, np.arange(4000), 8))


def test_replay_records_small_case():
    """The replay on a KG small enough to read: relation 1 has one subject (no
    s-corruption under TYPED / LCWA), LCWA's o' is RANDOM's, every negative is
    in its pool and not a training triple."""
    off = np.array([0, 3, 5, 6, 8, 10, 12, 12, 12])       # 4 relations' pools, relation 3 absent
    ent = np.array([0, 2, 4, 1, 3, 5, 6, 7, 8, 10, 9, 11])
    perm = np.arange(len(XS))[::-1]
    known = set(XS)
    out = {k: R.replay_records(k, XS, perm, 1, 0, None if k == R.RANDOM else (off, ent), 100, N)
           for k in (R.RANDOM, R.TYPED, R.LCWA)}
    assert np.array_equal(out[R.LCWA][1], out[R.RANDOM][1])
    for k, (rec, n1) in out.items():
        assert [tuple(r) for r in rec[:, :3].tolist()] == XS[::-1]
        for (s, o, p, a), b in zip(rec.tolist(), n1.tolist()):
            assert a < 0 or (a, o, p) not in known
            assert b < 0 or (s, b, p) not in known
            subj, obj = ent[off[2 * p]:off[2 * p + 1]], ent[off[2 * p + 1]:off[2 * p + 2]]
            can0 = any((c, o, p) not in known for c in subj.tolist())
            can1 = any((s, c, p) not in known for c in obj.tolist())
            if k != R.RANDOM:
                assert a < 0 or a in subj
                assert can0 or a < 0
            if k == R.TYPED:   # pools of 1-3 entries, 100 tries: found wherever one exists
                assert (a >= 0) == can0 and (b >= 0) == can1
                assert b < 0 or b in obj
    # relation 0's three positives and (8, 11, 2): (8, 9, 2) and (10, 9, 2) share
    # their object, relation 1 has one subject
    assert (out[R.TYPED][0][:, 3] >= 0).sum() == 4
