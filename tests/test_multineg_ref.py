"""The host replay of n negatives per positive over any modes
(tests/multineg_ref.py), checked on the CPU: at (1, [0, 1]) it is
sampler_ref.replay_records column for column; every negative passes its kind's
acceptance rule, re-checked by brute force against the triples; a slot is -1
only where all ntries candidates fail; slots are rep-major; and the shared KG
is the one the GPU tests' docstrings describe."""
import numpy as np
import pytest

import multineg_ref as MR
import sampler_ref as R

KINDS = [R.RANDOM, R.TYPED, R.LCWA]


def _subjects(p):
    return set(x[0] for x in MR.XS if x[2] == p)


def _objects(p):
    return set(x[1] for x in MR.XS if x[2] == p)


def test_kg_is_the_one_described():
    assert len(MR.XS) == len(MR.KNOWN) == MR.T == 299 and MR.T % 3 != 0
    assert max(max(x[:2]) for x in MR.XS) < MR.N == 60 and MR.M == 5
    assert set(x[2] for x in MR.XS) == {0, 1, 2, 3} and MR.REL_RANGE == 4 < MR.M
    assert all((s, o, 0) in MR.KNOWN for s in range(6) for o in range(6))
    assert sum(1 for x in MR.XS if x[2] == 0) == 36
    assert any(s == o for s, o, _ in MR.XS)                       # a self-loop
    assert MR.OFF[8] == MR.OFF[9] == MR.OFF[10] == len(MR.ENT)    # relation 4: empty pools
    for key in (0, 5):
        assert sorted(MR.perm_of(key).tolist()) == list(range(MR.T))
    # one try: some slots stay -1, and at (1, [0]) a few positives lose every slot
    pos, neg = MR.kg_replay(R.RANDOM, 3, [0, 1], 1, 0)
    assert 0 < (neg < 0).sum() < neg.size / 4
    _, one = MR.kg_replay(R.RANDOM, 1, [0], 1, 0)
    # (a block positive misses with probability 6/60; any other with about
    # 2.4/60, its own s and the ~1.4 other subjects of its (o, p): ~14 expected)
    assert 1 <= (one < 0).all(axis=1).sum() <= 40
    # (3, [0, 1]): a positive with two equal negatives, and one with s' == o
    pos, neg = MR.kg_replay(R.RANDOM, 3, [0, 1], 100, 0)
    s_neg = neg[:, 0::2]
    assert any(len(set(r)) < 3 for r in s_neg.tolist())
    assert (s_neg == pos[:, 1:2]).any()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ntries", [1, 100])
def test_one_negative_per_mode_is_the_record_replay(kind, ntries):
    perm = MR.perm_of(5)
    rec, n1 = R.replay_records(kind, MR.XS, perm, MR.SEED, 5, (MR.OFF, MR.ENT), ntries, MR.N)
    pos, neg = MR.kg_replay(kind, 1, [0, 1], ntries, 5)
    assert np.array_equal(pos, rec[:, :3])
    assert np.array_equal(neg[:, 0], rec[:, 3]) and np.array_equal(neg[:, 1], n1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,modes", MR.CASES)
@pytest.mark.parametrize("ntries", [1, 100])
def test_negatives_pass_their_kinds_rule_and_miss_only_when_every_try_fails(kind, n, modes,
                                                                            ntries):
    key = 0
    pos, neg = MR.kg_replay(kind, n, modes, ntries, key)
    assert np.array_equal(pos, np.asarray(MR.XS)[MR.perm_of(key)])
    assert neg.shape == (MR.T, n * len(modes))
    skey = R.epoch_sample_key(MR.SEED, key)
    rel_range = MR.REL_RANGE if kind == R.TYPED else MR.M

    def ok(x, mode, c):   # the rule, by brute force over the triples
        s, o, p = MR.negative_triple(x, mode, c)
        if any(t == (s, o, p) for t in MR.XS):
            return False
        if kind == R.LCWA:
            return any(t[0] == s and t[2] == p for t in MR.XS)
        if kind == R.TYPED and mode < 2:
            return c in (_subjects(p) if mode == 0 else _objects(p))
        return True

    found = 0
    for j in range(MR.T):
        x = tuple(pos[j].tolist())
        for k in range(neg.shape[1]):
            mode = modes[k % len(modes)]       # rep-major: slot k = rep * len(modes) + mi
            c = int(neg[j, k])
            cands = MR.candidates(kind, skey, j, k, mode, x, (MR.OFF, MR.ENT), ntries, MR.N, MR.M,
                                  rel_range)
            cands = [] if cands is None else [int(v) for v in cands]
            if mode == 2:
                assert all(0 <= v < rel_range for v in cands)
            if c < 0:
                assert not any(ok(x, mode, v) for v in cands), (j, k)
            else:
                found += 1
                assert ok(x, mode, c), (j, k, c)
                first = next(v for v in cands if ok(x, mode, v))
                assert c == first, (j, k)
    assert found > 0


def test_slot_field_is_the_slot_not_the_mode():
    """(4, [1, 0, 0]): slots 1 and 2 of a repetition are both mode 0 and draw
    different candidates; slot k of (1, [0, 1]) is slot k of (3, [0, 1])."""
    _, a = MR.kg_replay(R.RANDOM, 4, [1, 0, 0], 100, 0)
    assert (a[:, 1] != a[:, 2]).any()
    _, b = MR.kg_replay(R.RANDOM, 3, [0, 1], 100, 0)
    _, c = MR.kg_replay(R.RANDOM, 1, [0, 1], 100, 0)
    assert np.array_equal(b[:, :2], c)
