"""corruption_load and the count bound's sampler kinds (CPU).

corruption_load gives every entity row its expected corruptions per batch
under the RANDOM, TYPED and LCWA samplers; packed_count_bound uses it, per
row, to choose the packed sums' encoding.  The pools are a hand-built CSR; no
GPU is touched (CPU tensors in, CPU tensor out).
"""
import math
import types

import numpy as np
import pytest
import torch

from skge_amd import _lib as L
from skge_amd import device as DV

N, BATCH, T = 10, 20, 100
# three relations: 0 has subjects {1, 2, 3, 4} and the one object {5};
# 1 has subjects {0, 5} and objects {6, 7}; 2 never occurs (two empty pools)
OFF = torch.tensor([0, 4, 5, 7, 9, 9, 9], dtype=torch.int64)
ENT = torch.tensor([1, 2, 3, 4, 5, 0, 5, 6, 7], dtype=torch.int32)
CNT = torch.tensor([60, 40, 0], dtype=torch.int64)


def _load(kind, cnt=CNT):
    out = DV.corruption_load(kind, OFF, ENT, cnt, N, BATCH, T)
    assert out.dtype == torch.float64 and out.shape == (N,) and out.device.type == "cpu"
    return out.numpy()


def test_typed_pools_share_their_relations_positives():
    got = _load(L.SKGE_SAMPLER_TYPED)
    per0, per1 = 60 * BATCH / T, 40 * BATCH / T     # positives per batch of relations 0 and 1
    want = np.zeros(N)
    want[[1, 2, 3, 4]] += per0 / 4
    want[5] += per0                                  # a one-entity pool: its full share
    want[[0, 5]] += per1 / 2
    want[[6, 7]] += per1 / 2
    np.testing.assert_allclose(got, want, rtol=1e-12)
    assert got[8] == 0.0 and got[9] == 0.0          # in no pool
    # every positive of a relation with non-empty pools draws once per mode
    assert math.isclose(got.sum(), 2 * BATCH, rel_tol=1e-12)


def test_empty_pool_contributes_nothing_whatever_its_count():
    """Relation 2's pools are empty: a count for it (inconsistent with the
    pools, but it must not divide by zero or land on a row) adds nothing."""
    a = _load(L.SKGE_SAMPLER_TYPED)
    b = _load(L.SKGE_SAMPLER_TYPED, torch.tensor([60, 40, 1000]))
    assert np.array_equal(a, b) and np.isfinite(b).all()


def test_lcwa_is_pool_2p_plus_the_uniform_mode_1():
    got = _load(L.SKGE_SAMPLER_LCWA)
    want = np.full(N, BATCH / N)                     # mode 1: uniform over the entities
    want[[1, 2, 3, 4]] += 60 * BATCH / T / 4
    want[[0, 5]] += 40 * BATCH / T / 2
    np.testing.assert_allclose(got, want, rtol=1e-12)
    assert math.isclose(got[8], BATCH / N) and math.isclose(got[6], BATCH / N)   # object pools: none
    assert math.isclose(got.sum(), 2 * BATCH, rel_tol=1e-12)


def test_random_is_uniform_over_the_entities():
    got = _load(L.SKGE_SAMPLER_RANDOM)
    assert np.array_equal(got, np.full(N, 2.0 * BATCH / N))
    assert math.isclose(got.sum(), 2 * BATCH, rel_tol=1e-12)
    # RANDOM reads no pools
    assert np.array_equal(DV.corruption_load(L.SKGE_SAMPLER_RANDOM, None, None, None, N, BATCH,
                                             T).numpy(), got)


def test_unknown_kind_and_short_offsets_are_refused():
    with pytest.raises(ValueError, match="kind"):
        DV.corruption_load(7, OFF, ENT, CNT, N, BATCH, T)
    with pytest.raises(ValueError, match="pool_off"):
        DV.corruption_load(L.SKGE_SAMPLER_TYPED, OFF[:-2], ENT, CNT, N, BATCH, T)


def _random_kg(n_ent, n_rel, T, seed):
    rs = np.random.RandomState(seed)
    # skewed subjects, so the binomial tail and the min() both take part
    s = np.minimum(rs.zipf(1.3, T) - 1, n_ent - 1)
    trip = np.stack([s, rs.randint(n_ent, size=T), rs.randint(n_rel, size=T)], axis=1)
    return types.SimpleNamespace(trip=torch.tensor(trip, dtype=torch.int32))


def _old_bound(trip, n_ent, batch, tail):
    """packed_count_bound as it was before it took a sampler, restated."""
    T = float(max(len(trip), 1))
    B = float(min(int(batch), len(trip)))

    def per_batch(col):
        c = np.bincount(col, minlength=n_ent).astype(np.float64)
        return np.minimum(np.minimum(c, B), tail(c * (B / T)))
    occ = per_batch(trip[:, 0]) + per_batch(trip[:, 1])
    det = 3 * min(int(math.ceil(float(occ.max()))), 2 * int(batch))
    lam = 2.0 * batch / max(n_ent, 1)
    return det + min(2 * int(batch), int(math.ceil(tail(lam))))


@pytest.mark.parametrize("n_ent,T,batch", [(50, 400, 40), (1000, 5000, 5000), (7, 30, 3)])
def test_random_kind_bound_is_the_old_formula(n_ent, T, batch):
    kg = _random_kg(n_ent, 3, T, seed=n_ent)
    trip = kg.trip.numpy().astype(np.int64)
    for tail, old_tail in ((None, lambda m: m + 12.0 * m ** 0.5 + 40.0),
                           (DV._tail8, lambda m: m + 8.0 * m ** 0.5 + 20.0)):
        want = _old_bound(trip, n_ent, batch, old_tail)
        assert DV.packed_count_bound(kg, n_ent, batch, tail) == want
        assert DV.packed_count_bound(kg, n_ent, batch, tail, sampler=L.SKGE_SAMPLER_RANDOM,
                                     n_rel=3) == want


def _pools(xs, n_rel):
    off, ent = [0], []
    for p in range(n_rel):
        for side in (0, 1):
            ent += sorted(set(x[side] for x in xs if x[2] == p))
            off.append(len(ent))
    return torch.tensor(off, dtype=torch.int64), torch.tensor(ent, dtype=torch.int32)


def test_pool_kind_bound_is_per_row():
    """Row 0 has the most occurrences (7, in a subject pool of seven), rows 8
    and 9 -- relation 1's two-entity object pool -- the largest load (12 / 2):
    the bound is the largest per-row sum, below the sum of the two maxima."""
    xs = [(0, o, 0) for o in range(1, 8)] + [(s, s - 1, 0) for s in range(2, 8)]
    xs += [(s, o, 1) for s in range(1, 7) for o in (8, 9)]
    n_ent, n_rel, batch = 10, 2, len(xs)
    off, ent = _pools(xs, n_rel)
    kg = types.SimpleNamespace(trip=torch.tensor(xs, dtype=torch.int32),
                               pools=lambda n: (off, ent))
    ident = lambda m: m                              # no tail: the arithmetic alone
    load = DV.corruption_load(L.SKGE_SAMPLER_TYPED, off, ent, torch.tensor([13, 12]), n_ent,
                              batch, len(xs)).numpy()
    occ = np.bincount(np.asarray(xs)[:, :2].ravel(), minlength=n_ent)
    assert occ.argmax() == 0 and occ[0] == 7 and load.argmax() in (8, 9) and load[8] == 6.0
    want = int(max(3 * occ[i] + math.ceil(load[i]) for i in range(n_ent)))
    got = DV.packed_count_bound(kg, n_ent, batch, ident, sampler=L.SKGE_SAMPLER_TYPED, n_rel=n_rel)
    assert got == want == 24
    assert got < 3 * occ.max() + math.ceil(load.max())
    with pytest.raises(ValueError, match="relation count"):
        DV.packed_count_bound(kg, n_ent, batch, sampler=L.SKGE_SAMPLER_TYPED)
