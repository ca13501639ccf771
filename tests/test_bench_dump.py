"""bench.dump_outputs (host logic, no GPU): `--dump-outputs DIR` writes every
array as DIR/<name>.npy in float32 / float64, whole while the files fit the
byte budget, else the largest arrays cut to a fixed seeded sample -- the same
element positions in every run, so two builds compare output for output."""
import os

import numpy as np

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_written_whole(tmp_path):
    rs = np.random.RandomState(1)
    arrays = {"E": rs.rand(7, 5).astype(np.float32), "R": rs.rand(3, 5),
              "nviol": np.array([12], dtype=np.int64)}
    bench.dump_outputs(str(tmp_path / "o"), arrays)
    got = _load(str(tmp_path / "o"))
    assert sorted(got) == ["E", "R", "nviol"]
    assert got["E"].dtype == np.float32 and np.array_equal(got["E"], arrays["E"])
    assert got["R"].dtype == np.float64 and np.array_equal(got["R"], arrays["R"])
    assert got["nviol"].dtype == np.float64 and got["nviol"].tolist() == [12.0]


def test_large_outputs_sampled_within_budget_and_repeatable(tmp_path):
    rs = np.random.RandomState(2)
    big1 = rs.rand(100, 10).astype(np.float32)      # 4000 B
    big2 = rs.rand(90, 10).astype(np.float32)       # 3600 B
    small = rs.rand(4, 10).astype(np.float32)       # 160 B
    arrays = {"E": big1, "E_state": big2, "R": small}
    budget = 6000
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), arrays, budget=budget)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(v.nbytes for v in a.values()) <= budget
    assert np.array_equal(a["R"], small)             # below its share: whole
    for k in ("E", "E_state"):                       # both cut, to an equal share
        assert a[k].ndim == 1 and a[k].size == (budget - small.nbytes) // 2 // 4
        assert np.array_equal(a[k], b[k])            # the same positions every run
        src = arrays[k].reshape(-1)
        assert np.all(np.isin(a[k], src))
    # the sample follows the data: another build's values at the same positions
    bench.dump_outputs(str(tmp_path / "c"), {"E": big1 + 1, "E_state": big2, "R": small},
                       budget=budget)
    assert np.array_equal(_load(str(tmp_path / "c"))["E"], a["E"] + 1)


def test_only_the_largest_is_cut_when_that_suffices(tmp_path):
    big = np.arange(1000, dtype=np.float64)          # 8000 B
    mid = np.arange(100, dtype=np.float64)           # 800 B
    bench.dump_outputs(str(tmp_path / "o"), {"big": big, "mid": mid}, budget=4800)
    got = _load(str(tmp_path / "o"))
    assert np.array_equal(got["mid"], mid)
    assert got["big"].size == 500 and np.all(np.diff(got["big"]) > 0)
