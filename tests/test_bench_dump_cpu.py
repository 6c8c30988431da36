"""
CPU tier: bench.py's --dump-outputs writer (bench.dump_outputs) on host arrays shaped like a swarm's state -- what
it writes, in which dtype, and that a swarm too large for the 64 MB budget is written as a fixed, seeded sample of
its particles.  The GPU run that feeds it the real swarm is tests/test_gpu_bench_paths.py.
"""
import os

import numpy as np

import bench


def _state(S, D, seed=0):
    rng = np.random.default_rng(seed)
    return {"x": rng.standard_normal((S, D)), "v": rng.standard_normal((S, D)), "p": rng.standard_normal((S, D)),
            "fx": rng.random(S), "fp": rng.random(S)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_writes_the_whole_swarm_as_float64(tmp_path):
    st = _state(64, 22)
    best = (st["p"][5].copy(), float(st["fp"][5]))
    names = bench.dump_outputs(str(tmp_path), st, best)
    got = _load(str(tmp_path))
    assert sorted(names) == sorted(got) == sorted(["positions", "velocities", "personal_best_positions", "objective",
                                                   "personal_best_objective", "particle_index", "global_best_position",
                                                   "global_best_objective"])
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["positions"], st["x"])
    np.testing.assert_array_equal(got["velocities"], st["v"])
    np.testing.assert_array_equal(got["personal_best_positions"], st["p"])
    np.testing.assert_array_equal(got["objective"], st["fx"])
    np.testing.assert_array_equal(got["personal_best_objective"], st["fp"])
    np.testing.assert_array_equal(got["particle_index"], np.arange(64))
    np.testing.assert_array_equal(got["global_best_position"], best[0])
    assert got["global_best_objective"].shape == (1,) and got["global_best_objective"][0] == best[1]


def test_dump_samples_a_large_swarm_within_the_budget(tmp_path):
    S, D = 40000, 76                      # 40000 x (3 x 76 + 3) doubles: 74 MB, over the budget
    st = _state(S, D)
    best = (st["p"][0].copy(), float(st["fp"][0]))
    runs = []
    for k in range(2):
        d = tmp_path / str(k)
        bench.dump_outputs(str(d), st, best)
        total = sum(os.path.getsize(os.path.join(str(d), f)) for f in os.listdir(str(d)))
        assert total <= bench.DUMP_BUDGET_BYTES
        runs.append(_load(str(d)))
    a, b = runs
    idx = a["particle_index"].astype(np.int64)
    assert 0 < idx.size < S and np.all(np.diff(idx) > 0)           # a sorted subset of distinct particles ...
    for name in a:                                                  # ... the same one on every run
        np.testing.assert_array_equal(a[name], b[name])
    np.testing.assert_array_equal(a["positions"], st["x"][idx])
    np.testing.assert_array_equal(a["personal_best_objective"], st["fp"][idx])


def test_dump_of_a_rank_names_its_shard(tmp_path):
    st = _state(8, 13)
    best = (st["p"][0].copy(), float(st["fp"][0]))
    bench.dump_outputs(str(tmp_path / "r0"), st, best, rank=0, world=2, offset=0)
    bench.dump_outputs(str(tmp_path / "r1"), st, best, rank=1, world=2, offset=8)
    r0, r1 = _load(str(tmp_path / "r0")), _load(str(tmp_path / "r1"))
    assert "positions_rank0" in r0 and "global_best_position" in r0
    assert "positions_rank1" in r1 and "global_best_position" not in r1
    np.testing.assert_array_equal(r1["particle_index_rank1"], np.arange(8, 16))
