"""bench.py's plain run vs --full, and --dump-outputs: what the timed path computed, as .npy files of float32 / float64."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, REPO)


class _FakeEngine:
    """Engine.roots() of n slots with A actions, filled from a seed."""

    def __init__(self, n, A, seed=0):
        self.n_slots = n
        rs = np.random.RandomState(seed)
        self._r = dict(priors=rs.rand(n, A), total_value=rs.randn(n, A).astype(np.float32),
                       visits=rs.randint(0, 800, (n, A)).astype(np.int32), changed=np.zeros((n, A), np.int32),
                       stats=rs.randint(0, 9000, (n, 3)).astype(np.int32), q=rs.randn(n).astype(np.float32),
                       root_tv=rs.randn(n).astype(np.float32), root_nv=rs.randint(1, 900, n).astype(np.int32))
        self.edges = rs.randint(0, 1 << 62, (n, 4), dtype=np.int64).astype(np.uint64)

    def roots(self):
        return self._r

    def root_states(self):
        return dict(edges=self.edges)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_writes_every_slot_as_float(tmp_path):
    import bench
    e = _FakeEngine(64, 98)
    bench.dump_outputs(e, str(tmp_path))
    got = _load(str(tmp_path))
    assert set(got) == {"root_priors", "root_total_value", "root_visits", "root_stats", "root_q", "root_tv", "root_nv", "root_ply",
                        "slot"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    r = e.roots()
    assert np.array_equal(got["slot"], np.arange(64)) and np.array_equal(got["root_visits"], r["visits"])
    assert np.array_equal(got["root_priors"], r["priors"]) and np.array_equal(got["root_nv"], r["root_nv"])
    assert np.array_equal(got["root_ply"], [sum(bin(int(w)).count("1") for w in row) for row in e.edges])


def test_dump_samples_a_fixed_subset_above_the_limit(tmp_path):
    import bench
    e = _FakeEngine(1000, 98)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(e, a, limit=200_000)
    bench.dump_outputs(e, b, limit=200_000)
    ga, gb = _load(a), _load(b)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 200_000  # the .npy headers included
    slots = ga["slot"].astype(np.int64)
    assert 0 < len(slots) < 1000 and np.all(np.diff(slots) > 0) and np.array_equal(slots, gb["slot"])
    assert np.array_equal(ga["root_total_value"], e.roots()["total_value"][slots])


def test_dump_outputs_is_refused_outside_the_step_benchmark(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--train-data", "10", "--dump-outputs", str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr and not os.listdir(str(tmp_path))


_TINY = ["--gpus", "1", "--steps", "6", "--warmup", "2", "--board", "3", "--slots", "256", "--sims", "50", "--channels", "32",
         "--blocks", "2"]


def _bench(*flags):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + _TINY + list(flags), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_roots(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path))
    assert d["metric"] == "mcts_node_expansions_per_sec" and d["unit"] == "expansions/s" and d["higher_is_better"] is True
    assert d["steps"] == 6 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0 and "dtype" in d
    assert not {"cpu_baseline", "games_leg", "games_per_sec", "exact_f32_mode"} & set(d)
    got = _load(str(tmp_path))
    assert got["root_visits"].shape == (256, 32) and np.array_equal(got["slot"], np.arange(256))
    assert np.all(got["root_nv"] >= 0) and np.all(np.isfinite(got["root_priors"]))
    assert np.all(got["root_visits"] >= 0) and np.all((got["root_ply"] >= 0) & (got["root_ply"] <= 24))  # 3x3: 24 edges


@pytest.mark.gpu
def test_full_run_adds_the_games_leg_and_the_f32_side_run():
    d = _bench("--full", "--no-cpu-baseline")
    assert d["steps"] == 6 and d["value"] > 0
    assert d["games_leg"]["games"] == 256 and d["games_per_sec"] > 0
    assert d["exact_f32_mode"]["value"] > 0 and "cpu_baseline" not in d


@pytest.mark.gpu
def test_two_runs_dump_the_same_outputs(tmp_path):
    """Same arguments, same arrays: the leaves behind the network's full-rounds cut and the games handed to slots whose game
    ended follow the slot order, not the order in which workgroups finish (4 096 slots: more than one round of the network;
    3x3 games end during the preparation steps)."""
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for d in (a, b):
        _bench("--slots", "4096", "--steps", "30", "--dump-outputs", d)
    ga, gb = _load(a), _load(b)
    assert set(ga) == set(gb) and ga["slot"].shape == (4096,)
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
