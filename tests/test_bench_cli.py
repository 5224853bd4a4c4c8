"""bench.py's command line: --dump-outputs writes the last timed step's results, a plain run
carries no side measurements, --full brings them back.

CPU: the dump writer (float64 files, the 64 MB cap as a fixed seeded sample) and the options.
GPU: one small plain run with a dump, checked against the C oracle on the same seeded window, and
one small --full run.
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_geohip_bench", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_writes_float64_files(bench, tmp_path):
    arrays = {"idx": np.arange(7, dtype=np.int32), "dist": np.linspace(0.0, 1.0, 7),
              "pairs": np.arange(10, dtype=np.int64).reshape(5, 2), "count": np.array([7])}
    bench.dump_outputs(tmp_path / "d", arrays)
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == ["count.npy", "dist.npy", "idx.npy", "pairs.npy"]
    for name, a in arrays.items():
        got = np.load(tmp_path / "d" / f"{name}.npy")
        assert got.dtype == np.float64 and got.shape == a.shape and np.array_equal(got, a)


def test_dump_over_the_cap_is_a_fixed_sample(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 8 * 1000)
    arrays = {"x": np.arange(3000, dtype=np.float64), "pairs": np.arange(4000, dtype=np.int64).reshape(2000, 2)}
    bench.dump_outputs(tmp_path / "a", arrays)
    bench.dump_outputs(tmp_path / "b", arrays)
    total = 0
    for name, a in arrays.items():
        got = np.load(tmp_path / "a" / f"{name}.npy")
        assert np.array_equal(got, np.load(tmp_path / "b" / f"{name}.npy"))  # the same rows every time
        assert got.dtype == np.float64 and 0 < len(got) < len(a) and got.shape[1:] == a.shape[1:]
        # rows of the output, in their own order
        first = got if got.ndim == 1 else got[:, 0]
        assert np.all(np.diff(first) > 0) and np.all(np.isin(first, a if a.ndim == 1 else a[:, 0]))
        total += got.nbytes
    assert total <= 8 * 1000


def test_sorted_forms(bench):
    assert bench._sorted_set(np.array([5, 1, 3], np.int32)).tolist() == [1, 3, 5]
    assert bench._sorted_pairs(np.array([[2, 1], [1, 9], [1, 3]], np.int32)).tolist() == [[1, 3], [1, 9], [2, 1]]
    assert bench._sorted_pairs(np.zeros((0, 2), np.int32)).shape == (0, 2)


def test_options(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 1, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def _run_bench(*args):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", *args], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


SIDE = ("partition_cells", "e2e", "pipelined")


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_topk(tmp_path):
    import cref
    from spatialflink_amd import synth
    n, steps, warmup = 200_000, 3, 2
    res = _run_bench("--steps", str(steps), "--warmup", str(warmup), "--points", str(n),
                     "--dump-outputs", str(tmp_path / "d"))
    assert res["steps"] == steps and res["warmup"] == warmup and res["ms_per_step"] > 0
    assert res["unit"] == "points/sec" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert abs(res["value"] - n / (res["ms_per_step"] * 1e-3)) <= 1e-6 * res["value"]
    assert res["cpu_baseline"] is None and res["counts_verified"] is None and not any(k in res for k in SIDE)
    # the window of the last timed step (bench.KnnWorkload: 4 resident windows, seed 2 + 7919 w)
    w = (warmup + steps - 1) % 4
    x, y = synth.uniform(n, 2 + 7919 * w)
    bj, q = synth.BEIJING, synth.README_QUERY
    wi, wd = cref.knn_pp(cref.grid(bj[0], bj[2], (bj[1] - bj[0]) / 100, 100), x, y, q[0], q[1], 0.5, 50)
    gi, gd = np.load(tmp_path / "d" / "knn_idx.npy"), np.load(tmp_path / "d" / "knn_dist.npy")
    assert gi.dtype == gd.dtype == np.float64
    assert gi.tolist() == wi.tolist()
    assert np.array_equal(gd.view(np.uint64), wd.view(np.uint64))


@pytest.mark.gpu
def test_full_run_keeps_the_side_measurements():
    res = _run_bench("--steps", "4", "--warmup", "1", "--points", "200000", "--full", "--cpu-seconds", "0.2")
    assert res["counts_verified"] is True
    assert res["cpu_baseline"]["value"] > 0
    assert all(k in res for k in SIDE)
    assert res["e2e"]["matches_device_path"] and res["pipelined"]["matches_sequential"]
    assert res["partition_cells"]["matches_arrival_sharding"]
