"""bench.py's plain run and --dump-outputs: the plain run measures the
headline only (the other legs wait for --full), and the dump holds the last
timed step's arrays, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
NAMES = ("normals", "rep_idx", "rep_xyz", "rows")


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def _fake_out(m):
    g = torch.Generator().manual_seed(1)
    return {"rep_idx": torch.arange(m, dtype=torch.int32) * 3, "rep_xyz": torch.rand((m, 3), generator=g),
            "normals": torch.rand((m, 3), generator=g), "voxel_grid": None}


def _load(d):
    assert sorted(os.listdir(d)) == [n + ".npy" for n in NAMES]
    return {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}


def test_dump_outputs_small_holds_every_row(tmp_path):
    bench = _bench()
    out = _fake_out(1001)
    bench.dump_outputs(str(tmp_path / "d"), out)
    got = _load(tmp_path / "d")
    assert got["rows"].dtype == np.float64 and np.array_equal(got["rows"], np.arange(1001))
    assert got["rep_idx"].dtype == np.float64 and np.array_equal(got["rep_idx"], out["rep_idx"].numpy())
    for n in ("rep_xyz", "normals"):
        assert got[n].dtype == np.float32 and np.array_equal(got[n], out[n].numpy())


def test_dump_outputs_large_is_a_fixed_sample_within_budget(tmp_path):
    bench = _bench()
    m = bench.DUMP_BUDGET_BYTES // 40 + 12345  # just past the size at which the dump turns to sampling
    out = _fake_out(m)
    bench.dump_outputs(str(tmp_path / "a"), out)
    bench.dump_outputs(str(tmp_path / "b"), out)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    size = sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in NAMES)
    assert size <= 64 * 10 ** 6
    rows = a["rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_BUDGET_BYTES // 40 and rows[0] >= 0 and rows[-1] < m
    assert (np.diff(rows) > 0).all()  # sorted, no row twice
    assert np.array_equal(a["rep_idx"], out["rep_idx"].numpy()[rows])
    for n in ("rep_xyz", "normals"):
        assert np.array_equal(a[n], out[n].numpy()[rows])
    for n in NAMES:
        assert np.array_equal(a[n], b[n])


def test_dump_outputs_is_a_one_gpu_option():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--dump-outputs", "unused"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_dumps_repeat(tmp_path):
    lines = []
    for tag in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--n", "200000",
                            "--dump-outputs", str(tmp_path / tag)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1
        lines.append(json.loads(out[0]))
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "Mpoints/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(200000 / d["ms_per_step"] / 1e3, rel=0.02)
    assert d["cpu_baseline"] is None
    for leg in ("icp", "ransac", "c4_single_gpu", "c5_single_gpu", "f64_las", "cpu_icp"):
        assert leg not in d["extra"]
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    m = d["config"]["voxels"]
    assert a["rep_idx"].shape == (m,) and a["rep_xyz"].shape == (m, 3) and a["normals"].shape == (m, 3)
    assert np.allclose(np.linalg.norm(a["normals"], axis=1), 1.0, atol=1e-5)
    for n in NAMES:
        assert np.array_equal(a[n], b[n])
