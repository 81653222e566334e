"""bench.py's own contract: a plain run times exactly --steps frames and carries the headline only (everything else is --full),
and --dump-outputs writes the cloud the timed path returned in its last step, field by field, in float32 / float64."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")


def _records(n, seed=3):
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, 8), np.float32)
    pts[:, :3] = rng.normal(size=(n, 3)).astype(np.float32)
    pts[:, 4] = 64.0
    pts[:, 5] = (np.arange(n, dtype=np.int32) % 128).view(np.float32)
    hits = np.zeros((n, 4), np.uint32)
    hits[:, 0] = np.sort(rng.choice(1 << 31, size=n, replace=False))
    hits[:, 1] = np.arange(n) % 3
    hits[:, 2] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    hits[:, 3] = rng.uniform(0.5, 90.0, size=n).astype(np.float32).view(np.uint32)
    return pts, hits


def test_dump_outputs_writes_every_field_exactly(tmp_path, monkeypatch):
    import bench
    pts, hits = _records(1000)
    rec = bench.dump_outputs(str(tmp_path), pts.view(np.uint8), hits)
    assert rec["points"] == 1000 and not rec["sampled"]
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"n_points", "points_xyz", "points_intensity", "points_ring", "hits_ray", "hits_geom", "hits_prim", "hits_t"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["n_points"].tolist() == [1000]
    assert np.array_equal(got["points_xyz"], pts[:, :3]) and np.all(got["points_intensity"] == 64.0)
    assert np.array_equal(got["points_ring"], pts[:, 5].view(np.int32).astype(np.float64))
    for i, k in enumerate(("hits_ray", "hits_geom", "hits_prim")):   # u32 exactly, above 2**31 included
        assert np.array_equal(got[k], hits[:, i].astype(np.float64))
    assert np.array_equal(got["hits_t"], hits[:, 3].view(np.float32))
    # the same records as flat bytes (how the single-GPU path hands them over): the same files
    bench.dump_outputs(str(tmp_path / "flat"), pts.view(np.uint8).reshape(-1), hits.view(np.uint8).reshape(-1))
    for k, a in got.items():
        assert np.array_equal(np.load(tmp_path / "flat" / (k + ".npy")), a), k
    # over the size limit: the same seeded sample every time, in ray order, and the indices it kept
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 600 * 52)
    a = bench.dump_outputs(str(tmp_path / "a"), pts.view(np.uint8), hits)
    b = bench.dump_outputs(str(tmp_path / "b"), pts.view(np.uint8), hits)
    assert a["sampled"] and b["sampled"]
    ia, ib = np.load(tmp_path / "a" / "sample_index.npy"), np.load(tmp_path / "b" / "sample_index.npy")
    assert np.array_equal(ia, ib) and 0 < ia.size < 1000 and np.all(np.diff(ia) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "hits_ray.npy"), hits[ia.astype(np.int64), 0].astype(np.float64))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 600 * 52 + 9 * 256   # (+ .npy headers)


def test_bench_defaults_time_exactly_steps_and_leave_the_rest_to_full(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7"])
    a = bench.parse_args()
    assert a.steps == 7 and a.min_ms == 0.0 and a.full is False and a.dump_outputs is None


@pytest.mark.gpu
def test_plain_run_times_exactly_steps_and_dumps_the_last_frame(tmp_path):
    """A plain run: one window of exactly --steps frames, the headline fields, none of --full's; the dumped cloud is the frame the
    reference's XT-32 x ground + ben test knows (1781 points), equal to the oracle's field by field."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "7", "--warmup", "2", "--workload", "xt32",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["steps"] == 7 and rec["timing"]["windows"] == 1 and rec["timing"]["frames_per_window"] == 7
    assert abs(rec["timing"]["timed_ms_total"] - 7 * rec["ms_per_step"]) < 1e-9 * max(1.0, rec["timing"]["timed_ms_total"])
    for k in ("roofline", "cpu_baseline", "also_measured", "dropin", "stage_ms", "ms_per_step_windows_of_1000", "ms_per_step_one_frame_in_flight"):
        assert k not in rec, k
    assert rec["dump_outputs"]["points"] == 1781 and not rec["dump_outputs"]["sampled"]

    from oracle import oracle as O
    s = O.load_sensor(os.path.join(DATA, "config", "hesai-pandar-XT-32-lidar_0000.json"))
    ground = O.load_stl(os.path.join(DATA, "mesh", "ground.stl"))
    ben = O.load_stl(os.path.join(DATA, "mesh", "ben.stl"))
    ref = O.trace_frame(s, [(0, *ground, O.IDENTITY_AFFINE), (1, *ben, O.IDENTITY_AFFINE)])
    rp = ref["points"].view(np.float32).reshape(-1, 8)
    assert np.load(tmp_path / "n_points.npy").tolist() == [1781]
    assert np.array_equal(np.load(tmp_path / "points_xyz.npy"), rp[:, :3])
    assert np.array_equal(np.load(tmp_path / "points_ring.npy"), rp[:, 5].view(np.int32).astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "hits_ray.npy"), ref["hits"][:, 0].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "hits_geom.npy"), ref["hits"][:, 1].astype(np.float64))
