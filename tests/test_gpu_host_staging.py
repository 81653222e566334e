"""The host-memory variants share one staging buffer (every size of it, one call after the other) and the moving gathers two staged
tables next to each other: interleavings the per-call files do not run.  XT-32 0000 over ground + ben, sharded to columns 0..7 (256
rays).  A call on a handle that has made other calls before must give what the same call gives as the first call of a fresh handle
in the same scene state -- bit for bit."""
import numpy as np
import pytest

from conftest import make_tracer
from test_gpu_format import _velodyne, _times
from test_gpu_rays import _ground_ben
from test_gpu_returns import _full_model
from test_gpu_sweep import _twist_poses

pytestmark = pytest.mark.gpu

TURN = 0.1
REFL = [0.8, 0.6]
GROUND, BEN = 0, 1
MOVED = np.float32([1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 0.125])   # ben, half a metre aside


def _handle(oracle, capi, sensors, meshes, A_ben=None):
    tr = make_tracer(capi, sensors["0000"])
    _ground_ben(tr, oracle, meshes, A_ben)
    tr.setShard(0, 8)
    assert tr.getTotalRays() == 256
    return tr


def _bits(result):
    """the arrays of a call's result as bytes, everything else as it is"""
    items = result if isinstance(result, tuple) else (result,)
    return tuple(np.ascontiguousarray(x).view(np.uint8).reshape(-1).tobytes() if isinstance(x, np.ndarray) else x for x in items)


def _tables(oracle, capi, s, meshes):
    """the sensor's poses on the sweep tests' twist, a slow drift of the ground, ben on a twist about its own centroid"""
    pose = _twist_poses(capi, s)
    drift = capi.motion_constant_twist((0.5, 0.25, 0.0), (0.0, 0.0, 0.02), (0.0, 0.0, 0.0), 0.0, TURN / s.H, s.H)
    pivot = oracle.transform_vertices(meshes["ben"][0], oracle.IDENTITY_AFFINE, s).astype(np.float64).mean(0)
    twist = capi.motion_constant_twist((12.0, -9.0, 0.5), (0.05, -0.1, 0.5), pivot, 0.0, TURN / s.H, s.H)
    return pose, drift, twist


def test_one_staging_buffer_across_calls_and_sizes(oracle, capi, sensors, meshes):
    """16 rays, a sweep frame of the shard with its tables, the gathers over its records, a cloud, the frame again without points
    and without hits, 16 rays again: the buffer grows, then the small calls reuse it"""
    s = sensors["0000"]
    pose, _, twist = _tables(oracle, capi, s, meshes)
    motions = {BEN: twist}
    rays = np.zeros((16, 8), np.float32)
    rays[:, 4:7] = oracle.ray_dirs(s)[np.arange(16, 32) * s.H + 3]   # column 3 of the lower channels
    rays[:, 7] = 1e16
    model = _full_model(capi, range_min=0.0)
    fmt = _velodyne(capi)
    col_time, _ = _times(capi, s)

    tr = _handle(oracle, capi, sensors, meshes)
    first = tr.traceRays(rays)
    frame = tr.traceSweepMoving(pose, motions)
    rc, k, pts, hits = frame
    assert rc == 0 and 16 < k <= 256 and np.count_nonzero(first[1]["geom"] != capi.INVALID) > 0
    calls = [
        ("traceRays", lambda t: t.traceRays(rays), first),
        ("traceSweepMoving", lambda t: t.traceSweepMoving(pose, motions), frame),
        ("hitAttributesMoving", lambda t: t.hitAttributesMoving(hits, pose, motions), None),
        ("applyReturnModelMoving", lambda t: t.applyReturnModelMoving(model, hits, pose, motions, reflectivity=REFL), None),
        ("formatCloud", lambda t: t.formatCloud(fmt, hits, points=pts, echo=None, col_time=col_time), None),
        ("traceSweepMoving without points", lambda t: t.traceSweepMoving(pose, motions, points=False), None),
        ("traceSweepMoving without hits", lambda t: t.traceSweepMoving(pose, motions, hits=False), None),
        ("traceRays again", lambda t: t.traceRays(rays), None),
    ]
    got = [call(tr) if done is None else done for _, call, done in calls]
    tr.close()
    rc, attrs = got[2]
    assert rc == 0 and np.count_nonzero(attrs["flags"] == 1) > 16
    rc, rp, rh = got[3]
    assert rc == 0 and 0 < rh.shape[0] < k
    assert got[4].shape == (k, 22)
    assert got[5][2] is None and got[6][3] is None
    assert _bits(got[5][3]) == _bits(hits) and _bits(got[6][2]) == _bits(pts)
    assert _bits(got[7]) == _bits(first)
    for (name, call, _), mine in zip(calls, got):
        fresh = _handle(oracle, capi, sensors, meshes)
        want = call(fresh)
        fresh.close()
        assert _bits(mine) == _bits(want), name


def test_the_two_staged_tables_interleaved(oracle, capi, sensors, meshes):
    """the gather's table alone, with the motion table of one geometry, of the other, alone again; then the same after ben has
    moved: neither upload may leave the other table stale"""
    s = sensors["0000"]
    pose, drift, twist = _tables(oracle, capi, s, meshes)
    a, b = {GROUND: drift}, {BEN: twist}

    def records(A_ben):
        """the records each call of the sequence is given, traced in this scene state"""
        t = _handle(oracle, capi, sensors, meshes, A_ben)
        rc, _, frame = t.traceScene(0)
        rca, ka, _, ha = t.traceSweepMoving(pose, a)
        rcb, kb, _, hb = t.traceSweepMoving(pose, b)
        t.close()
        assert rc == 0 and rca == 0 and rcb == 0 and min(len(frame), ka, kb) > 16
        return frame, ha, hb

    def sequence(frame, ha, hb):
        return [lambda t: t.hitAttributes(frame), lambda t: t.hitAttributesMoving(ha, pose, a), lambda t: t.hitAttributesMoving(hb, pose, b),
                lambda t: t.hitAttributes(frame)]

    tr = _handle(oracle, capi, sensors, meshes)
    for A_ben in (None, MOVED):
        if A_ben is not None:
            tr.updateGeometryTransform("face", A_ben)
            assert tr.commitScene() == 0
        calls = sequence(*records(A_ben))
        got = [call(tr) for call in calls]
        for i, (call, mine) in enumerate(zip(calls, got)):
            assert mine[0] == 0 and np.count_nonzero(mine[1]["flags"] == 1) > 16
            fresh = _handle(oracle, capi, sensors, meshes, A_ben)
            want = call(fresh)
            fresh.close()
            assert _bits(mine) == _bits(want), (A_ben is not None, i)
        assert _bits(got[0]) == _bits(got[3])
    tr.close()
