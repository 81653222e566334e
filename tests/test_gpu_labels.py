"""ls_object_labels / ls_object_labels_host on the MI355X: per-geometry counts, t ranges and boxes of hit records against the numpy
reduction of tests/labels_reference.py, bit for bit, and the footprint (n_alone: the rays that hit a geometry taken alone) against
the brute force over each one-geometry scene -- frame records on both engines, arbitrary rays, a hidden object, more geometries than
one launch takes, ranges and degenerate rays, and the entry points' plumbing."""
import ctypes

import numpy as np
import pytest

import labels_reference as ref
from conftest import make_tracer
from test_gpu_rays import INV, _add, _ground_ben, _random_rays, _records, _scene_posed_quads

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = -2                      # LS_ERR_INVALID_ARGUMENT
OUT_OF_RANGE = -9                          # LS_ERR_OUT_OF_RANGE
FRAME_EAGER = 0                            # LS_FRAME_EAGER
GUARD = 256

# torch fills a new tensor on its own stream, the library works on the handle's: every buffer is filled (a device-wide
# synchronize) before the library gets it


def _geoms(ml):
    """{geomID: element count} of a mesh list"""
    return {int(m[0]): int(np.asarray(m[2]).shape[0]) for m in ml}


def _xyz(points32):
    return np.ascontiguousarray(np.ascontiguousarray(points32).reshape(-1, 32)[:, :12]).view(np.float32).reshape(-1, 3)


def _xyz_of_sensor_rays(oracle, s, rec):
    """t * d in float32, one product per axis, for records of the sensor's own rays (others: 0)"""
    d = oracle.ray_dirs(s)
    p = np.zeros((rec.shape[0], 3), np.float32)
    ok = rec[:, 0] < d.shape[0]
    with np.errstate(all="ignore"):
        p[ok] = (rec[ok, 3].view(np.float32)[:, None] * d[rec[ok, 0]]).astype(np.float32)
    return p


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    for name in want.dtype.names:
        assert np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), name
    assert got.tobytes() == want.tobytes()


def _to_device(a):
    import torch
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(b.copy()).to("cuda:0") if b.size else torch.zeros(16, dtype=torch.uint8, device="cuda:0")


def _labels_device(tr, capi, n_labels, records=None, rays=None, footprint=True, count=None, stream=None):
    """ls_object_labels on device buffers, 0xAB behind the n_labels records -> OBJECT_LABEL_DTYPE[n_labels]"""
    import torch
    n = 0 if records is None else np.asarray(records).reshape(-1, 4).shape[0]
    d_hits = _to_device(np.asarray(records, np.uint32)) if n else None
    d_rays = None if rays is None else _to_device(np.ascontiguousarray(rays, np.float32))
    d_count = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda:0")
    out = torch.full((n_labels * 64 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = tr.objectLabelsDevice(out.data_ptr(), n_labels, d_hits.data_ptr() if n else 0, n, 0 if rays is None else d_rays.data_ptr(),
                               0 if rays is None else np.asarray(rays).reshape(-1, 8).shape[0], 0 if count is None else d_count.data_ptr(),
                               footprint, stream)
    assert rc == 0
    tr.synchronize()
    torch.cuda.synchronize()
    b = out.cpu().numpy()
    assert np.all(b[n_labels * 64:] == 0xAB)
    return b[:n_labels * 64].copy().view(capi.OBJECT_LABEL_DTYPE)


def _check_ties(lab, rec, ok):
    """ray_min / ray_max: the lowest ray among the counted records that hold the extreme t"""
    for g in range(lab.shape[0]):
        m = ok & (rec[:, 1] == g)
        if not np.any(m):
            assert lab["n_hits"][g] == 0 and lab["ray_min"][g] == INV and lab["ray_max"][g] == INV
            continue
        t = rec[m, 3].view(np.float32)
        assert lab["t_min"][g] == t.min() and lab["ray_min"][g] == rec[m, 0][t == t.min()].min()
        assert lab["t_max"][g] == t.max() and lab["ray_max"][g] == rec[m, 0][t == t.max()].min()


# ---- 1. frame records ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine", ["projection", "bvh"])
def test_frame_records_equal_the_reference_reduction(oracle, capi, sensors, meshes, engine):
    """sensor 0000 over ground + ben (1781 points) and over the posed scene with quads: objectLabels(hits) is the reduction over the
    frame's own points32 xyz, bit for bit; the counts add up to the frame; the footprint of the sensor's rays is the oracle's frame
    over each geometry alone"""
    s = sensors["0000"]
    for k, setup in enumerate((lambda tr: _ground_ben(tr, oracle, meshes), lambda tr: _scene_posed_quads(oracle, capi, tr, meshes))):
        tr = make_tracer(capi, s, engine)
        ml = setup(tr)
        rc, pts, hits = tr.traceScene(0)
        assert rc == 0 and hits.shape[0] > 0
        assert hits.shape[0] == np.count_nonzero(oracle.trace_frame(s, ml)["gid"] != INV)
        if k == 0:
            assert hits.shape[0] == 1781   # (the reference's count for this frame, BASELINE.json)
        rec = _records(hits)
        n_labels = len(ml)
        want = ref.reduce_records(rec, _xyz(pts), _geoms(ml), n_labels, s.V * s.H)
        assert np.all(want["n_hits"] > 0)
        rc, got = tr.objectLabels(hits, footprint=False)
        assert rc == 0
        _same(got, want)
        assert int(got["n_hits"].sum()) == hits.shape[0]
        _check_ties(got, rec, np.ones(rec.shape[0], bool))
        # with the footprint: the same records, and per geometry the rays the oracle's frame over that geometry alone hits
        rc, full = tr.objectLabels(hits)
        assert rc == 0
        alone = np.array([np.count_nonzero(oracle.trace_frame(s, [m])["gid"] != INV) for m in ml])
        want["n_alone"] = alone
        _same(full, want)
        assert np.all(full["n_hits"] <= full["n_alone"])
        _same(_labels_device(tr, capi, n_labels, rec), want)
        assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
        tr.close()


# ---- 2. the footprint against the brute force ------------------------------------------------------------------------------------

def test_footprint_equals_the_brute_force_per_geometry(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    scene = oracle.assemble_scene(s, ml)
    rays = _random_rays(np.random.default_rng(5), 600, scene.verts.mean(0), 25.0, 1e3)
    rc, hits = tr.traceRays(rays)
    assert rc == 0
    rec = _records(hits)
    alone, M = ref.footprint(oracle, s, ml, rays, 3)
    # the reference's own numbers first: an empty case must not pass silently
    closest = np.bincount(rec[rec[:, 1] != INV, 1], minlength=3)
    assert list(closest) == [323, 11, 3]
    assert list(alone) == [336, 17, 7]
    assert np.count_nonzero(M.sum(axis=1) >= 2) == 20
    want = ref.reduce_records(rec, ref.record_points(rec, rays), _geoms(ml), 3, 600, rays)
    want["n_alone"] = alone
    rc, got = tr.objectLabels(hits, rays)
    assert rc == 0
    _same(got, want)
    assert list(got["n_hits"]) == [323, 11, 3] and np.all(got["n_hits"] < got["n_alone"])
    # equal totals can hide one missed ray plus one false one: one call per ray for the first 64 rays that pierce anything
    some = np.nonzero(M.any(axis=1))[0][:64]
    assert some.shape[0] == 64
    for r in some:
        rc, one = tr.objectLabels(None, rays[r:r + 1])
        assert rc == 0 and np.array_equal(one["n_alone"], M[r].astype(np.uint32)), r
        assert np.all(one["n_hits"] == 0)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 3. a hidden object ----------------------------------------------------------------------------------------------------------

def _box(lo, hi):
    lo, hi = np.float64(lo), np.float64(hi)
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float64)
    f = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]]
    return v, np.array(f, np.uint32)


def test_a_hidden_object_has_a_footprint_and_no_hits(oracle, capi, sensors):
    """a wall, a smaller box entirely behind it and a box beside it, given in the sensor frame and carried into the world through the
    sensor pose; the sensor's own rays (a 16 x 120 raster with the XT-32's pose)"""
    s0 = sensors["0000"]
    s = oracle.Sensor(uid="small", vertical=np.linspace(-15.0, 15.0, 16).astype(np.float32), h_begin=np.float32(0.0), h_end=np.float32(360.0),
                      h_count=120, R=s0.R, Rinv=s0.Rinv, t=s0.t)
    R = np.asarray(s.R, np.float64).reshape(3, 3)
    world = lambda v: (v @ R.T + np.asarray(s.t, np.float64)).astype(np.float32)
    wall = (world(np.float64([[5, -3, -3], [5, 3, -3], [5, 3, 3], [5, -3, 3]])), np.uint32([[0, 1, 2], [0, 2, 3]]))
    hv, hf = _box([7, -1, -1], [8, 1, 1])
    fv, ff = _box([4, 7, -1], [5, 8.5, 1])
    hidden, free = (world(hv), hf), (world(fv), ff)
    tr = make_tracer(capi, s)
    ml = []
    for gid, (name, mesh) in enumerate((("wall", wall), ("hidden", hidden), ("free", free))):
        assert _add(tr, name, *mesh) == gid
        tr.updateGeometry(name, oracle.IDENTITY_AFFINE, *mesh)
        ml.append((gid, *mesh, oracle.IDENTITY_AFFINE))
    assert tr.commitScene() == 0
    rc, pts, hits = tr.traceScene(0)
    assert rc == 0
    rec = _records(hits)
    rays = np.zeros((s.V * s.H, 8), np.float32)
    rays[:, 4:7] = oracle.ray_dirs(s)
    rays[:, 7] = np.inf
    alone, _ = ref.footprint(oracle, s, ml, rays, 3)
    want = ref.reduce_records(rec, _xyz(pts), _geoms(ml), 3, s.V * s.H)
    want["n_alone"] = alone
    assert alone[1] > 4 and want["n_hits"][0] > 20 and want["n_hits"][2] > 4
    rc, got = tr.objectLabels(hits)
    assert rc == 0
    _same(got, want)
    h = got[1]
    assert h["n_hits"] == 0 and h["flags"] == 1 and h["n_alone"] > 0
    assert h["t_min"] == np.inf and h["t_max"] == -np.inf and h["ray_min"] == INV and h["ray_max"] == INV
    assert np.all(h["lo"] == np.inf) and np.all(h["hi"] == -np.inf) and np.all(h["reserved"] == 0)
    assert got["n_hits"][2] == got["n_alone"][2] and got["n_hits"][0] == got["n_alone"][0]
    # an azimuth shard changes nothing: the footprint runs over the full raster, hit.ray is the global index
    tr.setShard(30, 40)
    rc, sharded = tr.objectLabels(hits)
    assert rc == 0
    _same(sharded, want)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 4. more than one launch -----------------------------------------------------------------------------------------------------

def test_twenty_geometries_in_two_launches(oracle, capi, sensors, meshes):
    """the scene of test_many_geometries_with_singular_and_ill_conditioned_poses: one pose scaled to zero, one at a 1:2000 scale ratio,
    one kept in the sensor frame, two that coincide.  With n_labels = 18 the two highest ids are counted nowhere."""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    rng = np.random.default_rng(3)
    ml = [(0, *meshes["ground"], oracle.IDENTITY_AFFINE)]
    _add(tr, "g0", *meshes["ground"])
    tr.updateGeometry("g0", oracle.IDENTITY_AFFINE, *meshes["ground"])
    for k in range(1, 20):
        A = oracle.affine_from_components(np.float32(rng.uniform(-15, 15, 3) * [1, 1, 0]), np.float32(rng.uniform(-1, 1, 3)))
        if k == 4:
            A = np.zeros(12, np.float32)
            A[3], A[7] = 2.0, 2.0
        if k == 9:
            A = np.float32([1.0, 0, 0, -3.0, 0, 1e-3 / 2, 0, 4.0, 0, 0, 0.5, 0.5])
        if k == 15:
            A = np.float32([0.8, 0, 0, 6.0, 0, 0.8e-4, 0, -4.0, 0, 0, 0.4, 0.5])
        if k == 12:
            A = ml[1][3]
        _add(tr, f"g{k}", *meshes["ben"])
        tr.updateGeometry(f"g{k}", A, *meshes["ben"])
        ml.append((k, *meshes["ben"], A))
    assert tr.commitScene() == 0
    scene = oracle.assemble_scene(s, ml)
    rays = _random_rays(rng, 320, scene.verts.mean(0), 20.0, 300.0)
    rc, hits = tr.traceRays(rays)
    assert rc == 0
    rec = _records(hits)
    # the brute force without the geometry scaled to zero: its triangles are points, which the exact test never hits (and which
    # would be candidates of every ray there)
    assert np.all(oracle.assemble_scene(s, [ml[4]]).verts == oracle.assemble_scene(s, [ml[4]]).verts[0])
    live = [m for m in ml if m[0] != 4]
    alone, M = ref.footprint(oracle, s, live, rays, 20)
    assert np.count_nonzero(alone) >= 8 and alone[4] == 0 and alone[1] == alone[12] > 0
    assert np.count_nonzero(alone[16:]) >= 2 and np.count_nonzero(M.sum(axis=1) >= 2) > 5
    want = ref.reduce_records(rec, ref.record_points(rec, rays), _geoms(ml), 20, 320, rays)
    want["n_alone"] = alone
    assert want["n_hits"][12] == 0 < want["n_hits"][1]          # equal t on both: the lower id wins the closest hit
    rc, got = tr.objectLabels(hits, rays)
    assert rc == 0
    _same(got, want)
    _same(_labels_device(tr, capi, 20, rec, rays), want)
    # n_labels = 18: ids 18 and 19 are counted nowhere, and nothing is written past record 18 (the guard of _labels_device)
    want18 = ref.reduce_records(rec, ref.record_points(rec, rays), _geoms(ml), 18, 320, rays)
    want18["n_alone"] = alone[:18]
    _same(want18, want[:18])
    assert want["n_hits"][18] + want["n_hits"][19] + alone[18] + alone[19] > 0
    _same(_labels_device(tr, capi, 18, rec, rays), want18)
    rc, got18 = tr.objectLabels(hits, rays, n_labels=18)
    assert rc == 0
    _same(got18, want18)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 5. ranges and degenerate rays -----------------------------------------------------------------------------------------------

def test_ranges_decide_which_geometries_a_ray_counts_in(oracle, capi, sensors):
    """two parallel planes (test_tmin_tmax_filter's): a ray counts in one, both or neither as [tmin, tmax] says, edges included"""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    plane = (np.float32([[-5, -5, 0], [5, -5, 0], [5, 5, 0], [-5, 5, 0]]), np.uint32([[0, 1, 2], [0, 2, 3]]))
    A1 = oracle.affine_from_components(np.float32([0, 0, 1.0]), np.float32([0, 0, 0]))
    A2 = oracle.affine_from_components(np.float32([0, 0, 2.0]), np.float32([0, 0, 0]))
    _add(tr, "p1", *plane)
    _add(tr, "p2", *plane)
    tr.updateGeometry("p1", A1, *plane)
    tr.updateGeometry("p2", A2, *plane)
    assert tr.commitScene() == 0
    ml = [(0, *plane, A1), (1, *plane, A2)]
    rng = np.random.default_rng(9)
    n = 60
    ow = np.c_[rng.uniform(-3, 3, (n, 2)), np.zeros(n)]
    dw = np.c_[rng.uniform(-0.3, 0.3, (n, 2)), np.ones(n)]
    R = np.asarray(s.Rinv, np.float64).reshape(3, 3)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = (R @ (ow - np.asarray(s.t, np.float64)).T).T, (R @ dw.T).T, np.inf
    t1 = _records(tr.traceRays(rays)[1])[:, 3].view(np.float32).copy()
    past = rays.copy()
    past[:, 3] = np.nextafter(t1, np.float32(np.inf))
    rec2 = _records(tr.traceRays(past)[1])
    assert np.all(rec2[:, 1] == 1)
    t2 = rec2[:, 3].view(np.float32).copy()
    short2 = rays.copy()
    short2[:, 7] = np.nextafter(t2, np.float32(0))
    between = past.copy()
    between[:, 7] = np.nextafter(t2, np.float32(0))
    exact1 = rays.copy()
    exact1[:, 3], exact1[:, 7] = t1, t1
    edges = rays.copy()
    edges[:, 3], edges[:, 7] = t1, t2
    for rr, expect in ((rays, [n, n]), (past, [0, n]), (short2, [n, 0]), (between, [0, 0]), (exact1, [n, 0]), (edges, [n, n])):
        alone, _ = ref.footprint(oracle, s, ml, rr, 2)
        assert list(alone) == expect
        rc, got = tr.objectLabels(None, rr)
        assert rc == 0 and list(got["n_alone"]) == expect and np.all(got["n_hits"] == 0) and np.all(got["flags"] == 1)
    # all six kinds in one call
    mixed = np.concatenate([rays[:10], past[10:20], short2[20:30], between[30:40], exact1[40:50], edges[50:60]])
    alone, _ = ref.footprint(oracle, s, ml, mixed, 2)
    assert list(alone) == [40, 30]
    assert list(tr.objectLabels(None, mixed)[1]["n_alone"]) == [40, 30]
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_degenerate_rays_and_bad_records_count_nowhere(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _ground_ben(tr, oracle, meshes)
    good = np.float32([0, 0, 0, 0, 0.3, 0.2, -1.0, np.inf])
    bad = []
    for k in (0, 1, 2, 4, 5, 6):
        for v in (np.nan, np.inf, -np.inf):
            r = good.copy()
            r[k] = v
            bad.append(r)
    z = good.copy()
    z[4:7] = 0
    bad.append(z)
    r = good.copy()
    r[3], r[7] = 5.0, 4.0
    bad.append(r)
    r = good.copy()
    r[3] = np.nan
    bad.append(r)
    r = good.copy()
    r[7] = np.nan
    bad.append(r)
    rays = np.stack([good] + bad + [good])
    n = rays.shape[0]
    rc, hits = tr.traceRays(rays)
    first = _records(hits)[0]
    assert rc == 0 and first[1] == 0
    f = lambda x: np.float32(x).view(np.uint32)
    # a record per ray, all naming the good ray's triangle at its t: only the two good rays' records count
    rec = np.tile(first, (n, 1))
    rec[:, 0] = np.arange(n)
    n_ground, n_ben = (int(m[2].shape[0]) for m in ml)
    extra = np.array([[n, 0, 0, f(1.0)], [INV, 0, 0, f(1.0)],            # ray >= n_rays
                      [0, 0, n_ground, f(1.0)], [0, 1, n_ben, f(1.0)], [0, 1, INV, f(1.0)],   # prim >= its element count
                      [0, 2, 0, f(1.0)], [0, 7, 0, f(1.0)], [0, INV, INV, f(-1.0)],            # an unknown geom, a miss record
                      [0, 0, 0, f(np.nan)], [0, 0, 0, f(-np.nan)], [0, 0, 0, f(-1.0)], [0, 0, 0, f(-1e-30)],
                      [0, 0, 0, f(np.inf)], [0, 0, 0, f(-np.inf)]], np.uint32)
    both = np.concatenate([rec, extra, rec[::-1]])
    ok = ref.counted(both, _geoms(ml), 4, n, rays)
    assert np.count_nonzero(ok) == 4 and not np.any(ok[n:n + extra.shape[0]])
    want = ref.reduce_records(both, ref.record_points(both, rays), _geoms(ml), 4, n, rays)
    alone, _ = ref.footprint(oracle, s, ml, rays, 4)
    want["n_alone"] = alone
    assert list(want["n_hits"]) == [4, 0, 0, 0] and list(alone) == [2, 0, 0, 0] and list(want["flags"]) == [1, 1, 0, 0]
    rc, got = tr.objectLabels(both, rays, n_labels=4)
    assert rc == 0
    _same(got, want)
    assert got["ray_min"][0] == 0 and got["ray_max"][0] == 0
    _same(_labels_device(tr, capi, 4, both, rays), want)
    # the same records against the sensor's own rays: the bound is V * H, so the record of ray n -- beyond the caller's rays -- counts
    rc, own = tr.objectLabels(extra, n_labels=4, footprint=False)
    assert rc == 0 and n < s.V * s.H and list(own["n_hits"]) == [1, 0, 0, 0] and own["ray_min"][0] == n
    _same(own, ref.reduce_records(extra, _xyz_of_sensor_rays(oracle, s, extra), _geoms(ml), 4, s.V * s.H))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 6. plumbing -----------------------------------------------------------------------------------------------------------------

def test_entry_points(oracle, capi, sensors, meshes):
    """a device count below n; n = 0 (the footprint alone); no flag: n_alone = 0 and LS_INFO_RAY_QUERY_BUILT untouched; a caller
    stream; device == host; two calls and shuffled records: the same bytes; refused arguments in their order; a removed geometry;
    no commit: -1 and nothing written.  (LS_ERR_NOT_COMMITTED -- a layout entry whose geometry is gone or changed -- is not
    reachable through the public entry points, for this call as for the other queries: ls_remove_geometry commits the remaining
    scene itself, and the call follows it.)"""
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    scene = oracle.assemble_scene(s, ml)
    rays = _random_rays(np.random.default_rng(41), 3000, scene.verts.mean(0), 25.0, 500.0)
    # without the flag nothing is built and the word is left as it is
    rec0 = np.array([[0, 0, 0, np.float32(1.0).view(np.uint32)]], np.uint32)
    built = tr.info(capi.LS_INFO_RAY_QUERY_BUILT)
    rc, plain = tr.objectLabels(rec0, rays, footprint=False)
    assert rc == 0 and list(plain["n_hits"]) == [1, 0, 0] and np.all(plain["n_alone"] == 0)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == built
    rc, hits = tr.traceRays(rays)
    assert rc == 0 and tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 3
    rec = _records(hits)
    rc, plain = tr.objectLabels(hits, rays, footprint=False)
    assert rc == 0 and np.all(plain["n_alone"] == 0) and tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 3
    want_plain = ref.reduce_records(rec, ref.record_points(rec, rays), _geoms(ml), 3, 3000, rays)
    _same(plain, want_plain)
    # with it: the shared hierarchies are there already
    rc, host = tr.objectLabels(hits, rays)
    assert rc == 0 and tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 0
    assert np.all(host["n_hits"] > 0) and np.all(host["n_hits"] <= host["n_alone"])
    want = want_plain.copy()
    want["n_alone"] = host["n_alone"]
    _same(host, want)
    # device == host, twice, on a caller stream, for shuffled records
    _same(_labels_device(tr, capi, 3, rec, rays), host)
    _same(_labels_device(tr, capi, 3, rec, rays), host)
    st = torch.cuda.Stream()
    _same(_labels_device(tr, capi, 3, rec, rays, stream=st.cuda_stream), host)
    perm = np.random.default_rng(7).permutation(rec.shape[0])
    _same(_labels_device(tr, capi, 3, rec[perm], rays), host)
    _same(tr.objectLabels(hits[perm], rays)[1], host)
    # a device count below n: the records beyond it are not read
    part = ref.reduce_records(rec[:1234], ref.record_points(rec[:1234], rays), _geoms(ml), 3, 3000, rays)
    part["n_alone"] = host["n_alone"]
    _same(_labels_device(tr, capi, 3, rec, rays, count=1234), part)
    _same(_labels_device(tr, capi, 3, rec, rays, count=5000), host)
    # n = 0: the footprint alone; n_labels = 0: nothing to write
    only = ref.empty_labels(3)
    only["flags"] = 1
    only["n_alone"] = host["n_alone"]
    _same(_labels_device(tr, capi, 3, None, rays), only)
    _same(tr.objectLabels(None, rays)[1], only)
    assert tr.objectLabelsDevice(0, 0) == 0 and tr.objectLabels(hits, rays, n_labels=0)[1].shape == (0,)
    # refusals, nothing written
    d_rays, d_hits = _to_device(rays), _to_device(rec)
    out = torch.full((3 * 64 + 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L, h = tr.L, tr.h
    args = lambda **kw: [kw.get(k, v) for k, v in (("flags", 1), ("rays", d_rays.data_ptr()), ("n_rays", 3000), ("hits", d_hits.data_ptr()),
                                                    ("count", None), ("n", 3000), ("labels", out.data_ptr()), ("n_labels", 3))]
    assert L.ls_object_labels(h, None, *args(labels=None)) == INVALID_ARGUMENT
    assert L.ls_object_labels(h, None, *args(hits=None)) == INVALID_ARGUMENT
    assert L.ls_object_labels(h, None, *args(flags=2)) == INVALID_ARGUMENT
    assert L.ls_object_labels(h, None, *args(flags=0x80000001)) == INVALID_ARGUMENT
    assert L.ls_object_labels(h, None, *args(rays=d_rays.data_ptr() + 8)) == INVALID_ARGUMENT
    assert L.ls_object_labels(h, None, *args(hits=d_hits.data_ptr() + 4)) == INVALID_ARGUMENT
    assert L.ls_object_labels(h, None, *args(labels=out.data_ptr() + 8)) == INVALID_ARGUMENT
    assert L.ls_object_labels(h, None, *args(count=out.data_ptr() + 2)) == INVALID_ARGUMENT
    assert L.ls_object_labels(h, None, *args(n=0xFFF00001)) == OUT_OF_RANGE
    assert L.ls_object_labels(h, None, *args(n_rays=0xFFF00001)) == OUT_OF_RANGE
    assert L.ls_object_labels(h, None, *args(n_labels=65537)) == OUT_OF_RANGE
    assert L.ls_object_labels(h, None, *args(flags=2, n_labels=65537)) == INVALID_ARGUMENT       # the earlier refusal answers
    hostbuf = np.full(3 * 64, 0xAB, np.uint8)
    assert L.ls_object_labels_host(h, 2, rays.ctypes.data, 3000, rec.ctypes.data, 3000, hostbuf.ctypes.data, 3) == INVALID_ARGUMENT
    assert L.ls_object_labels_host(h, 1, rays.ctypes.data, 3000, None, 3000, hostbuf.ctypes.data, 3) == INVALID_ARGUMENT
    assert L.ls_object_labels_host(h, 1, rays.ctypes.data, 3000, rec.ctypes.data, 3000, hostbuf.ctypes.data, 65537) == OUT_OF_RANGE
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB) and np.all(hostbuf == 0xAB)
    # 65536 labels are allowed: the records past the highest id are empty
    rc, many = tr.objectLabels(hits, rays, footprint=False, n_labels=65536)
    assert rc == 0
    _same(many[:3], want_plain)
    assert many[3:].tobytes() == ref.empty_labels(65533).tobytes()
    # a removal commits the remaining scene: the call follows it, the removed geometry's records count nowhere
    assert tr.removeGeometry("face") >= 0
    rc, after = tr.objectLabels(hits, rays, n_labels=3)
    assert rc == 0
    left = {g: ne for g, ne in _geoms(ml).items() if g != 1}
    want_after = ref.reduce_records(rec, ref.record_points(rec, rays), left, 3, 3000, rays)
    want_after["n_alone"] = host["n_alone"]
    want_after["n_alone"][1] = 0
    _same(after, want_after)
    assert after["flags"][1] == 0 and after["n_hits"][1] == 0
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
    # no commit: -1, nothing written
    t2 = make_tracer(capi, s)
    assert t2.objectLabelsDevice(out.data_ptr(), 3, d_hits.data_ptr(), 3000, d_rays.data_ptr(), 3000) == -1
    assert t2.L.ls_object_labels_host(t2.h, 1, rays.ctypes.data, 3000, rec.ctypes.data, 3000, hostbuf.ctypes.data, 3) == -1
    rc, none = t2.objectLabels(hits, rays, n_labels=3)
    assert rc == -1 and none.tobytes() == ref.empty_labels(3).tobytes()
    t2.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB) and np.all(hostbuf == 0xAB)
    t2.close()


def test_open_frame_graph_is_refused(oracle, capi, sensors, meshes):
    import torch
    s = sensors["0001"]
    tr = make_tracer(capi, s, "projection")
    tr.setOption(capi.LS_OPT_PIPELINE, 2)
    tr.setOption(capi.LS_OPT_FRAME_GRAPH, 1)
    _ground_ben(tr, oracle, meshes)
    cap = s.V * s.H
    p, h, c = (torch.zeros(32 * cap, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * cap, dtype=torch.uint8, device="cuda:0"),
               torch.zeros(4, dtype=torch.int32, device="cuda:0"))
    tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), cap)
    out = torch.full((2 * 64,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L = tr.L
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != FRAME_EAGER   # the frame is being captured: the graph is open
    assert L.ls_object_labels(tr.h, None, 1, None, 0, h.data_ptr(), c.data_ptr(), cap, out.data_ptr(), 2) == INVALID_ARGUMENT
    assert L.ls_object_labels_host(tr.h, 0, None, 0, None, 0, None, 0) == INVALID_ARGUMENT
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB)
    # the frame went out, and the handle labels its records where they lie: d_hits, the device count, n = the capacity
    k = int(c[0].item())
    assert k > 0
    assert tr.objectLabelsDevice(out.data_ptr(), 2, h.data_ptr(), cap, d_count=c.data_ptr()) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    lab = out.cpu().numpy().view(capi.OBJECT_LABEL_DTYPE)
    rec = h.cpu().numpy()[:16 * k].view(np.uint32).reshape(k, 4)
    want = ref.reduce_records(rec, _xyz(p.cpu().numpy()[:32 * k]), {0: meshes["ground"][1].shape[0], 1: meshes["ben"][1].shape[0]}, 2, cap)
    assert int(lab["n_hits"].sum()) == k and np.all(lab["n_hits"] <= lab["n_alone"])
    want["n_alone"] = lab["n_alone"]
    _same(lab, want)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 7. a removed and re-added geometry ------------------------------------------------------------------------------------------

def test_a_free_id_below_the_highest_gets_the_empty_record(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    assert tr.removeGeometry("face") >= 0
    A = oracle.affine_from_components(np.float32([-2.0, 2.0, 0.2]), np.float32([0.0, 0.0, 0.5]))
    new_id = _add(tr, "face", *meshes["ben"])
    tr.updateGeometry("face", A, *meshes["ben"])
    assert tr.commitScene() == 0
    ids = {name: tr.getGeometryId(name) for name in ("ground", "face", "plate")}
    assert ids["ground"] == 0 and ids["plate"] == 2 and ids["face"] == new_id
    now = [ml[0], (new_id, *meshes["ben"], A), ml[2]]
    n_labels = max(ids.values()) + 1
    free = sorted(set(range(n_labels)) - set(ids.values()))
    if new_id == 1:   # the id was handed out again: free one below the highest by removing the ground's neighbour instead
        assert tr.removeGeometry("face") >= 0
        now = [ml[0], ml[2]]
        free = [1]
    assert free and free[0] < n_labels - 1
    rc, pts, hits = tr.traceScene(0)
    assert rc == 0 and hits.shape[0] > 0
    rec = _records(hits)
    want = ref.reduce_records(rec, _xyz(pts), _geoms(now), n_labels, s.V * s.H)
    want["n_alone"] = [0 if g in free else np.count_nonzero(oracle.trace_frame(s, [m for m in now if m[0] == g])["gid"] != INV)
                       for g in range(n_labels)]
    rc, got = tr.objectLabels(hits)
    assert rc == 0 and got.shape[0] == n_labels
    _same(got, want)
    for g in free:
        assert got[g].tobytes() == ref.empty_labels(1)[0].tobytes()
    # a stale record that names the free id counts nowhere
    stale = rec.copy()
    stale[::3, 1] = free[0]
    rc, got = tr.objectLabels(stale, footprint=False)
    assert rc == 0 and got["n_hits"][free[0]] == 0 and got["flags"][free[0]] == 0
    assert int(got["n_hits"].sum()) == rec.shape[0] - stale[::3].shape[0]
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
