"""ls_trace_rays / ls_trace_rays_host on the MI355X: closest hits of caller rays, against the frame's own hits (the sensor's
rays, another sensor's rays) and against a brute force over the oracle's scene with lso_tri_intersect (arbitrary origins,
ranges, degenerate rays, pose and vertex changes, more than one launch's worth of geometries)."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from conftest import make_tracer

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF


def _add(tr, name, verts, elems, gtype=0):
    gid = tr.addGeometry(name, verts.shape[0], elems.shape[0], gtype)
    assert gid >= 0
    return gid


def _ground_ben(tr, oracle, meshes, A_ben=None):
    A_ben = oracle.IDENTITY_AFFINE if A_ben is None else A_ben
    _add(tr, "ground", *meshes["ground"])
    _add(tr, "face", *meshes["ben"])
    tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *meshes["ground"])
    tr.updateGeometry("face", A_ben, *meshes["ben"])
    assert tr.commitScene() == 0
    return [(0, *meshes["ground"], oracle.IDENTITY_AFFINE), (1, *meshes["ben"], A_ben)]


def _records(hits):
    return np.stack([hits["ray"], hits["geom"], hits["prim"], hits["t"].view(np.uint32)], axis=1)


def _from_gid(scene, t, gid):
    """dense (t, global triangle id) -> ls_hit records (ray, geom, prim, t bits)"""
    n = gid.shape[0]
    out = np.zeros((n, 4), np.uint32)
    out[:, 0] = np.arange(n)
    hit = gid != INV
    slot = np.searchsorted(scene.geom_first.astype(np.int64), gid[hit].astype(np.int64), side="right") - 1
    local = gid[hit].astype(np.int64) - scene.geom_first[slot]
    quad = scene.geom_quad[slot] if scene.geom_quad is not None else np.zeros_like(slot, bool)
    out[hit, 1] = scene.geom_ids[slot]
    out[hit, 2] = np.where(quad, local >> 1, local)
    out[hit, 3] = t[hit].view(np.uint32)
    out[~hit, 1] = INV
    out[~hit, 2] = INV
    out[~hit, 3] = np.float32(-1.0).view(np.uint32)
    return out


def _sensor_rays(tr, capi):
    import torch
    n = tr.getTotalRays()
    d = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    tr.generateRaysAos(d.data_ptr(), None)
    tr.synchronize()
    return d, n


def _trace_device(tr, d_rays, n, stream=None):
    import torch
    out = torch.full((n * 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    assert tr.traceRaysDevice(d_rays.data_ptr(), n, out.data_ptr(), stream) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(n, 4)


def _brute(oracle, scene, rays):
    """closest_brute over the oracle's scene with lso_tri_intersect, from each ray's origin: ascending global id, a hit kept
    when tmin <= t <= tmax and t < the running best (+inf at first).  Candidates prefiltered in float64."""
    L = oracle.lib()
    f32p = ctypes.POINTER(ctypes.c_float)
    V = scene.verts.astype(np.float64)
    T = scene.tris.astype(np.int64)
    a, b, c = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    e1, e2 = b - a, c - a
    out = np.zeros((rays.shape[0], 4), np.uint32)
    tt = np.zeros(1, np.float32)
    for r in range(rays.shape[0]):
        o = rays[r, 0:3].astype(np.float32)
        d = rays[r, 4:7].astype(np.float32)
        tmin, tmax = rays[r, 3], rays[r, 7]
        out[r] = (r, INV, INV, np.float32(-1.0).view(np.uint32))
        if not (np.all(np.isfinite(o)) and np.all(np.isfinite(d)) and np.any(d != 0) and tmin <= tmax):
            continue
        od, dd = o.astype(np.float64), d.astype(np.float64)
        p = np.cross(dd, e2)
        det = np.einsum("ij,ij->i", e1, p)
        scale = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) * np.linalg.norm(dd) + 1e-300
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            s = od - a
            u = np.einsum("ij,ij->i", s, p) * inv
            qv = np.cross(s, e1)
            v = (qv @ dd) * inv
            t = np.einsum("ij,ij->i", e2, qv) * inv
        tol = 1e-3
        cand = np.nonzero((np.abs(det) < 1e-7 * scale) | ((u >= -tol) & (v >= -tol) & (u + v <= 1 + tol) & (t >= -1e-3 * (1 + np.abs(t)))))[0]
        best, bid = np.float32(np.inf), INV
        for k in cand:   # ascending global id
            v0, v1, v2 = (np.ascontiguousarray(scene.verts[scene.tris[k, j]], np.float32) for j in range(3))
            if L.lso_tri_intersect(o.ctypes.data_as(f32p), d.ctypes.data_as(f32p), v0.ctypes.data_as(f32p), v1.ctypes.data_as(f32p),
                                   v2.ctypes.data_as(f32p), tt.ctypes.data_as(f32p)):
                if tmin <= tt[0] <= tmax and tt[0] < best:
                    best, bid = np.float32(tt[0]), int(k)
        if bid != INV:
            out[r] = _from_gid(scene, np.array([best], np.float32), np.array([bid], np.uint32))[0]
            out[r, 0] = r
    return out


def _random_rays(rng, n, center, spread, far):
    """origins inside and outside the scene box (some up to `far` away), random directions, tmin 0, tmax +inf"""
    r = np.zeros((n, 8), np.float32)
    near = rng.uniform(-spread, spread, (n, 3))
    away = rng.normal(size=(n, 3))
    away *= (rng.uniform(0, far, n) / np.linalg.norm(away, axis=1))[:, None]
    pick = rng.uniform(size=n) < 0.5
    r[:, 0:3] = center + np.where(pick[:, None], near, away)
    # half the rays aim at a point of the scene, half go anywhere
    target = center + rng.uniform(-spread, spread, (n, 3))
    aim = rng.uniform(size=n) < 0.7
    d = np.where(aim[:, None], target - r[:, 0:3], rng.normal(size=(n, 3)))
    d *= rng.uniform(0.3, 3.0, n)[:, None] / np.linalg.norm(d, axis=1)[:, None]   # not normalised: t is along d as given
    r[:, 4:7] = d
    r[:, 3] = 0.0
    r[:, 7] = np.inf
    return r


@pytest.mark.parametrize("engine", ["projection", "bvh"])
def test_sensor_rays_equal_the_frame(oracle, capi, sensors, meshes, engine):
    """the sensor's own rays (ls_generate_rays_aos) give the frame's dense hits, bit for bit, on both engines"""
    A = oracle.affine_from_components(np.float32([0.4, -0.3, 0.1]), np.float32([0.0, 0.0, 0.6]))
    for uid in ("0000", "0001"):
        s = sensors[uid]
        for A_ben in (oracle.IDENTITY_AFFINE, A):
            tr = make_tracer(capi, s, engine)
            ml = _ground_ben(tr, oracle, meshes, A_ben)
            rc, _, _ = tr.traceScene(0)
            assert rc == 0
            t, gid = tr.denseHits()
            scene = oracle.assemble_scene(s, ml)
            d_rays, n = _sensor_rays(tr, capi)
            got = _trace_device(tr, d_rays, n)
            assert np.array_equal(got, _from_gid(scene, t, gid))
            assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 2
            tr.close()


@pytest.mark.parametrize("engine", ["projection", "bvh"])
def test_syn128_raster_over_a_grid_equals_the_frame(oracle, capi, sensors, engine):
    from lidarshooter_amd import synth
    s0 = sensors["0000"]
    s = oracle.Sensor(uid="syn", vertical=synth.syn_vertical(128), h_begin=np.float32(0.0), h_end=np.float32(360.0), h_count=4096,
                      R=s0.R, Rinv=s0.Rinv, t=s0.t)
    grid = synth.grid_mesh(250, 200)   # 100 000 triangles
    tr = make_tracer(capi, s, engine)
    _add(tr, "grid", *grid)
    tr.updateGeometry("grid", oracle.IDENTITY_AFFINE, *grid)
    assert tr.commitScene() == 0
    assert tr.traceScene(0)[0] == 0
    t, gid = tr.denseHits()
    scene = oracle.assemble_scene(s, [(0, *grid, oracle.IDENTITY_AFFINE)])
    d_rays, n = _sensor_rays(tr, capi)
    got = _trace_device(tr, d_rays, n)
    assert np.count_nonzero(got[:, 1] != INV) > n // 4
    assert np.array_equal(got, _from_gid(scene, t, gid))
    tr.close()


def test_one_scene_several_sensors(oracle, capi, sensors, meshes):
    """handle A traces sensor B's rays (same pose, another raster / the other unit's channels): B's own frame, bit for bit;
    both sensors' rays in one call too"""
    import torch
    sa = sensors["0000"]
    others = [oracle.Sensor(uid="b1", vertical=sa.vertical, h_begin=np.float32(7.5), h_end=np.float32(300.0), h_count=233, R=sa.R, Rinv=sa.Rinv, t=sa.t),
              oracle.Sensor(uid="b2", vertical=sensors["0001"].vertical, h_begin=sensors["0001"].h_begin, h_end=sensors["0001"].h_end,
                            h_count=sensors["0001"].h_count, R=sa.R, Rinv=sa.Rinv, t=sa.t)]
    ta = make_tracer(capi, sa)
    ml = _ground_ben(ta, oracle, meshes)
    assert ta.traceScene(0)[0] == 0
    ra, na = _sensor_rays(ta, capi)
    ta_t, ta_gid = ta.denseHits()
    scene = oracle.assemble_scene(sa, ml)
    for sb in others:
        tb = make_tracer(capi, sb)
        _ground_ben(tb, oracle, meshes)
        assert tb.traceScene(0)[0] == 0
        t, gid = tb.denseHits()
        rb, nb = _sensor_rays(tb, capi)
        want_b = _from_gid(scene, t, gid)
        assert np.array_equal(_trace_device(ta, rb, nb), want_b)
        both = torch.cat([ra, rb])
        got = _trace_device(ta, both, na + nb)
        want = np.concatenate([_from_gid(scene, ta_t, ta_gid), want_b])
        want[:, 0] = np.arange(na + nb)
        assert np.array_equal(got, want)
        tb.close()
    ta.close()


def _scene_posed_quads(oracle, capi, tr, meshes):
    """ground + ben posed + a quad mesh (a 6 x 4 plate of quads, tilted, posed)"""
    A_ben = oracle.affine_from_components(np.float32([1.5, -2.0, 0.3]), np.float32([0.2, -0.1, 1.1]))
    ml = [(0, *meshes["ground"], oracle.IDENTITY_AFFINE), (1, *meshes["ben"], A_ben)]
    xs, ys = np.meshgrid(np.linspace(-3, 3, 7), np.linspace(-2, 2, 5), indexing="xy")
    pv = np.stack([xs, ys, 0.3 * xs], -1).reshape(-1, 3).astype(np.float32)
    q = []
    for j in range(4):
        for i in range(6):
            v00 = j * 7 + i
            q.append([v00, v00 + 1, v00 + 8, v00 + 7])
    pq = np.array(q, np.uint32)
    A_plate = oracle.affine_from_components(np.float32([4.0, 3.0, 1.5]), np.float32([0.3, 0.0, -0.4]))
    ml.append((2, pv, pq, A_plate))
    _add(tr, "ground", *meshes["ground"])
    _add(tr, "face", *meshes["ben"])
    _add(tr, "plate", pv, pq, capi.LS_GEOMETRY_TYPE_QUAD)
    tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *meshes["ground"])
    tr.updateGeometry("face", A_ben, *meshes["ben"])
    tr.updateGeometry("plate", A_plate, pv, pq)
    assert tr.commitScene() == 0
    return ml


def test_arbitrary_origins_equal_the_brute_force(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    scene = oracle.assemble_scene(s, ml)
    center = scene.verts.mean(0)
    rng = np.random.default_rng(5)
    rays = _random_rays(rng, 600, center, 25.0, 1e3)
    rc, hits = tr.traceRays(rays)
    assert rc == 0
    got = _records(hits)
    want = _brute(oracle, scene, rays)
    assert np.count_nonzero(want[:, 1] != INV) > 150 and len(set(want[:, 1]) - {INV}) == 3
    assert np.array_equal(got, want)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_tmin_tmax_filter(oracle, capi, sensors):
    """two parallel planes: tmin just past the first hit gives the second, tmax just short of the first gives a miss"""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    plane = (np.float32([[-5, -5, 0], [5, -5, 0], [5, 5, 0], [-5, 5, 0]]), np.uint32([[0, 1, 2], [0, 2, 3]]))
    A1 = oracle.affine_from_components(np.float32([0, 0, 1.0]), np.float32([0, 0, 0]))
    A2 = oracle.affine_from_components(np.float32([0, 0, 2.0]), np.float32([0, 0, 0]))
    # world planes; rays in the sensor frame: build them from world points through the sensor pose
    _add(tr, "p1", *plane)
    _add(tr, "p2", *plane)
    tr.updateGeometry("p1", A1, *plane)
    tr.updateGeometry("p2", A2, *plane)
    assert tr.commitScene() == 0
    ml = [(0, *plane, A1), (1, *plane, A2)]
    scene = oracle.assemble_scene(s, ml)
    rng = np.random.default_rng(9)
    n = 200
    ow = np.c_[rng.uniform(-3, 3, (n, 2)), np.zeros(n)]          # world origins below both planes
    dw = np.c_[rng.uniform(-0.3, 0.3, (n, 2)), np.ones(n)]
    R = np.asarray(s.Rinv, np.float64).reshape(3, 3)
    o = (R @ (ow - np.asarray(s.t, np.float64)).T).T
    d = (R @ dw.T).T
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = o, d, np.inf
    rc, h = tr.traceRays(rays)
    first = _records(h)
    assert rc == 0 and np.all(first[:, 1] == 0)
    assert np.array_equal(first, _brute(oracle, scene, rays))
    t1 = first[:, 3].view(np.float32)
    past = rays.copy()
    past[:, 3] = np.nextafter(t1, np.float32(np.inf))
    short = rays.copy()
    short[:, 7] = np.nextafter(t1, np.float32(0))
    exact = rays.copy()
    exact[:, 3] = t1
    exact[:, 7] = t1
    for rr in (past, short, exact):
        rc, h = tr.traceRays(rr)
        assert np.array_equal(_records(h), _brute(oracle, scene, rr))
    assert np.all(_records(tr.traceRays(past)[1])[:, 1] == 1)
    assert np.all(_records(tr.traceRays(short)[1])[:, 1] == INV)
    assert np.array_equal(_records(tr.traceRays(exact)[1]), first)
    tr.close()


def test_degenerate_rays_are_misses(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
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
    rc, h = tr.traceRays(rays)
    got = _records(h)
    assert rc == 0
    assert got[0, 1] != INV and np.array_equal(got[0, 1:], got[-1, 1:])
    assert np.all(got[1:-1, 1] == INV) and np.all(got[1:-1, 2] == INV) and np.all(got[1:-1, 3].view(np.float32) == -1.0)
    assert np.array_equal(got[:, 0], np.arange(len(rays)))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_pose_only_change_builds_nothing_and_new_vertices_rebuild_one(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    rng = np.random.default_rng(11)
    scene = oracle.assemble_scene(s, ml)
    rays = _random_rays(rng, 300, scene.verts.mean(0), 20.0, 100.0)
    tr.traceRays(rays)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 3
    tr.traceRays(rays)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 0
    # a pose change and a commit: nothing built, the answers follow the new pose
    A_new = oracle.affine_from_components(np.float32([-1.0, 2.5, 0.2]), np.float32([0.0, 0.3, -0.7]))
    tr.updateGeometryTransform("face", A_new)
    assert tr.commitScene() == 0
    rc, h = tr.traceRays(rays)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 0
    ml[1] = (1, *meshes["ben"], A_new)
    assert np.array_equal(_records(h), _brute(oracle, oracle.assemble_scene(s, ml), rays))
    # new vertices for one geometry: only that one is built (refitted)
    v2 = meshes["ben"][0] * np.float32(1.3)
    tr.updateGeometry("face", A_new, v2, None)
    assert tr.commitScene() == 0
    rc, h = tr.traceRays(rays)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 1
    ml[1] = (1, v2, meshes["ben"][1], A_new)
    assert np.array_equal(_records(h), _brute(oracle, oracle.assemble_scene(s, ml), rays))
    # new indices: that one again
    tris = meshes["ben"][1][::-1].copy()
    tr.updateGeometry("face", A_new, v2, tris)
    assert tr.commitScene() == 0
    rc, h = tr.traceRays(rays)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 1
    ml[1] = (1, v2, tris, A_new)
    assert np.array_equal(_records(h), _brute(oracle, oracle.assemble_scene(s, ml), rays))
    tr.close()


def test_many_geometries_with_singular_and_ill_conditioned_poses(oracle, capi, sensors, meshes):
    """20 geometries (two launches): one scaled to zero (no inverse), one at a 1:2000 scale ratio (kept in the sensor
    frame), the rest posed copies of ben; equal to the brute force, ties to the lowest global id"""
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
            A = np.float32([1.0, 0, 0, -3.0, 0, 1e-3 / 2, 0, 4.0, 0, 0, 0.5, 0.5])   # x : y = 2000 : 1 (mesh space, wide boxes)
        if k == 15:
            A = np.float32([0.8, 0, 0, 6.0, 0, 0.8e-4, 0, -4.0, 0, 0, 0.4, 0.5])   # 10 000 : 1: kept in the sensor frame
        if k == 12:
            A = ml[1][3]   # the same pose as geometry 1: equal t on both, the lower id wins
        _add(tr, f"g{k}", *meshes["ben"])
        tr.updateGeometry(f"g{k}", A, *meshes["ben"])
        ml.append((k, *meshes["ben"], A))
    assert tr.commitScene() == 0
    scene = oracle.assemble_scene(s, ml)
    rays = _random_rays(rng, 320, scene.verts.mean(0), 20.0, 300.0)
    rc, h = tr.traceRays(rays)
    assert rc == 0 and tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 20
    got = _records(h)
    want = _brute(oracle, scene, rays)
    assert len(set(want[:, 1]) - {INV}) >= 8
    assert np.array_equal(got, want)
    # new poses: the 1:10 000 geometry is rebuilt (it is kept in the sensor frame), the 1:2000 one and the rest are not
    A9 = np.float32([1.0, 0, 0, -2.0, 0, 1e-3 / 2, 0, 5.0, 0, 0, 0.5, 0.5])
    A15 = np.float32([0.8, 0, 0, 7.0, 0, 0.8e-4, 0, -3.0, 0, 0, 0.4, 0.2])
    tr.updateGeometryTransform("g9", A9)
    tr.updateGeometryTransform("g15", A15)
    assert tr.commitScene() == 0
    rc, h = tr.traceRays(rays)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 1
    ml[9] = (9, *meshes["ben"], A9)
    ml[15] = (15, *meshes["ben"], A15)
    assert np.array_equal(_records(h), _brute(oracle, oracle.assemble_scene(s, ml), rays))
    tr.close()


def test_frames_are_unaffected_by_queries(oracle, capi, sensors, meshes):
    """three-stream frames with frame graphs, issued before, between and after queries on another stream: the same clouds as
    without queries, and the oracle's"""
    import torch
    s = sensors["0001"]
    A = oracle.affine_from_components(np.float32([0.3, 0.2, 0.0]), np.float32([0.0, 0.0, 0.4]))
    ref = oracle.trace_frame(s, [(0, *meshes["ground"], oracle.IDENTITY_AFFINE), (1, *meshes["ben"], A)])
    cap = s.V * s.H

    def run(with_queries):
        tr = make_tracer(capi, s, "projection")
        tr.setOption(capi.LS_OPT_PIPELINE, 2)
        tr.setOption(capi.LS_OPT_FRAME_GRAPH, 1)
        _ground_ben(tr, oracle, meshes, A)
        rays, n = _sensor_rays(tr, capi)
        qs = torch.cuda.Stream()
        outs = [torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0") for _ in range(5)]
        bufs = [(torch.zeros(32 * cap, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * cap, dtype=torch.uint8, device="cuda:0"),
                 torch.zeros(4, dtype=torch.int32, device="cuda:0")) for _ in range(9)]
        for i in range(9):
            p, h, c = bufs[i]
            tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), cap)
            tr.traceSceneAsync(i)
            if with_queries and i % 2 == 0:
                assert tr.traceRaysDevice(rays.data_ptr(), n, outs[i // 2].data_ptr(), qs.cuda_stream) == 0
        tr.flush()
        tr.synchronize()
        torch.cuda.synchronize()
        digests = []
        for p, h, c in bufs:
            k = int(c[0].item())
            pts = p.cpu().numpy()[:32 * k]
            assert np.array_equal(pts.reshape(k, 32), ref["points"])
            digests.append(hashlib.sha256(pts.tobytes()).hexdigest())
        if with_queries:
            t, gid = ref["t"], ref["gid"]
            want = _from_gid(oracle.assemble_scene(s, [(0, *meshes["ground"], oracle.IDENTITY_AFFINE), (1, *meshes["ben"], A)]), t, gid)
            for o in outs:
                assert np.array_equal(o.cpu().numpy().view(np.uint32).reshape(n, 4), want)
        assert tr.info(capi.LS_INFO_FRAME_GRAPH_STATE) == 1
        tr.close()
        return digests

    assert run(True) == run(False)


def test_host_entry_point_equals_device_entry_point(oracle, capi, sensors, meshes):
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    scene = oracle.assemble_scene(s, ml)
    rays = _random_rays(np.random.default_rng(17), 4000, scene.verts.mean(0), 25.0, 500.0)
    rc, h = tr.traceRays(rays)
    d = torch.from_numpy(rays.view(np.uint8).reshape(-1)).to("cuda:0")
    assert np.array_equal(_records(h), _trace_device(tr, d, rays.shape[0]))
    # n = 0 launches nothing; NULL pointers with n > 0 are refused; no commit: -1
    assert tr.traceRaysDevice(0, 0, 0) == 0
    with pytest.raises(capi.LidarShooterHipError):
        tr.traceRaysDevice(0, 4, 0)
    tr.close()
    t2 = make_tracer(capi, s)
    rc, h = t2.traceRays(rays[:5])
    assert rc == -1 and np.all(h["geom"] == INV)
    t2.close()
