"""ls_occluded_rays / ls_occluded_rays_host on the MI355X: any-hit tests of caller rays, against ls_trace_rays on the same rays
and state (occluded exactly where it reports a hit), the frame's own hits, and the brute force over the oracle's scene
(arbitrary origins and ranges, range edges, degenerate rays, segments, more than one launch's worth of geometries)."""
import ctypes

import numpy as np
import pytest

from conftest import make_tracer
from test_gpu_rays import INV, _add, _brute, _ground_ben, _random_rays, _records, _scene_posed_quads

pytestmark = pytest.mark.gpu

GUARD = 16
INVALID_ARGUMENT = -2                      # LS_ERR_INVALID_ARGUMENT
FRAME_EAGER = 0                            # LS_FRAME_EAGER

# torch fills a new tensor on its own stream, the library works on the handle's: every buffer is filled (a device-wide
# synchronize) before the library gets it


def _sensor_rays(tr):
    """the sensor's own rays (ls_generate_rays_aos) in device memory"""
    import torch
    n = tr.getTotalRays()
    d = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    tr.generateRaysAos(d.data_ptr(), None)
    tr.synchronize()
    return d, n


def _occluded_device(tr, d_rays, n, stream=None, offset=0):
    """ls_occluded_rays into a 0xAB-filled buffer at byte `offset` (any alignment); the bytes around the n results untouched"""
    import torch
    buf = torch.full((offset + n + GUARD,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert tr.occludedRaysDevice(d_rays.data_ptr(), n, buf.data_ptr() + offset, stream) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert np.all(b[:offset] == 0xAB) and np.all(b[offset + n:] == 0xAB)
    out = b[offset:offset + n]
    assert np.all((out == 0) | (out == 1))
    return out.astype(bool)


def _hit(tr, rays):
    rc, h = tr.traceRays(rays)
    assert rc == 0
    return _records(h)[:, 1] != INV


def _occluded(tr, rays):
    rc, occ = tr.occludedRays(rays)
    assert rc == 0 and occ.dtype == np.bool_ and occ.shape == (rays.shape[0],)
    return occ


@pytest.mark.parametrize("engine", ["projection", "bvh"])
def test_sensor_rays_are_occluded_where_the_frame_hits(oracle, capi, sensors, meshes, engine):
    """the sensor's own rays: occluded == ls_trace_rays hit, elementwise, and the occluded rays are those of the frame's ls_hit
    records (ground + ben; the posed scene with a quad mesh)"""
    import torch
    s = sensors["0000"]
    for setup in (lambda tr: _ground_ben(tr, oracle, meshes), lambda tr: _scene_posed_quads(oracle, capi, tr, meshes)):
        tr = make_tracer(capi, s, engine)
        setup(tr)
        rc, _, hits = tr.traceScene(0)
        assert rc == 0 and hits.shape[0] > 0
        d_rays, n = _sensor_rays(tr)
        occ = _occluded_device(tr, d_rays, n)
        out = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert tr.traceRaysDevice(d_rays.data_ptr(), n, out.data_ptr()) == 0
        tr.synchronize()
        torch.cuda.synchronize()
        closest = out.cpu().numpy().view(np.uint32).reshape(n, 4)
        assert np.array_equal(occ, closest[:, 1] != INV)
        assert np.array_equal(np.nonzero(occ)[0], np.sort(hits["ray"]))
        tr.close()


def test_arbitrary_rays_and_ranges_equal_the_brute_force(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    scene = oracle.assemble_scene(s, ml)
    rng = np.random.default_rng(23)
    rays = _random_rays(rng, 600, scene.verts.mean(0), 25.0, 1e3)
    # random finite ranges on two thirds of them
    k = rng.uniform(size=600) < 2 / 3
    rays[k, 3] = rng.uniform(0.0, 10.0, np.count_nonzero(k))
    rays[k, 7] = rays[k, 3] + rng.uniform(0.0, 30.0, np.count_nonzero(k))
    want = _brute(oracle, scene, rays)[:, 1] != INV
    assert 100 < np.count_nonzero(want) < 500
    got = _occluded(tr, rays)
    assert np.array_equal(got, want)
    assert np.array_equal(got, _hit(tr, rays))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_range_edges(oracle, capi, sensors, meshes):
    """tmax = the closest hit's t: occluded; tmin = tmax = t: occluded; tmax one ulp short: as the brute force"""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    scene = oracle.assemble_scene(s, ml)
    rays = _random_rays(np.random.default_rng(29), 800, scene.verts.mean(0), 20.0, 200.0)
    rc, h = tr.traceRays(rays)
    rec = _records(h)
    rays = rays[rec[:, 1] != INV]
    t = rec[rec[:, 1] != INV, 3].view(np.float32)
    assert rays.shape[0] > 150
    at = rays.copy()
    at[:, 7] = t
    assert np.all(_occluded(tr, at))
    exact = at.copy()
    exact[:, 3] = t
    assert np.all(_occluded(tr, exact))
    short = rays.copy()
    short[:, 7] = np.nextafter(t, np.float32(0))
    got = _occluded(tr, short)
    assert np.array_equal(got, _brute(oracle, scene, short)[:, 1] != INV)
    assert np.array_equal(got, _hit(tr, short))
    tr.close()


def test_degenerate_rays_are_not_occluded(oracle, capi, sensors, meshes):
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
    got = _occluded(tr, rays)
    assert got[0] and got[-1] and not np.any(got[1:-1])
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_forty_geometries_in_three_launches(oracle, capi, sensors, meshes):
    """40 geometries (launches over geometries 0-15, 16-31, 32-39), singular and ill-conditioned poses among them: rays occluded
    only in the first batch, only in the last, in both -- equal to ls_trace_rays and the brute force"""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    rng = np.random.default_rng(31)
    ml = [(0, *meshes["ground"], oracle.IDENTITY_AFFINE)]
    _add(tr, "g0", *meshes["ground"])
    tr.updateGeometry("g0", oracle.IDENTITY_AFFINE, *meshes["ground"])
    for k in range(1, 40):
        A = oracle.affine_from_components(np.float32(rng.uniform(-15, 15, 3) * [1, 1, 0]), np.float32(rng.uniform(-1, 1, 3)))
        if k in (4, 35):
            A = np.zeros(12, np.float32)                                            # scaled to zero: no inverse
            A[3], A[7] = 2.0, 2.0
        if k in (9, 37):
            A = np.float32([1.0, 0, 0, -3.0, 0, 1e-3 / 2, 0, 4.0, 0, 0, 0.5, 0.5])   # 2000 : 1
        if k in (15, 38):
            A = np.float32([0.8, 0, 0, 6.0, 0, 0.8e-4, 0, -4.0, 0, 0, 0.4, 0.5])   # 10 000 : 1: kept in the sensor frame
        _add(tr, f"g{k}", *meshes["ben"])
        tr.updateGeometry(f"g{k}", A, *meshes["ben"])
        ml.append((k, *meshes["ben"], A))
    assert tr.commitScene() == 0
    scene = oracle.assemble_scene(s, ml)
    # half the rays aim at the middle of a geometry of the last batch -- a quarter end there (tmax = 1), a quarter go on (often
    # onto the ground) --, the rest go anywhere
    n = 360
    rays = _random_rays(rng, n, scene.verts.mean(0), 20.0, 300.0)
    centres = [oracle.assemble_scene(s, [ml[k]]).verts.mean(0) for k in (32, 33, 34, 36, 39)]
    aim = np.arange(n) < n // 2
    tgt = np.stack([centres[i % len(centres)] for i in range(n)]) + rng.uniform(-0.3, 0.3, (n, 3))
    rays[aim, 4:7] = (tgt - rays[:, 0:3])[aim]
    rays[: n // 4, 7] = 1.0
    got = _occluded(tr, rays)
    assert np.array_equal(got, _hit(tr, rays))
    # the brute force without the two geometries scaled to zero: their triangles are points, which the exact test never hits
    # (and which would be candidates of every ray there)
    assert np.all(oracle.assemble_scene(s, [ml[4], ml[35]]).verts == np.float32(oracle.assemble_scene(s, [ml[4]]).verts[0]))
    live = [m for k, m in enumerate(ml) if k not in (4, 35)]
    assert np.array_equal(got, _brute(oracle, oracle.assemble_scene(s, live), rays)[:, 1] != INV)
    first = _brute(oracle, oracle.assemble_scene(s, live[:15]), rays)[:, 1] != INV   # geometries 0-15
    last = _brute(oracle, oracle.assemble_scene(s, live[31:]), rays)[:, 1] != INV    # geometries 32-39
    assert np.count_nonzero(first & ~last) > 10 and np.count_nonzero(last & ~first) > 10 and np.count_nonzero(first & last) > 10
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 0   # (built by the first query above)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_segments_from_the_sensor_to_ground_points(oracle, capi, sensors, meshes):
    """A -> B with d = B - A, tmax = 1 - 1e-4: B on the ground is not occluded by its own triangle, ben in the way occludes"""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    A_ben = oracle.affine_from_components(np.float32([4.0, 1.0, 0.0]), np.float32([0.0, 0.0, 0.3]))
    ml = _ground_ben(tr, oracle, meshes, A_ben)
    scene = oracle.assemble_scene(s, ml)
    ground = oracle.assemble_scene(s, ml[:1])
    rng = np.random.default_rng(37)
    n = 1500
    tri = ground.tris[rng.integers(0, ground.tris.shape[0], n)]
    w = rng.dirichlet([1, 1, 1], n)
    B = np.einsum("nk,nkj->nj", w, ground.verts[tri].astype(np.float64))
    # half of the targets behind ben as the sensor sees it
    ben_c = oracle.assemble_scene(s, ml[1:]).verts.mean(0).astype(np.float64)
    B[: n // 2] = ben_c * rng.uniform(1.2, 3.0, (n // 2, 1)) + rng.normal(scale=0.5, size=(n // 2, 3))
    rays = np.zeros((n, 8), np.float32)
    rays[:, 4:7] = B                       # the sensor origin (0, 0, 0) of the sensor frame to B
    rays[:, 7] = 1.0 - 1e-4
    want = _brute(oracle, scene, rays)[:, 1] != INV
    assert 50 < np.count_nonzero(want) < n - 50
    assert np.array_equal(_occluded(tr, rays), want)
    tr.close()


def test_entry_points(oracle, capi, sensors, meshes):
    """host == device; a non-default stream; any output alignment and guard bytes; n = 0; refused arguments; a removed
    geometry; no commit: -1 and out untouched.  (LS_ERR_NOT_COMMITTED, a layout entry whose geometry is gone or changed, is
    not reachable through the public entry points: ls_remove_geometry commits the remaining scene itself, a failed commit
    leaves no commit -- -1 --, and a geometry's id and triangle count are fixed when it is added.)"""
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    scene = oracle.assemble_scene(s, ml)
    rays = _random_rays(np.random.default_rng(41), 4000, scene.verts.mean(0), 25.0, 500.0)
    host = _occluded(tr, rays)
    assert 500 < np.count_nonzero(host) < 3500
    d = torch.from_numpy(rays.view(np.uint8).reshape(-1)).to("cuda:0")
    assert np.array_equal(_occluded_device(tr, d, 4000), host)
    st = torch.cuda.Stream()
    for off in (0, 1, 3):
        assert np.array_equal(_occluded_device(tr, d, 4000, st.cuda_stream, off), host)
    assert np.array_equal(_occluded_device(tr, d, 17, None, 5), host[:17])
    # n = 0 writes nothing
    buf = torch.full((GUARD,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert tr.occludedRaysDevice(d.data_ptr(), 0, buf.data_ptr()) == 0
    assert tr.occludedRaysDevice(0, 0, 0) == 0
    assert tr.occludedRays(np.zeros((0, 8), np.float32))[0] == 0
    with pytest.raises(capi.LidarShooterHipError):
        tr.occludedRaysDevice(0, 4, 0)
    with pytest.raises(capi.LidarShooterHipError):
        tr.occludedRaysDevice(d.data_ptr() + 8, 4, buf.data_ptr())   # rays must be 16-byte aligned
    tr.synchronize()
    assert np.all(buf.cpu().numpy() == 0xAB)
    # a removal commits the remaining scene (EmbreeTracer's behaviour): the query follows it, as ls_trace_rays does
    assert tr.removeGeometry("face") >= 0
    after = _occluded(tr, rays)
    assert np.array_equal(after, _hit(tr, rays))
    assert np.array_equal(after, _brute(oracle, oracle.assemble_scene(s, [ml[0], ml[2]]), rays)[:, 1] != INV)
    assert np.count_nonzero(after) < np.count_nonzero(host)
    tr.close()
    # no commit: -1, out untouched
    t2 = make_tracer(capi, s)
    assert t2.occludedRaysDevice(d.data_ptr(), 4, buf.data_ptr()) == -1
    rc, occ = t2.occludedRays(rays[:5])
    assert rc == -1 and occ.dtype == np.bool_ and not np.any(occ)
    t2.synchronize()
    assert np.all(buf.cpu().numpy() == 0xAB)
    t2.close()


def test_open_frame_graph_is_refused(oracle, capi, sensors, meshes):
    import torch
    s = sensors["0001"]
    tr = make_tracer(capi, s, "projection")
    tr.setOption(capi.LS_OPT_PIPELINE, 2)
    tr.setOption(capi.LS_OPT_FRAME_GRAPH, 1)
    _ground_ben(tr, oracle, meshes)
    rays, n = _sensor_rays(tr)
    cap = s.V * s.H
    p, h, c = (torch.zeros(32 * cap, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * cap, dtype=torch.uint8, device="cuda:0"),
               torch.zeros(4, dtype=torch.int32, device="cuda:0"))
    tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), cap)
    out = torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L = tr.L
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != FRAME_EAGER   # the frame is being captured: the graph is open
    assert L.ls_occluded_rays(tr.h, None, rays.data_ptr(), n, out.data_ptr()) == INVALID_ARGUMENT
    assert L.ls_occluded_rays_host(tr.h, None, 0, None) == INVALID_ARGUMENT
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB)
    # the frame went out, and the handle answers queries again
    assert int(c[0].item()) > 0
    assert tr.occludedRaysDevice(rays.data_ptr(), n, out.data_ptr()) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.count_nonzero(out.cpu().numpy() == 1) == int(c[0].item())
    tr.close()


def test_shared_query_set(oracle, capi, sensors, meshes):
    """one set for both queries: what ls_trace_rays built serves ls_occluded_rays and the other way round"""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    rays = _random_rays(np.random.default_rng(43), 400, oracle.assemble_scene(s, ml).verts.mean(0), 20.0, 100.0)
    _hit(tr, rays)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 3
    A_new = oracle.affine_from_components(np.float32([-1.0, 2.5, 0.2]), np.float32([0.0, 0.3, -0.7]))
    tr.updateGeometryTransform("face", A_new)
    assert tr.commitScene() == 0
    got = _occluded(tr, rays)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 0
    ml[1] = (1, *meshes["ben"], A_new)
    assert np.array_equal(got, _brute(oracle, oracle.assemble_scene(s, ml), rays)[:, 1] != INV)
    v2 = meshes["ben"][0] * np.float32(1.3)
    tr.updateGeometry("face", A_new, v2, None)
    assert tr.commitScene() == 0
    got = _occluded(tr, rays)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 1
    ml[1] = (1, v2, meshes["ben"][1], A_new)
    want = _brute(oracle, oracle.assemble_scene(s, ml), rays)
    assert np.array_equal(got, want[:, 1] != INV)
    rc, h = tr.traceRays(rays)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 0
    assert np.array_equal(_records(h), want)
    tr.close()


def test_frames_are_unaffected_by_occlusion_queries(oracle, capi, sensors, meshes):
    """three-stream frames with frame graphs, occlusion queries on another stream between them: the same clouds as without"""
    import hashlib

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
        rays, n = _sensor_rays(tr)
        qs = torch.cuda.Stream()
        outs = [torch.zeros(n, dtype=torch.uint8, device="cuda:0") for _ in range(5)]
        bufs = [(torch.zeros(32 * cap, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * cap, dtype=torch.uint8, device="cuda:0"),
                 torch.zeros(4, dtype=torch.int32, device="cuda:0")) for _ in range(9)]
        torch.cuda.synchronize()
        for i in range(9):
            p, h, c = bufs[i]
            tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), cap)
            tr.traceSceneAsync(i)
            if with_queries and i % 2 == 0:
                assert tr.occludedRaysDevice(rays.data_ptr(), n, outs[i // 2].data_ptr(), qs.cuda_stream) == 0
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
            for o in outs:
                assert np.array_equal(o.cpu().numpy().astype(bool), ref["gid"] != INV)
        assert tr.info(capi.LS_INFO_FRAME_GRAPH_STATE) == 1
        tr.close()
        return digests

    assert run(True) == run(False)
