"""ls_trace_scene_sweep / ls_trace_scene_sweep_host on the MI355X: frames whose sensor moves during the turn.  Identity poses
against the frame; a real twist against the rays restated in numpy (test_sweep_cpu.restate_rays) and the brute force of
test_gpu_rays over the oracle's scene; deskewed points and d_rays_out against ls_hit_attributes and ls_apply_return_model; azimuth
shards, a NaN pose, the compaction across wave and workgroup boundaries, two launch batches, return codes, frames around a sweep,
host against device.  Everything is compared bit for bit."""
import ctypes

import numpy as np
import pytest

from conftest import make_tracer
from test_gpu_rays import INV, _add, _brute, _from_gid, _ground_ben
from test_sweep_cpu import IDENTITY_POSE, restate_rays

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = -2                      # LS_ERR_INVALID_ARGUMENT
FRAME_EAGER = 0
FILL = 0xAB
F = np.float32
# a carrier at about 10 m/s turning at about 1 rad/s, one turn of the sensor in 0.1 s
LIN_VEL, ANG_VEL, TURN = (8.0, -5.0, 0.5), (0.1, -0.15, 1.0), 0.1


# ---- expectations ----------------------------------------------------------------------------------------------------------

def _twist_poses(capi, s):
    return capi.sweep_poses_constant_twist(LIN_VEL, ANG_VEL, 0.0, TURN / s.H, s.H)


def _all_rays(oracle, s, pose):
    """the ray records of the full raster, global index r = v * H + h, under the per-column poses"""
    return restate_rays(oracle.ray_dirs(s), pose[np.arange(s.V * s.H) % s.H])


def _points(xyz, ring, intensity=64.0):
    p = np.zeros((xyz.shape[0], 8), np.uint32)
    p[:, 0:3] = np.ascontiguousarray(xyz, np.float32).view(np.uint32)
    p[:, 4] = F(intensity).view(np.uint32)
    p[:, 5] = ring
    return p.view(np.uint8).reshape(-1, 32)


def _expect(oracle, s, dense, rays, deskew=False):
    """dense ls_hit records of the full raster (global ray index) -> (the hits in ascending ray index, their points): xyz =
    float32(t) * d, or o + t * d' (one product, one sum) when deskewing; intensity 64, ring v"""
    hit = dense[dense[:, 1] != INV]
    r = hit[:, 0].astype(np.int64)
    t = hit[:, 3].view(np.float32)
    if deskew:
        xyz = rays[r, 0:3] + t[:, None] * rays[r, 4:7]
    else:
        xyz = t[:, None] * oracle.ray_dirs(s)[r]
    return hit, _points(xyz.astype(np.float32), (r // s.H).astype(np.uint32))


_cache = {}


def _xt32(oracle, capi, sensors, meshes):
    """XT-32 0000 over ground + ben under the twist: the scene, the poses, the restated rays and the brute force's dense records --
    computed once, shared by the tests that need them, never changed"""
    if "xt32" not in _cache:
        s = sensors["0000"]
        ml = [(0, *meshes["ground"], oracle.IDENTITY_AFFINE), (1, *meshes["ben"], oracle.IDENTITY_AFFINE)]
        scene = oracle.assemble_scene(s, ml)
        pose = _twist_poses(capi, s)
        rays = _all_rays(oracle, s, pose)
        dense = _brute(oracle, scene, rays)
        for a in (pose, rays, dense):
            a.setflags(write=False)
        _cache["xt32"] = (s, ml, scene, pose, rays, dense)
    return _cache["xt32"]


# ---- the device entry point ------------------------------------------------------------------------------------------------

def _sweep(tr, pose, flags=0, points=True, hits=True, rays=False, stream=None):
    """ls_trace_scene_sweep with capacity exactly the shard's ray count and one canary record behind every buffer -> (k,
    points uint8 (k, 32) | None, hits uint32 (k, 4) | None, rays float32 (V * H, 8) | None); whatever lies past record k, the
    canary included, must still hold the fill pattern"""
    import torch
    n = tr.getTotalRays()
    d_pose = torch.from_numpy(np.array(pose, np.float32)).to("cuda:0")
    p = torch.full(((n + 1) * 32,), FILL, dtype=torch.uint8, device="cuda:0") if points else None
    h = torch.full(((n + 1) * 16,), FILL, dtype=torch.uint8, device="cuda:0") if hits else None
    c = torch.full((16,), FILL, dtype=torch.uint8, device="cuda:0")
    r = torch.full((tr.V * tr.H * 32,), FILL, dtype=torch.uint8, device="cuda:0") if rays else None
    torch.cuda.synchronize()
    rc = tr.traceSweepDevice(d_pose.data_ptr(), pose.shape[0], c.data_ptr(), n, p.data_ptr() if points else 0, h.data_ptr() if hits else 0,
                             r.data_ptr() if rays else 0, flags=flags, stream=stream)
    assert rc == 0
    tr.synchronize()
    torch.cuda.synchronize()
    cw = c.cpu().numpy()
    k = int(cw[:4].view(np.uint32)[0])
    assert 0 <= k <= n and np.all(cw[4:] == FILL)
    out = [k, None, None, None]
    if points:
        a = p.cpu().numpy().reshape(n + 1, 32)
        assert np.all(a[k:] == FILL), "a point record written past the count"
        out[1] = a[:k].copy()
    if hits:
        a = h.cpu().numpy().reshape(n + 1, 16)
        assert np.all(a[k:] == FILL), "a hit record written past the count"
        out[2] = a[:k].copy().view(np.uint32).reshape(k, 4)
    if rays:
        out[3] = r.cpu().numpy().view(np.float32).reshape(tr.V * tr.H, 8)
    return tuple(out)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- 1. identity poses reproduce the frame ---------------------------------------------------------------------------------

@pytest.mark.parametrize("engine", ["projection", "bvh"])
def test_identity_poses_reproduce_the_frame(oracle, capi, sensors, meshes, engine):
    """points32, hits and count of ls_trace_scene, on both engines of the frame side: the reference's 1668 points over the ground,
    1781 over ground + ben"""
    s = sensors["0000"]
    pose = np.tile(IDENTITY_POSE, (s.H, 1))
    for with_ben, known in ((False, 1668), (True, 1781)):
        tr = make_tracer(capi, s, engine)
        if with_ben:
            _ground_ben(tr, oracle, meshes)
        else:
            _add(tr, "ground", *meshes["ground"])
            tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *meshes["ground"])
            assert tr.commitScene() == 0
        rc, pts, hits = tr.traceScene(0)
        assert rc == 0 and len(pts) == known
        k, p, h, _ = _sweep(tr, pose)
        assert k == known
        assert _same_bits(p, np.asarray(pts).reshape(-1, 32))
        assert np.array_equal(h, np.stack([hits["ray"], hits["geom"], hits["prim"], hits["t"].view(np.uint32)], axis=1))
        assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == (2 if with_ben else 1)
        # the deskewed points of an identity table: 0 + t * d, the same bits but for the sign of a zero
        k2, p2, h2, _ = _sweep(tr, pose, flags=capi.LS_SWEEP_DESKEW)
        assert k2 == k and np.array_equal(h2, h) and np.array_equal(p2.view(np.float32), p.view(np.float32))
        assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 0
        tr.close()


# ---- 2. a real twist equals the brute force --------------------------------------------------------------------------------

def test_twist_equals_the_brute_force(oracle, capi, sensors, meshes):
    s, ml, scene, pose, rays, dense = _xt32(oracle, capi, sensors, meshes)
    # the twist matters: the brute force alone differs from the static frame in at least 100 records
    ref = oracle.trace_frame(s, ml)
    static = _from_gid(scene, ref["t"], ref["gid"])
    assert np.count_nonzero(np.any(dense != static, axis=1)) >= 100
    assert np.count_nonzero((dense[:, 1] != INV) != (static[:, 1] != INV)) >= 50
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    k, p, h, _ = _sweep(tr, pose)
    want_h, want_p = _expect(oracle, s, dense, rays)
    assert k == len(want_h) and set(want_h[:, 1]) == {0, 1}
    assert np.array_equal(h, want_h)
    assert _same_bits(p, want_p)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 3. LS_SWEEP_DESKEW and d_rays_out -------------------------------------------------------------------------------------

def test_deskew_and_rays_out_feed_attributes_and_returns(oracle, capi, sensors, meshes):
    import torch
    s, ml, scene, pose, rays, dense = _xt32(oracle, capi, sensors, meshes)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    k, p, h, r = _sweep(tr, pose, flags=capi.LS_SWEEP_DESKEW, rays=True)
    assert _same_bits(r, rays)                                   # the rays equal the restated ones
    want_h, want_p = _expect(oracle, s, dense, rays, deskew=True)
    assert np.array_equal(h, want_h) and _same_bits(p, want_p)
    # ls_hit_attributes over (d_rays_out, hits): every record valid, its point the deskewed xyz
    d_rays = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_hits = torch.from_numpy(h.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_attr = torch.zeros(k * 48, dtype=torch.uint8, device="cuda:0")
    d_n = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    d_pts = torch.zeros(k * 32, dtype=torch.uint8, device="cuda:0")
    d_out = torch.zeros(k * 16, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()   # (the fills run on torch's stream, the queries on the handle's: fills first)
    assert tr.hitAttributesDevice(d_hits.data_ptr(), k, d_attr.data_ptr(), d_rays=d_rays.data_ptr(), n_rays=s.V * s.H) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    attr = d_attr.cpu().numpy().view(capi.HIT_ATTR_DTYPE)
    assert np.all(attr["flags"] == 1) and np.array_equal(attr["ray"], h[:, 0])
    assert _same_bits(attr["p"], p[:, 0:12].copy().view(np.float32).reshape(k, 3))
    # the identity return model over the same pair keeps every record (ring 0: caller rays)
    m = capi.ReturnModel()
    assert m.intensity_scale == 64.0 and m.flags == 0
    assert tr.applyReturnModelDevice(m, d_hits.data_ptr(), k, d_n.data_ptr(), d_points32=d_pts.data_ptr(), d_hits_out=d_out.data_ptr(),
                                     d_rays=d_rays.data_ptr(), n_rays=s.V * s.H) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert int(d_n[0].item()) == k
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32).reshape(k, 4), h)
    ring0 = p.copy()
    ring0[:, 20:24] = 0
    assert _same_bits(d_pts.cpu().numpy().reshape(k, 32), ring0)
    tr.close()


# ---- 4. a shard not aligned to anything ------------------------------------------------------------------------------------

def test_unaligned_shard_is_the_full_turn_restricted(oracle, capi, sensors, meshes):
    s, ml, scene, pose, rays, dense = _xt32(oracle, capi, sensors, meshes)
    first, count = 37, 61
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for flags in (0, capi.LS_SWEEP_DESKEW):
        tr.setShard(0, s.H)
        kf, pf, hf, rf = _sweep(tr, pose, flags=flags, rays=True)
        tr.setShard(first, count)
        assert tr.getTotalRays() == s.V * count
        k, p, h, r = _sweep(tr, pose, flags=flags, rays=True)      # the table is still indexed by the global column
        col = hf[:, 0] % s.H
        inside = (col >= first) & (col < first + count)
        assert 100 < np.count_nonzero(inside) < kf
        assert k == np.count_nonzero(inside) and np.array_equal(h, hf[inside]) and _same_bits(p, pf[inside])
        cols = np.arange(s.V * s.H) % s.H
        mine = (cols >= first) & (cols < first + count)
        assert _same_bits(r[mine], rf[mine]) and _same_bits(r[mine], rays[mine])
        assert np.all(r[~mine].view(np.uint8) == FILL)           # the other records keep their fill pattern
    tr.close()


# ---- 5. a NaN in one column's pose -----------------------------------------------------------------------------------------

def test_nan_pose_column_misses(oracle, capi, sensors, meshes):
    s, ml, scene, pose, rays, dense = _xt32(oracle, capi, sensors, meshes)
    want_h, want_p = _expect(oracle, s, dense, rays)
    hits_per_col = np.bincount(want_h[:, 0] % s.H, minlength=s.H)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for col, entry in ((int(np.argmax(hits_per_col)), 5), (3, 7), (s.H - 1, 0)):
        assert hits_per_col[col] > 0
        bad = pose.copy()
        bad[col, entry] = np.nan
        k, p, h, r = _sweep(tr, bad, rays=True)
        keep = want_h[:, 0] % s.H != col
        assert k == np.count_nonzero(keep) and np.array_equal(h, want_h[keep]) and _same_bits(p, want_p[keep])
        cols = np.arange(s.V * s.H) % s.H
        assert _same_bits(r[cols != col], rays[cols != col])
        assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 6. compaction across block and wave boundaries --------------------------------------------------------------------------

def _syn_sensor(oracle, sensors):
    from lidarshooter_amd import synth
    s0 = sensors["0000"]
    return oracle.Sensor(uid="syn", vertical=synth.syn_vertical(64), h_begin=np.float32(0.0), h_end=np.float32(360.0), h_count=96,
                         R=s0.R, Rinv=s0.Rinv, t=s0.t)


def _box_around(center, half):
    """a closed box, 12 triangles: every ray from inside hits"""
    c = np.asarray(center, np.float64)
    v = np.array([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], np.float64) + c
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = [tri for a, b, c_, d in q for tri in ((a, b, c_), (a, c_, d))]
    return v.astype(np.float32), np.array(t, np.uint32)


def _holed_grid():
    """a relief grid with a random half of its cells removed: hits and misses alternate irregularly along every ring"""
    from lidarshooter_amd import synth
    v, t = synth.grid_mesh(48, 40)
    keep = np.random.default_rng(61).permutation(48 * 40) < 48 * 20
    return v, np.ascontiguousarray(t.reshape(48 * 40, 2, 3)[keep].reshape(-1, 3))


@pytest.mark.parametrize("which", ["every_ray_hits", "holed_grid"])
def test_compaction_across_wave_and_block_boundaries(oracle, capi, sensors, which):
    s = _syn_sensor(oracle, sensors)
    n = s.V * s.H
    assert n == 24 * 256 and s.H % 64 != 0
    mesh = _box_around(s.t, 40.0) if which == "every_ray_hits" else _holed_grid()
    ml = [(0, *mesh, oracle.IDENTITY_AFFINE)]
    scene = oracle.assemble_scene(s, ml)
    pose = _twist_poses(capi, s)
    rays = _all_rays(oracle, s, pose)
    dense = _brute(oracle, scene, rays)
    hit = dense[:, 1] != INV
    if which == "every_ray_hits":
        assert np.all(hit)
    else:
        # irregular: hits in every 256-ray block of the lower rings, many changes between hit and miss, no block all of one kind there
        per_block = hit.reshape(-1, 256).sum(1)
        assert 1000 < hit.sum() < n - 1000 and np.count_nonzero(hit[1:] != hit[:-1]) > 500
        assert np.count_nonzero((per_block > 0) & (per_block < 256)) >= 8 and len(set(hit.reshape(-1, 64).sum(1))) > 10
    tr = make_tracer(capi, s)
    _add(tr, "mesh", *mesh)
    tr.updateGeometry("mesh", oracle.IDENTITY_AFFINE, *mesh)
    assert tr.commitScene() == 0
    for flags in (0, capi.LS_SWEEP_DESKEW):
        k, p, h, r = _sweep(tr, pose, flags=flags, rays=True)
        want_h, want_p = _expect(oracle, s, dense, rays, deskew=bool(flags))
        assert k == len(want_h) and np.array_equal(h, want_h) and _same_bits(p, want_p) and _same_bits(r, rays)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 7. eighteen geometries, one of them a quad mesh: two launch batches -----------------------------------------------------

def _eighteen(oracle, capi, s, meshes):
    """the ground and seventeen small plates around the sensor (6 x 4 cells, tilted, posed), number 16 a quad mesh; the last two
    belong to the second launch batch"""
    xs, ys = np.meshgrid(np.linspace(-3, 3, 7), np.linspace(-2, 2, 5), indexing="xy")
    pv = np.stack([xs, ys, 0.3 * xs], -1).reshape(-1, 3).astype(np.float32)
    pq = np.array([[j * 7 + i, j * 7 + i + 1, j * 7 + i + 8, j * 7 + i + 7] for j in range(4) for i in range(6)], np.uint32)
    pt = oracle.quads_to_triangles(pq)
    rng = np.random.default_rng(18)
    geoms = [("g0", meshes["ground"][0], meshes["ground"][1], oracle.IDENTITY_AFFINE, 0)]
    for k in range(1, 18):
        ang = 2 * np.pi * k / 17
        dist = 7.0 + 0.6 * k
        lin = np.float32([s.t[0] + dist * np.cos(ang), s.t[1] + dist * np.sin(ang), s.t[2] - 2.0 + rng.uniform(-1.5, 1.5)])
        A = oracle.affine_from_components(lin, np.float32([rng.uniform(-0.3, 0.3), 1.2 + rng.uniform(-0.3, 0.3), ang]))
        geoms.append((f"g{k}", pv, pq if k == 16 else pt, A, capi.LS_GEOMETRY_TYPE_QUAD if k == 16 else 0))
    return geoms


def test_eighteen_geometries_two_batches_and_the_canary(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    geoms = _eighteen(oracle, capi, s, meshes)
    ml = [(i, v, e, A) for i, (name, v, e, A, gt) in enumerate(geoms)]
    scene = oracle.assemble_scene(s, ml)
    pose = _twist_poses(capi, s)
    rays = _all_rays(oracle, s, pose)
    dense = _brute(oracle, scene, rays)
    seen = set(dense[:, 1]) - {INV}
    assert {0, 16, 17} <= seen and len(seen) >= 12     # both batches, the quad mesh among them
    tr = make_tracer(capi, s)
    for name, v, e, A, gt in geoms:
        _add(tr, name, v, e, gt)
        tr.updateGeometry(name, A, v, e)
    assert tr.commitScene() == 0
    # (_sweep: capacity is exactly the ray count, one canary record lies behind it and is checked)
    k, p, h, r = _sweep(tr, pose, rays=True)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 18
    want_h, want_p = _expect(oracle, s, dense, rays)
    assert k == len(want_h) and np.array_equal(h, want_h) and _same_bits(p, want_p) and _same_bits(r, rays)
    tr.close()


# ---- 8. return codes -------------------------------------------------------------------------------------------------------

def test_return_codes(oracle, capi, sensors, meshes):
    import torch
    s, ml, scene, pose, rays, dense = _xt32(oracle, capi, sensors, meshes)
    n = s.V * s.H
    d_pose = torch.from_numpy(np.array(pose, np.float32)).to("cuda:0")
    bufs = {k: torch.full((size,), FILL, dtype=torch.uint8, device="cuda:0") for k, size in
            (("p", n * 32 + 64), ("h", n * 16 + 64), ("c", 64), ("r", n * 32 + 64))}
    torch.cuda.synchronize()
    P, H_, C_, R = (bufs[k].data_ptr() for k in "phcr")
    host_n = ctypes.c_uint32(0xABABABAB)
    host_p, host_h = np.full((n, 32), FILL, np.uint8), np.full((n, 16), FILL, np.uint8)

    def untouched():
        torch.cuda.synchronize()
        return all(np.all(b.cpu().numpy() == FILL) for b in bufs.values()) and host_n.value == 0xABABABAB and \
            np.all(host_p == FILL) and np.all(host_h == FILL)

    def both(tr):
        return (tr.L.ls_trace_scene_sweep(tr.h, None, d_pose.data_ptr(), s.H, 0, P, H_, C_, n, R),
                tr.L.ls_trace_scene_sweep_host(tr.h, pose.ctypes.data, s.H, 0, host_p.ctypes.data, host_h.ctypes.data, ctypes.byref(host_n), n, None))

    tr = make_tracer(capi, s)
    assert both(tr) == (-1, -1) and untouched()                     # before a commit
    _add(tr, "ground", *meshes["ground"])
    _add(tr, "face", *meshes["ben"])
    assert both(tr) == (-1, -1) and untouched()                     # geometries without a commit
    tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *meshes["ground"])
    tr.updateGeometry("face", oracle.IDENTITY_AFFINE, *meshes["ben"])
    assert tr.commitScene() == 0
    L, h = tr.L, tr.h
    sweep, host = L.ls_trace_scene_sweep, L.ls_trace_scene_sweep_host
    pd, ph = d_pose.data_ptr(), pose.ctypes.data
    refused = [
        sweep(h, None, pd, s.H - 1, 0, P, H_, C_, n, R), sweep(h, None, pd, s.H + 1, 0, P, H_, C_, n, R),      # n_cols != H
        host(h, ph, s.H - 1, 0, None, None, ctypes.byref(host_n), n, None),
        sweep(h, None, pd, s.H, 0, P, H_, C_, n - 1, R), host(h, ph, s.H, 0, None, None, ctypes.byref(host_n), n - 1, None),   # a small capacity
        sweep(h, None, pd, s.H, 0, P + 8, H_, C_, n, R), sweep(h, None, pd, s.H, 0, P, H_ + 8, C_, n, R),      # misaligned buffers
        sweep(h, None, pd, s.H, 0, P, H_, C_, n, R + 16 - 4), sweep(h, None, pd, s.H, 0, P, H_, C_ + 2, n, R),
        sweep(h, None, pd + 2, s.H, 0, P, H_, C_, n, R),
        sweep(h, None, pd, s.H, 0, P, H_, None, n, R), host(h, ph, s.H, 0, None, None, None, n, None),          # NULL count
        sweep(h, None, None, s.H, 0, P, H_, C_, n, R), host(h, None, s.H, 0, None, None, ctypes.byref(host_n), n, None),
        sweep(h, None, pd, s.H, 2, P, H_, C_, n, R), sweep(h, None, pd, s.H, 0x80000001, P, H_, C_, n, R),      # unknown flags
        host(h, ph, s.H, 4, None, None, ctypes.byref(host_n), n, None),
    ]
    assert refused == [INVALID_ARGUMENT] * len(refused) and untouched()
    assert tr.last_error()
    # a shard: the capacity that counts is the shard's
    tr.setShard(10, 20)
    assert sweep(h, None, pd, s.H, 0, P, H_, C_, s.V * 20 - 1, R) == INVALID_ARGUMENT and untouched()
    assert sweep(h, None, pd, 20, 0, P, H_, C_, n, R) == INVALID_ARGUMENT and untouched()
    tr.setShard(0, s.H)
    # the handle still answers
    k, p, hh, _ = _sweep(tr, pose)
    want_h, want_p = _expect(oracle, s, dense, rays)
    assert np.array_equal(hh, want_h)
    # A removal commits the remaining scene itself (EmbreeTracer's behaviour, ls_remove_geometry): LS_ERR_NOT_COMMITTED -- a layout
    # entry whose geometry is gone -- is not reachable through the public entry points, for this query as for ls_trace_rays.  The
    # sweep returns what ls_trace_rays returns in the same state and follows the remaining scene; an emptied scene: -1.
    assert tr.removeGeometry("face") >= 0
    probe = torch.zeros(32, dtype=torch.uint8, device="cuda:0")
    out = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert L.ls_trace_rays(h, None, probe.data_ptr(), 1, out.data_ptr()) == 0
    k2, p2, h2, _ = _sweep(tr, pose)
    ground_only = dense[:, 1] == 0
    assert 0 < k2 < k and np.all(h2[:, 1] == 0)
    assert np.array_equal(h2[np.isin(h2[:, 0], dense[ground_only, 0])], want_h[want_h[:, 1] == 0])   # what the ground alone showed stays
    assert tr.removeGeometry("ground") >= 0
    assert L.ls_trace_rays(h, None, probe.data_ptr(), 1, out.data_ptr()) == -1
    assert both(tr) == (-1, -1) and untouched()                     # an empty scene
    tr.close()


def test_open_frame_graph_is_refused(oracle, capi, sensors, meshes):
    import torch
    s = sensors["0001"]
    tr = make_tracer(capi, s, "projection")
    tr.setOption(capi.LS_OPT_PIPELINE, 2)
    tr.setOption(capi.LS_OPT_FRAME_GRAPH, 1)
    _ground_ben(tr, oracle, meshes)
    n = s.V * s.H
    pose = np.tile(IDENTITY_POSE, (s.H, 1))
    d_pose = torch.from_numpy(pose).to("cuda:0")
    p, h, c = (torch.zeros(32 * n, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * n, dtype=torch.uint8, device="cuda:0"),
               torch.zeros(4, dtype=torch.int32, device="cuda:0"))
    tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), n)
    out = torch.full((n * 16 + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L = tr.L
    host_n = ctypes.c_uint32(7)
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != FRAME_EAGER   # the frame is being captured: the graph is open
    assert L.ls_trace_scene_sweep(tr.h, None, d_pose.data_ptr(), s.H, 0, None, out.data_ptr() + 16, out.data_ptr(), n, None) == INVALID_ARGUMENT
    assert L.ls_trace_scene_sweep_host(tr.h, pose.ctypes.data, s.H, 0, None, None, ctypes.byref(host_n), n, None) == INVALID_ARGUMENT
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == FILL) and host_n.value == 7
    # the frame went out, and the handle sweeps again: the identity table gives that frame
    k_frame = int(c[0].item())
    assert k_frame > 0
    k, _, hh, _ = _sweep(tr, pose)
    assert k == k_frame and _same_bits(hh, h.cpu().numpy()[:16 * k].view(np.uint32).reshape(k, 4))
    tr.close()


# ---- 9. frames are unaffected ----------------------------------------------------------------------------------------------

def test_frames_around_a_sweep_on_a_caller_stream(oracle, capi, sensors, meshes):
    """LS_OPT_PIPELINE = 2: a frame, a sweep on a caller stream, a frame again -- both frames the oracle's cloud, the sweep the same
    sweep on the handle's stream"""
    import torch
    s, ml, scene, pose, rays, dense = _xt32(oracle, capi, sensors, meshes)
    ref = oracle.trace_frame(s, ml)
    n = s.V * s.H
    tr = make_tracer(capi, s, "projection")
    tr.setOption(capi.LS_OPT_PIPELINE, 2)
    _ground_ben(tr, oracle, meshes)
    qs = torch.cuda.Stream()
    d_pose = torch.from_numpy(np.array(pose, np.float32)).to("cuda:0")
    frames = [(torch.zeros(32 * n, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * n, dtype=torch.uint8, device="cuda:0"),
               torch.zeros(4, dtype=torch.int32, device="cuda:0")) for _ in range(4)]
    sp, sh, sc = (torch.full((32 * n,), FILL, dtype=torch.uint8, device="cuda:0"), torch.full((16 * n,), FILL, dtype=torch.uint8, device="cuda:0"),
                  torch.zeros(4, dtype=torch.int32, device="cuda:0"))
    torch.cuda.synchronize()
    for i, (p, h, c) in enumerate(frames):
        tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), n)
        tr.traceSceneAsync(i)
        if i == 1:
            assert tr.traceSweepDevice(d_pose.data_ptr(), s.H, sc.data_ptr(), n, sp.data_ptr(), sh.data_ptr(), stream=qs.cuda_stream) == 0
    tr.flush()
    tr.synchronize()
    torch.cuda.synchronize()
    for p, h, c in frames:
        k = int(c[0].item())
        assert k == len(ref["points"]) and np.array_equal(p.cpu().numpy()[:32 * k].reshape(k, 32), ref["points"])
    k = int(sc[0].item())
    k2, p2, h2, _ = _sweep(tr, pose)                               # the handle's stream
    assert k == k2 and _same_bits(sp.cpu().numpy()[:32 * k].reshape(k, 32), p2)
    assert _same_bits(sh.cpu().numpy()[:16 * k].view(np.uint32).reshape(k, 4), h2)
    want_h, want_p = _expect(oracle, s, dense, rays)
    assert np.array_equal(h2, want_h) and _same_bits(p2, want_p)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 10. the host entry point equals the device entry point ------------------------------------------------------------------

def test_host_entry_point_equals_device_entry_point(oracle, capi, sensors, meshes):
    s, ml, scene, pose, rays, dense = _xt32(oracle, capi, sensors, meshes)
    n = s.V * s.H
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for first, count in ((0, s.H), (37, 61)):
        tr.setShard(first, count)
        for flags in (0, capi.LS_SWEEP_DESKEW):
            k, p, h, r = _sweep(tr, pose, flags=flags, rays=True)
            assert k > 100
            for want_p in (True, False):
                for want_h in (True, False):
                    for want_r in (True, False):
                        ro = np.full((n, 8), np.float32(-7.5)) if want_r else None
                        rc, kh, ph, hh = tr.traceSweep(pose, flags=flags, points=want_p, hits=want_h, rays_out=ro)
                        assert rc == 0 and kh == k
                        assert (ph is None) if not want_p else _same_bits(ph, p)
                        assert (hh is None) if not want_h else np.array_equal(
                            np.stack([hh["ray"], hh["geom"], hh["prim"], hh["t"].view(np.uint32)], axis=1), h)
                        if want_r:
                            cols = np.arange(n) % s.H
                            mine = (cols >= first) & (cols < first + count)
                            assert _same_bits(ro[mine], r[mine]) and np.all(ro[~mine] == np.float32(-7.5))
    tr.close()
    t2 = make_tracer(capi, s)
    rc, k, p, h = t2.traceSweep(pose)
    assert rc == -1 and k == 0 and len(p) == 0 and len(h) == 0
    t2.close()
