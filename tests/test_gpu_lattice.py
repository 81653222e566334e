"""The hierarchy walks on lattice scenes, on the MI355X: k_trace_rays, k_occluded_rays, k_closest_points, k_project, k_trace_inst
(four-wide and binary), k_trace, k_sweep_rays and k_trace_rays_moving over tests/lattice_reference.py's terraces -- rays with exact
zeros in their direction that run in the face planes of hierarchy boxes, and one t on up to eight triangles that a seeded
permutation scattered over the ids, the leaves and the subtrees.

Every result is compared bit for bit: with the oracle's brute force, and -- where every float32 intermediate of the triangle test is
exact (lattice_reference.exact_closest's mask; test_lattice_cpu.py asserts that it covers the rays and that the rays tie) -- with the
exact integer rule as well.  The references are computed once per scene (test_lattice_cpu.lattice_case, frame_case) and shared."""
import dataclasses

import numpy as np
import pytest

import lattice_reference as LR
from conftest import make_tracer
from test_gpu_closest import _Brute, _query, _with_radius
from test_gpu_occlusion import _occluded_device
from test_gpu_rays import INV, _from_gid, _records
from test_gpu_sweep import FILL, _points, _same_bits, _sweep
from test_gpu_sweep_moving import _moving
from test_lattice_cpu import N, SEED, SENSOR_T, frame_case, frame_exact, lattice_case
from test_sweep_cpu import restate_rays
from test_sweep_moving_cpu import contributions, merge

pytestmark = pytest.mark.gpu

LEAF_SIZES = (1, 2, 4, 8)
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _brute_c(oracle, scene, rays):
    """test_gpu_rays._brute with its loop in the oracle's C: the same records"""
    t, gid = oracle.rays_bruteforce(rays, scene)
    return _from_gid(scene, t, gid)


def _add_all(tr, ml):
    for gid, v, e, A in ml:
        assert tr.addGeometry(f"g{gid}", v.shape[0], e.shape[0]) == gid
        tr.updateGeometry(f"g{gid}", A, v, e)
    assert tr.commitScene() == 0


def _trace_guarded(tr, rays):
    """ls_trace_rays into a filled buffer with one canary record behind the n results -> uint32 (n, 4)"""
    import torch
    n = rays.shape[0]
    d = torch.from_numpy(np.array(rays, np.float32).view(np.uint8).reshape(-1)).to("cuda:0")
    out = torch.full(((n + 1) * 16,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert tr.traceRaysDevice(d.data_ptr(), n, out.data_ptr()) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    b = out.cpu().numpy()
    assert np.all(b[n * 16:] == FILL), "a hit record written past the count"
    return b[:n * 16].view(np.uint32).reshape(n, 4), d


def _assert_records(got, want, what):
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:4]], want[bad[:4]])


# ---- 3. caller rays ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pose", list(LR.POSES))
def test_caller_rays_on_the_posed_terraces(oracle, capi, pose):
    """ls_trace_rays: (geom, prim, t bits) of the oracle's brute force, and of the exact rule where its mask holds; ls_occluded_rays:
    occluded exactly where the exact rule has a hit in [tmin, tmax]; at every leaf size"""
    c = lattice_case(oracle, pose)
    e, rays = c["exact"], c["rays"]
    want = _from_gid(c["scene"], c["oracle_t"], c["oracle_gid"])
    m = e["mask"]
    assert m.mean() >= 0.95 and np.array_equal(want[m], _from_gid(c["scene"], e["t"], e["gid"])[m])
    for g in LEAF_SIZES:
        tr = make_tracer(capi, c["sensor"], "bvh")
        tr.setOption(capi.LS_OPT_LEAF_SIZE, g)
        _add_all(tr, [(0, c["verts"], c["tris"], c["A"])])
        got, d_rays = _trace_guarded(tr, rays)
        _assert_records(got, want, (pose, g))
        rc, hits = tr.traceRays(rays)
        assert rc == 0 and np.array_equal(_records(hits), want)
        occ = _occluded_device(tr, d_rays, rays.shape[0], offset=3)
        assert np.array_equal(occ[m], (e["gid"] != LR.INV)[m]) and np.array_equal(occ, want[:, 1] != INV), (pose, g)
        assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
        tr.close()


@pytest.mark.parametrize("parts", [2, 17])
def test_terraces_split_into_geometries(oracle, capi, parts):
    """the triangles dealt into 2 geometries, and into 17 (two launch batches): a tie inside one hierarchy and a tie across
    geometries and batches meet in one ray; the lowest (geomID, primID) wins"""
    c = lattice_case(oracle, "identity")
    rays = c["rays"]
    ml = [(k, v, t, LR.POSES["identity"]) for k, (v, t) in enumerate(LR.split_scene(c["verts"], c["tris"], parts, SEED))]
    scene = oracle.assemble_scene(c["sensor"], ml)
    want = _brute_c(oracle, scene, rays)
    e = LR.exact_closest(rays, scene.verts, scene.tris)
    m = e["mask"]
    assert m.mean() >= 0.95 and np.array_equal(want[m], _from_gid(scene, e["t"], e["gid"])[m])
    assert np.array_equal(e["ties"], c["exact"]["ties"]) and len(set(want[:, 1]) - {INV}) == parts
    for g in (1, 4):
        tr = make_tracer(capi, c["sensor"], "bvh")
        tr.setOption(capi.LS_OPT_LEAF_SIZE, g)
        _add_all(tr, ml)
        got, d_rays = _trace_guarded(tr, rays)
        _assert_records(got, want, (parts, g))
        occ = _occluded_device(tr, d_rays, rays.shape[0])
        assert np.array_equal(occ, want[:, 1] != INV)
        assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
        tr.close()


def test_far_origins(oracle, capi):
    """The THROUGH rays moved back along their direction by 2^20: the origin's coordinates are still float32 lattice numbers, the
    slab test's products (lo - (o +- eps)) * 1e30 reach 1e36.  1e30 |o| stays finite up to about 3e8 m; beyond that the box test
    has no meaning and nothing is promised, so this test stops at 2^20 (about 1e6 m).  Against the oracle alone: t is near 2^20 and
    the triangle test's products round."""
    c = lattice_case(oracle, "identity")
    base = c["rays"][c["kind"] == LR.THROUGH]
    o = base[:, 0:3].astype(np.float64) - 2.0 ** 20 * base[:, 4:7].astype(np.float64)
    rays = base.copy()
    rays[:, 0:3] = o
    assert np.array_equal(rays[:, 0:3].astype(np.float64), o) and np.abs(o).max() >= 2.0 ** 20
    want = _brute_c(oracle, c["scene"], rays)
    hit = want[:, 1] != INV
    assert 0.5 < hit.mean() < 1.0
    for g in (1, 8):
        tr = make_tracer(capi, c["sensor"], "bvh")
        tr.setOption(capi.LS_OPT_LEAF_SIZE, g)
        _add_all(tr, [(0, c["verts"], c["tris"], c["A"])])
        got, d_rays = _trace_guarded(tr, rays)
        _assert_records(got, want, g)
        assert np.array_equal(_occluded_device(tr, d_rays, rays.shape[0]), hit)
        assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
        tr.close()


def _lattice_points(c, n_each=80):
    """lattice points in the sensor frame: above and below vertices (the 4 or 8 triangles around the vertex tie), above midpoints of
    level edges (two triangles tie), and points of a slope half-way between the two plateaus it joins -- equidistant from both; the
    slope they lie on is nearer, d = 0 on an edge that two triangles share"""
    rng = np.random.default_rng(SEED + 4)
    v = c["verts"].astype(np.float64)
    p = v[c["tris"].astype(np.int64)]
    level = p[:, 0, 2] == p[:, 1, 2]
    mid = 0.5 * (p[level, 0] + p[level, 1])
    h = LR.heights(N, SEED)
    slope = []
    for i in range(LR.BLOCK - 1, N - 1, LR.BLOCK):                          # the slope cells between vertex rows i and i + 1
        for j in range(N + 1):
            if h[i, j] != h[i + 1, j]:
                slope.append(((i + 0.5 - N // 2) * LR.SPACING, (j - N // 2) * LR.SPACING, (h[i, j] + h[i + 1, j]) * 0.5 * LR.HEIGHT_STEP))
    slope = np.array(slope)
    pick = lambda a: a[rng.choice(a.shape[0], min(n_each, a.shape[0]), replace=False)]      # noqa: E731
    up = np.array([0.0, 0.0, 0.5])
    pts = np.concatenate([pick(v) + up, pick(v) - up, pick(v), pick(mid) + up, pick(mid), pick(slope)])
    return (pts - SENSOR_T.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("radius", [np.inf, 0.25])
def test_nearest_points_on_lattice_points(oracle, capi, radius):
    c = lattice_case(oracle, "identity")
    pts = _with_radius(_lattice_points(c), radius)
    if ("closest", radius) not in _cache:
        _cache["closest", radius] = _Brute(capi, c["scene"])(pts)
    want = _cache["closest", radius]
    found = want[:, 4] != INV
    assert found.all() if radius == np.inf else (0 < np.count_nonzero(found) < found.size)
    for g in LEAF_SIZES:
        tr = make_tracer(capi, c["sensor"], "bvh")
        tr.setOption(capi.LS_OPT_LEAF_SIZE, g)
        _add_all(tr, [(0, c["verts"], c["tris"], c["A"])])
        got = _query(tr, pts)
        bad = np.nonzero(np.any(got != want, axis=1))[0]
        assert bad.size == 0, (g, bad[:10], got[bad[:3]], want[bad[:3]])
        assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
        tr.close()


# ---- 4. frames ----------------------------------------------------------------------------------------------------------------------

def _tables_tracer(capi, c, **options):
    st, ct, elev, sp, cp = c["tabs"]
    s = c["sensor"]
    tr = capi.Tracer.fromTables(st, ct, elev, sp, cp, 0.0, 1.0, s.Rinv, s.t)
    for k, val in options.items():
        tr.setOption(getattr(capi, k), val)
    _add_all(tr, [(0, c["verts"], c["tris"], LR.POSES["identity"])])
    return tr


def _frame_want(oracle, c):
    if "frame_want" not in _cache:
        _cache["frame_want"] = oracle.pack_points(c["oracle_t"], c["oracle_gid"], c["dirs"], LR.H_COLUMNS, c["scene"])
    return _cache["frame_want"]


FRAME_ENGINES = {
    "project-pipeline-0": dict(LS_OPT_ENGINE=2, LS_OPT_PIPELINE=0),
    "project-pipeline-2": dict(LS_OPT_ENGINE=2, LS_OPT_PIPELINE=2),
    "inst-wide-leaf-1": dict(LS_OPT_ENGINE=1, LS_OPT_LEAF_SIZE=1, LS_OPT_BVH_WIDE=1),
    "inst-wide-leaf-8": dict(LS_OPT_ENGINE=1, LS_OPT_LEAF_SIZE=8, LS_OPT_BVH_WIDE=1),
    "inst-binary-leaf-1": dict(LS_OPT_ENGINE=1, LS_OPT_LEAF_SIZE=1, LS_OPT_BVH_WIDE=0),
    "inst-binary-leaf-8": dict(LS_OPT_ENGINE=1, LS_OPT_LEAF_SIZE=8, LS_OPT_BVH_WIDE=0),
    "classic-leaf-1": dict(LS_OPT_ENGINE=1, LS_OPT_LEAF_SIZE=1, LS_OPT_BVH_INSTANCED=0),
    "classic-leaf-8": dict(LS_OPT_ENGINE=1, LS_OPT_LEAF_SIZE=8, LS_OPT_BVH_INSTANCED=0),
}


def _assert_frame(tr, want_t, want_gid, want_pts, want_hits, what):
    for f in range(2):
        rc, pts, hits = tr.traceScene(f)
        assert rc == 0
        t, gid = tr.denseHits()
        bad = np.nonzero((gid != want_gid) | (_bits(t) != _bits(want_t)))[0]
        assert bad.size == 0, (what, f, bad[:8], gid[bad[:8]], want_gid[bad[:8]], t[bad[:8]], want_t[bad[:8]])
        assert np.array_equal(np.asarray(pts).reshape(-1, 32), want_pts), (what, f)
        assert np.array_equal(np.stack([hits["ray"], hits["geom"], hits["prim"], hits["t"].view(np.uint32)], axis=1), want_hits), (what, f)


@pytest.mark.parametrize("engine", list(FRAME_ENGINES))
def test_frames_through_tables_with_exact_axes(oracle, capi, engine):
    """a raster whose tables hold exact 0, +-1 and +-0.70710677, the sensor on a lattice point above a vertex at a plateau's height:
    dense (t bits, id), hit records and points equal the oracle's brute force as bytes; on the axes the exact rule agrees"""
    c = frame_case(oracle)
    axis, e = frame_exact(c)
    assert np.array_equal(c["oracle_gid"][axis], e["gid"]) and np.array_equal(_bits(c["oracle_t"][axis]), _bits(e["t"]))
    want_pts, want_hits = _frame_want(oracle, c)
    assert want_pts.shape[0] > 2 * LR.H_COLUMNS
    opts = FRAME_ENGINES[engine]
    tr = _tables_tracer(capi, c, **opts)
    assert tr.getTotalRays() == c["dirs"].shape[0]
    _assert_frame(tr, c["oracle_t"], c["oracle_gid"], want_pts, want_hits, engine)
    if opts["LS_OPT_ENGINE"] == 1:
        assert tr.info(capi.LS_INFO_BVH_INSTANCED) == (0 if opts.get("LS_OPT_BVH_INSTANCED") == 0 else 2)
        if "LS_OPT_BVH_WIDE" in opts:
            assert tr.info(capi.LS_INFO_BVH_WIDE) == opts["LS_OPT_BVH_WIDE"]
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


@pytest.mark.parametrize("engine", ["projection", "bvh"])
def test_frame_of_a_descriptor_sensor_over_the_terraces(oracle, capi, engine):
    """h_begin = 0, identity pose: the ordinary zero of sinf in column 0, the 0-degree ring in a plateau's plane"""
    c = frame_case(oracle)
    s = c["sensor"]
    ml = [(0, c["verts"], c["tris"], LR.POSES["identity"])]
    if "descriptor" not in _cache:
        _cache["descriptor"] = oracle.trace_frame(s, ml)
    ref = _cache["descriptor"]
    assert ref["points"].shape[0] > s.H
    tr = make_tracer(capi, s, engine)
    _add_all(tr, ml)
    _assert_frame(tr, ref["t"], ref["gid"], ref["points"], ref["hits"], engine)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 5. scans -----------------------------------------------------------------------------------------------------------------------

def _quarter_turn(k):
    """yaw by k * 90 degrees: exact entries"""
    c, s = (1, 0, -1, 0)[k % 4], (0, 1, 0, -1)[k % 4]
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def _exact_table(seed, H=LR.H_COLUMNS):
    """float32 (H, 12) records [R | o]: yaw in 90-degree steps and a dyadic shift per column"""
    rng = np.random.default_rng(seed)
    out = np.zeros((H, 12), np.float32)
    for h in range(H):
        out[h] = LR.affine(_quarter_turn(int(rng.integers(0, 4))), rng.integers(-4, 5, 3) * (0.5, 0.5, 0.25))
    return out


def _expect(dense, dirs, H):
    """test_gpu_sweep._expect for directions that come from given tables"""
    hit = dense[dense[:, 1] != INV]
    r = hit[:, 0].astype(np.int64)
    xyz = hit[:, 3].view(np.float32)[:, None] * dirs[r]
    return hit, _points(xyz.astype(np.float32), (r // H).astype(np.uint32))


def test_sweep_with_exact_poses(oracle, capi):
    """ls_trace_scene_sweep: every column at a dyadic offset and a yaw of a multiple of 90 degrees -- the rays keep their exact zeros
    and stay on the lattice"""
    c = frame_case(oracle)
    H = LR.H_COLUMNS
    pose = _exact_table(SEED + 5)
    rays = restate_rays(c["dirs"], pose[np.arange(c["dirs"].shape[0]) % H])
    dense = _brute_c(oracle, c["scene"], rays)
    assert np.count_nonzero(np.any(dense[:, 1:] != _from_gid(c["scene"], c["oracle_t"], c["oracle_gid"])[:, 1:], axis=1)) > 100
    tr = _tables_tracer(capi, c)
    k, p, h, _ = _sweep(tr, pose)
    want_h, want_p = _expect(dense, c["dirs"], H)
    assert k == len(want_h) > 2 * H
    _assert_records(h, want_h, "sweep")
    assert _same_bits(p, want_p)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_moving_sweep_with_exact_motions(oracle, capi):
    """ls_trace_scene_sweep_moving: the terraces dealt into two geometries, one at rest, one on a motion table of exact quarter turns
    and dyadic shifts; the sensor at rest"""
    c = frame_case(oracle)
    H = LR.H_COLUMNS
    ml = [(k, v, t, LR.POSES["identity"]) for k, (v, t) in enumerate(LR.split_scene(c["verts"], c["tris"], 2, SEED))]
    motion = _exact_table(SEED + 6)
    rays = restate_rays(c["dirs"], np.tile(LR.POSES["identity"], (c["dirs"].shape[0], 1)))
    raster = dataclasses.replace(c["sensor"], h_count=H)                    # the tables' raster: contributions() asks it for H
    dense = merge(contributions(oracle, _brute_c, raster, ml, rays, {1: motion}))
    assert set(dense[:, 1]) >= {0, 1}
    st, ct, elev, sp, cp = c["tabs"]
    tr = capi.Tracer.fromTables(st, ct, elev, sp, cp, 0.0, 1.0, c["sensor"].Rinv, c["sensor"].t)
    _add_all(tr, ml)
    k, p, h = _moving(tr, None, {1: motion})
    want_h, want_p = _expect(dense, c["dirs"], H)
    assert k == len(want_h) > 2 * H
    _assert_records(h, want_h, "moving")
    assert _same_bits(p, want_p)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
