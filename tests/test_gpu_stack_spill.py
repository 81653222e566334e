"""Walks that cross the boundary between the 32 references a lane keeps in LDS (kStackLds) and the 64 it keeps in global memory
(kStackSpill), in the shipped library, on the MI355X: k_trace, k_trace_inst (four-wide and binary, one geometry with the LDS
treelet and two geometries), k_trace_rays, k_occluded_rays, k_closest_points and k_trace_rays_moving.  On ground + ben and the
synthetic grids no walk comes near 32 entries, so the push and pop code past the boundary -- it exists once per kernel -- never ran
under a test.

The scene is bvh_reference.staircase_deck: the radix tree peels the anchor and 24 single triangles ("stairs") off, one level each,
before it reaches a deck of 4096 triangles of ONE key (12 levels of ties, split by index).  The sensor looks up the z axis (8 rings
at 88.0 .. 89.9 degrees of elevation, 64 columns, identity pose): every ray enters every box on the way from the root to the first
deck leaf, so a walk that goes left first holds every right sibling of that path when it gets there.

The premise is asserted, not assumed:
  * k_trace: the CPU replay (oracle.fat_traverse_stats) of the downloaded nodes -- they are first compared with the reference, bit for
    bit -- reports its deepest stack: 36 at leaf size 1 (24 stairs + 12 levels of the deck), 4 past the LDS part; 23 at leaf size 2
    (two stairs share a leaf, the deck has 11 levels): the same scene below the boundary.
  * the other kernels have no replay: a float64 slab test on the reference tree shows that every test ray enters both child boxes of
    every node on the path from the root to leaf 0 (but the anchor's corner, which no ray looks at): 36 right siblings at leaf size
    1.  A binary walk holds those 36; a four-wide walk (a node's slots are its grandchildren, the nearest hit is walked on, the
    others are pushed: up to 2 per pair of staircase levels, up to 3 per pair of deck levels), restated in float64 on the reference's
    four-wide nodes, holds 41 (28 at leaf size 2).  The ray-query kernels and the default frame walk are four-wide.  Both counts stay
    below the capacity of 96.  The nearest-point walk is four-wide too and drops a slot only when its box lies beyond the best distance so far
    (none before the first leaf, without a radius): from a point below the deck it goes down the same path.

Every result is compared bit for bit: with the exhaustive device checker, the replay, or the brute-force / host loops of the
per-call suites (for the caller rays the loop of test_gpu_rays._brute runs in the oracle's C, oracle.rays_bruteforce, because every
ray meets all 4120 triangles here; the Python loop confirms it on a few rays)."""
import numpy as np
import pytest

import bvh_reference as B
from conftest import make_tracer
from test_gpu_closest import _Brute, _query, _with_radius
from test_gpu_rays import INV, _brute, _from_gid, _records
from test_gpu_sweep import _expect
from test_gpu_sweep_moving import _moving
from test_sweep_cpu import IDENTITY_POSE, restate_rays
from test_sweep_moving_cpu import contributions, merge

pytestmark = pytest.mark.gpu

LDS_ENTRIES, CAPACITY = 32, 96          # kStackLds, kStackLds + kStackSpill (csrc/ls_kernels.h)
_cache = {}


def _deck():
    if "deck" not in _cache:
        v, t, _ = B.staircase_deck()
        v.setflags(write=False)
        t.setflags(write=False)
        _cache["deck"] = (v, t)
    return _cache["deck"]


def _sensor(oracle):
    """identity pose, 8 rings at 88.0 .. 89.9 degrees of elevation, 64 columns: every ray within 2 degrees of +z"""
    if "sensor" not in _cache:
        eye = np.eye(3, dtype=np.float32).reshape(9)
        _cache["sensor"] = oracle.Sensor(uid="zenith", vertical=np.linspace(88.0, 89.9, 8).astype(np.float32), h_begin=np.float32(0.0),
                                         h_end=np.float32(360.0), h_count=64, R=eye, Rinv=eye.copy(), t=np.zeros(3, np.float32))
    return _cache["sensor"]


def _reference(g):
    """the reference tree over the deck's vertices as they are (the sensor frame of _sensor is the mesh's own)"""
    if ("ref", g) not in _cache:
        _cache["ref", g] = B.build(*_deck(), g)
    return _cache["ref", g]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_premise(g, origins, dirs, key=None):
    """every ray enters every box down to leaf 0 of the reference tree: a binary walk holds 36 references there at leaf size 1 (23 at
    leaf size 2), a four-wide walk -- restated in float64 on the reference's four-wide nodes -- 41 (28); at leaf size 1 both are past
    what the LDS part holds"""
    nodes = _reference(g)[0]
    ok, held = B.rays_enter_every_box_on_the_spine(nodes, origins, dirs)
    assert ok
    if key is None or (key, g) not in _cache:
        _cache[key, g] = B.wide_walk_holds(nodes, origins, dirs)
    wide = _cache[key, g]
    assert held == {1: 36, 2: 23}[g] and np.all(wide == {1: 41, 2: 28}[g]) and max(held, int(wide.max())) < CAPACITY
    if g == 1:
        assert held > LDS_ENTRIES and int(wide.min()) > LDS_ENTRIES
    return held


def _pose(oracle):
    """a 30 degree turn about z and a translation of (1, -2, 0)"""
    return oracle.affine_from_components(np.float32([1.0, -2.0, 0.0]), np.float32([0.0, 0.0, np.pi / 6]))


def _mesh_space(A, origins, dirs):
    """rays of the sensor frame (= the world: identity pose) in the mesh space of a geometry posed by [M | a]: float64"""
    M = np.asarray(A, np.float64).reshape(3, 4)
    Minv = np.linalg.inv(M[:, :3])
    return (np.asarray(origins, np.float64) - M[:, 3]) @ Minv.T, np.asarray(dirs, np.float64) @ Minv.T


def _caller_rays(n=2000, seed=3):
    """origins around (0, 0, -5), directions within 2 degrees of +z (not normalised), tmin 0, tmax +inf"""
    if "rays" not in _cache:
        rng = np.random.default_rng(seed)
        r = np.zeros((n, 8), np.float32)
        r[:, 0:3] = np.array([0.0, 0.0, -5.0]) + rng.uniform(-1.0, 1.0, (n, 3))
        tilt, phi = np.deg2rad(rng.uniform(0.0, 2.0, n)), rng.uniform(0.0, 2 * np.pi, n)
        d = np.stack([np.sin(tilt) * np.cos(phi), np.sin(tilt) * np.sin(phi), np.cos(tilt)], 1)
        r[:, 4:7] = d * rng.uniform(0.5, 2.0, n)[:, None]
        r[:, 7] = np.inf
        r.setflags(write=False)
        _cache["rays"] = r
    return _cache["rays"]


def _brute_c(oracle, scene, rays):
    """test_gpu_rays._brute with its loop in the oracle's C: the same records"""
    t, gid = oracle.rays_bruteforce(rays, scene)
    return _from_gid(scene, t, gid)


def _scene_of(oracle, A=None):
    v, t = _deck()
    return oracle.assemble_scene(_sensor(oracle), [(0, v, t, oracle.IDENTITY_AFFINE if A is None else A)])


def _tracer(oracle, capi, g, A=None, **options):
    v, t = _deck()
    tr = make_tracer(capi, _sensor(oracle), "bvh")
    tr.setOption(capi.LS_OPT_LEAF_SIZE, g)
    for k, val in options.items():
        tr.setOption(getattr(capi, k), val)
    assert tr.addGeometry("deck", v.shape[0], t.shape[0]) == 0
    tr.updateGeometry("deck", oracle.IDENTITY_AFFINE if A is None else A, v, t)
    return tr


# ---- k_trace ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [1, 2])
def test_classic_walk_past_the_lds_stack(oracle, capi, g):
    s = _sensor(oracle)
    tr = _tracer(oracle, capi, g, LS_OPT_BVH_INSTANCED=0, LS_OPT_COUNT_VISITS=1)
    assert tr.commitScene() == 0 and tr.info(capi.LS_INFO_BVH_INSTANCED) == 0
    nodes, tri, leaf = tr.downloadBvh()
    want, rec, _, _ = _reference(g)
    assert leaf == g and np.array_equal(nodes.view(np.uint32), want.view(np.uint32)) and np.array_equal(tri["gid"], rec["gid"])
    dirs = oracle.ray_dirs(s)
    held = _assert_premise(g, np.zeros((1, 3)), dirs)
    rc, _, _ = tr.traceScene(0)
    assert rc == 0
    t, gid = tr.denseHits()
    t2, gid2, stats = oracle.fat_traverse_stats(nodes, tri, g, dirs)
    print(f"leaf size {g}: deepest stack of the replay {int(stats[2])}, right siblings on the path to leaf 0 {held}")
    assert int(stats[2]) == held
    if g == 1:
        assert int(stats[2]) > LDS_ENTRIES
    bt, bg = tr.bruteForce()
    assert np.all(gid == 0) and np.all(t > 0)                                # the deck's first pair shares every t: the lower id wins
    assert np.array_equal(gid, bg) and np.array_equal(_bits(t), _bits(bt))
    assert np.array_equal(gid, gid2) and np.array_equal(_bits(t), _bits(t2))
    assert tr.visitCounts() == (int(stats[0]), int(stats[1]))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- k_trace_inst ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("wide", [1, 0])
@pytest.mark.parametrize("geoms", [1, 2])
def test_instanced_walk_past_the_lds_stack(oracle, capi, meshes, geoms, wide, g):
    """the deck turned by 30 degrees about z and moved by (1, -2, 0) -- alone (the binary walk stages its LDS treelet), and next to
    ben.stl posed off the axis"""
    s = _sensor(oracle)
    A = _pose(oracle)
    _assert_premise(g, *_mesh_space(A, np.zeros((1, 3)), oracle.ray_dirs(s)))
    tr = _tracer(oracle, capi, g, A, LS_OPT_BVH_WIDE=wide)
    if geoms == 2:
        bv, bt = meshes["ben"]
        assert tr.addGeometry("face", bv.shape[0], bt.shape[0]) == 1
        tr.updateGeometry("face", oracle.affine_from_components(np.float32([40.0, 30.0, 60.0]), np.float32([0.3, 0.0, 1.0])), bv, bt)
    assert tr.commitScene() == 0 and tr.info(capi.LS_INFO_BVH_INSTANCED) == 2
    nodes, _, _, leaf = tr.downloadHierarchy("deck", wide=bool(wide))
    assert leaf == g and np.array_equal(nodes.view(np.uint32), _reference(g)[0].view(np.uint32))
    rc, _, _ = tr.traceScene(0)
    assert rc == 0 and tr.info(capi.LS_INFO_BVH_WIDE) == wide
    t, gid = tr.denseHits()
    bt_, bg = tr.bruteForce()
    assert np.all(gid == 0)
    assert np.array_equal(gid, bg) and np.array_equal(_bits(t), _bits(bt_))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- k_trace_rays, k_occluded_rays ------------------------------------------------------------------------------------------------

def _closest_want(oracle):
    """the brute force over the caller rays, once; the Python loop of the per-call suite agrees on the first rays"""
    if "want" not in _cache:
        rays, scene = _caller_rays(), _scene_of(oracle)
        want = _brute_c(oracle, scene, rays)
        assert np.array_equal(want[:3], _brute(oracle, scene, rays[:3]))
        want.setflags(write=False)
        _cache["want"] = want
    return _cache["want"]


@pytest.mark.parametrize("g", [1, 2])
def test_caller_rays_past_the_lds_stack(oracle, capi, g):
    rays = _caller_rays()
    _assert_premise(g, rays[:, 0:3], rays[:, 4:7], "caller")
    want = _closest_want(oracle)
    assert np.all(want[:, 1] == 0) and np.all(want[:, 2] == 0)              # every ray meets the deck's first pair first
    tr = _tracer(oracle, capi, g)
    assert tr.commitScene() == 0
    rc, hits = tr.traceRays(rays)
    assert rc == 0 and np.array_equal(_records(hits), want)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


@pytest.mark.parametrize("g", [1, 2])
def test_occlusion_rays_pop_from_the_spill_and_go_on(oracle, capi, g):
    """tmin past half of the deck: the leaves the walk reaches first fail the range, it has to pop what it spilled and go on until a
    triangle counts; tmin past everything: it pops all of it and finds nothing"""
    base = _caller_rays()
    _assert_premise(g, base[:, 0:3], base[:, 4:7], "caller")
    scene = _scene_of(oracle)
    half = base.copy()
    half[:, 3] = (np.float32(0.28) - base[:, 2]) / base[:, 6]               # where the ray crosses z = 0.28: the deck spans 0.25 .. 0.3125
    beyond = base.copy()
    beyond[:, 3] = 600.0
    tr = _tracer(oracle, capi, g)
    assert tr.commitScene() == 0
    for rays, expect_any in ((half, True), (beyond, False)):
        records = _brute_c(oracle, scene, rays)
        assert np.array_equal(records[:2], _brute(oracle, scene, rays[:2]))
        want = records[:, 1] != INV
        assert want.all() if expect_any else not want.any()
        if expect_any:   # what counts first lies past the pairs below z = 0.28
            assert np.all((records[:, 2] > 1000) & (records[:, 2] < B.DECK))
        rc, occ = tr.occludedRays(rays)
        assert rc == 0 and np.array_equal(occ, want)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- k_closest_points ---------------------------------------------------------------------------------------------------------------

def _points(n=2000, seed=8):
    """near the axis, z in [-1, 130]: a fifth below and inside the deck (the deep walks), the rest up the staircase"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-2.0, 2.0, (n, 3))
    low = n // 5
    p[:low, 2] = rng.uniform(-1.0, 0.32, low)
    p[low:, 2] = rng.uniform(0.32, 130.0, n - low)
    return p.astype(np.float32)


@pytest.mark.parametrize("radius", [np.inf, 0.01])
@pytest.mark.parametrize("part", range(4))
def test_nearest_points_past_the_lds_stack(oracle, capi, part, radius):
    """2000 points, 500 a case (the host loop of test_gpu_closest takes 5 ms a point on this scene), both leaf sizes in each"""
    pts = _with_radius(_points()[part::4], radius)
    want = _Brute(capi, _scene_of(oracle))(pts)
    found = want[:, 4] != INV
    assert found.all() if radius == np.inf else (0 < np.count_nonzero(found) < found.size)
    for g in (1, 2):
        tr = _tracer(oracle, capi, g)
        assert tr.commitScene() == 0
        got = _query(tr, pts)
        bad = np.nonzero(np.any(got != want, axis=1))[0]
        assert bad.size == 0, (g, bad[:10], got[bad[:3]], want[bad[:3]])
        assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
        tr.close()


# ---- k_trace_rays_moving --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [1, 2])
def test_moving_deck_past_the_lds_stack(oracle, capi, g):
    """ls_trace_scene_sweep_moving, the sensor at rest, the deck on a small constant twist about z (0.05 rad and half a unit over the
    turn: the rays stay well inside every triangle)"""
    s = _sensor(oracle)
    v, t = _deck()
    if "moving" not in _cache:
        motion = capi.motion_constant_twist((3.0, -4.0, 0.0), (0.0, 0.0, 0.5), np.zeros(3), 0.0, 0.1 / s.H, s.H)
        rays = restate_rays(oracle.ray_dirs(s), np.tile(IDENTITY_POSE, (s.V * s.H, 1)))
        contrib = contributions(oracle, _brute_c, s, [(0, v, t, oracle.IDENTITY_AFFINE)], rays, {0: motion})
        for a in (motion, rays, contrib[0]):
            a.setflags(write=False)
        _cache["moving"] = (motion, rays, contrib)
    motion, rays, contrib = _cache["moving"]
    # the rays the deck sees (through the inverse of its motion) enter every box down to leaf 0
    from test_sweep_moving_cpu import restate_motion_rays
    seen = restate_motion_rays(rays, motion[np.arange(rays.shape[0]) % s.H])
    _assert_premise(g, seen[:, 0:3], seen[:, 4:7])
    dense = merge(contrib)
    assert np.all(dense[:, 1] == 0) and np.all(dense[:, 2] == 0)
    tr = _tracer(oracle, capi, g)
    assert tr.commitScene() == 0
    k, p, h = _moving(tr, None, {0: motion})
    want_h, want_p = _expect(oracle, s, dense, rays)
    assert k == len(want_h) == s.V * s.H and np.array_equal(h, want_h)
    assert np.array_equal(p.view(np.uint32), want_p.view(np.uint32))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
